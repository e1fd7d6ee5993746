// loudness.h -- the host side of the loudness meter (ITU-R BS.1770-4, EBU Tech 3341 / 3342): the K-weighting
// coefficients and the true-peak FIR for a rate, the tiling of a signal for k_loudness, its descriptor, and the gating,
// short-term windows, loudness range and dB figures computed in double from what the kernel leaves.  Header-only: the
// host engine (engine.cpp) is all that includes it.
#pragma once
#include <math.h>
#include <string.h>

#include <cmath>

#include <algorithm>
#include <limits>
#include <vector>

#include "kernels.h"

namespace tde {
namespace loud {
using namespace tdk;

constexpr double kForget = 1e-12;   // the warm-up in front of a tile: r^warm <= kForget for the cascade's largest pole radius r
constexpr size_t kTileHops = 4;     // hops per tile
constexpr double kKaiserBeta = 3.5;

// BS.1770-4's two stages for any rate fs, from the bilinear forms that reproduce its 48 kHz table: kw = shelf b0 b1 b2 a1 a2,
// then high-pass b0 b1 b2 a1 a2 (a0 = 1).
inline void kweight(double fs, double kw[10]) {
    {
        const double f0 = 1681.974450955533, G = 3.999843853973347, Q = 0.7071752369554196;
        const double K = tan(M_PI * f0 / fs), Vh = pow(10.0, G / 20.0), Vb = pow(Vh, 0.4996667741545416);
        const double a0 = 1.0 + K / Q + K * K;
        kw[0] = (Vh + Vb * K / Q + K * K) / a0;
        kw[1] = 2.0 * (K * K - Vh) / a0;
        kw[2] = (Vh - Vb * K / Q + K * K) / a0;
        kw[3] = 2.0 * (K * K - 1.0) / a0;
        kw[4] = (1.0 - K / Q + K * K) / a0;
    }
    {
        const double f0 = 38.13547087602444, Q = 0.5003270373238773;
        const double K = tan(M_PI * f0 / fs), a0 = 1.0 + K / Q + K * K;
        kw[5] = 1.0;
        kw[6] = -2.0;
        kw[7] = 1.0;
        kw[8] = 2.0 * (K * K - 1.0) / a0;
        kw[9] = (1.0 - K / Q + K * K) / a0;
    }
}
inline size_t hop(size_t sr) { return (size_t)llround((double)sr / 10.0); }
inline size_t phases(size_t sr) { return sr < 96000 ? 4 : sr < 192000 ? 2 : 1; }

// The true-peak interpolator: phase p of `phases(sr)`, tap i weighs x[m - 5 + i] in the point at m + p / P.  A Kaiser-windowed
// (beta 3.5, half-width 6 frames) sinc cut off at the input's Nyquist rate: sinc vanishes at every non-zero integer, so phase 0
// is the unit impulse and the samples themselves are among the points examined.
inline void fir(size_t sr, float out[4][kLoudTaps]) {
    const size_t P = phases(sr);
    memset(out, 0, sizeof(float) * 4 * kLoudTaps);
    for (size_t p = 0; p < P; ++p)
        for (size_t i = 0; i < kLoudTaps; ++i) {
            const double t = 5.0 - (double)i + (double)p / (double)P;
            if (p == 0) { out[p][i] = t == 0.0 ? 1.0f : 0.0f; continue; }
            const double u = t / 6.0, s = sin(M_PI * t) / (M_PI * t);
            const double w = std::cyl_bessel_i(0.0, kKaiserBeta * sqrt(std::max(0.0, 1.0 - u * u))) / std::cyl_bessel_i(0.0, kKaiserBeta);
            out[p][i] = (float)(s * w);
        }
}

// The cascade's state matrix for zero input: state (s1, s2) of the shelf, (t1, t2) of the high-pass (transposed direct form II).
inline void state_matrix(const double kw[10], double A[16]) {
    const double a1 = kw[3], a2 = kw[4], b0 = kw[5], b1 = kw[6], b2 = kw[7], c1 = kw[8], c2 = kw[9];
    const double M[16] = {-a1, 1.0, 0.0, 0.0,
                          -a2, 0.0, 0.0, 0.0,
                          b1 - c1 * b0, 0.0, -c1, 1.0,
                          b2 - c2 * b0, 0.0, -c2, 0.0};
    memcpy(A, M, sizeof M);
}
inline void matmul(const double* X, const double* Y, double* Z) {
    double T[16];
    for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c) {
            double a = 0.0;
            for (int k = 0; k < 4; ++k) a += X[r * 4 + k] * Y[k * 4 + c];
            T[r * 4 + c] = a;
        }
    memcpy(Z, T, sizeof T);
}
inline double pole_radius(double a1, double a2) {   // max |z| over the roots of z^2 + a1 z + a2
    const double disc = a1 * a1 - 4.0 * a2;
    if (disc < 0.0) return sqrt(a2);
    const double s = sqrt(disc);
    return std::max(fabs((-a1 + s) / 2.0), fabs((-a1 - s) / 2.0));
}

// A signal as the kernel sees it; frames and rate are the render's.
struct Signal {
    const void* pcm = nullptr;
    uint32_t kind = 0;      // 0 int16, 1 int32, 2 f32
    double scale = 1.0;
    size_t frames = 0, sr = 0;
};
// 1 / 2^(bits - 1), as a WAV reader scales a word (8-bit renders hold +-127 in int16 words)
inline double word_scale(int bits) { return ldexp(1.0, -(bits - 1)); }

// Fills d for s (everything but the device pointers); 0 and *why set when the rate cannot be measured.
inline int describe(const Signal& s, LoudDesc& d, const char** why) {
    memset(&d, 0, sizeof d);
    const size_t H = hop(s.sr);
    if (s.sr < 8000 || s.sr > 768000) { *why = "loudness: the sample rate must lie in [8000, 768000] Hz"; return 0; }
    if (s.frames > 0xFFFFFFFFu) { *why = "loudness: at most 2^32 - 1 frames per signal"; return 0; }
    kweight((double)s.sr, d.kw);
    const double r = std::max(pole_radius(d.kw[3], d.kw[4]), pole_radius(d.kw[8], d.kw[9]));
    if (!(r < 1.0)) { *why = "loudness: the K-weighting filter is unstable at this rate"; return 0; }
    const size_t warm = (size_t)ceil(log(kForget) / log(r));
    const size_t tile = kTileHops * H;
    const size_t run = (warm + tile + kThreads - 1) / kThreads;
    if (run > H) { *why = "loudness: the warm-up is too long for this rate"; return 0; }
    d.kind = s.kind;
    d.frames = (uint32_t)s.frames;
    d.hop = (uint32_t)H;
    d.tile = (uint32_t)tile;
    d.run = (uint32_t)run;
    d.n_tiles = (uint32_t)((s.frames + tile - 1) / tile);
    d.phases = (uint32_t)phases(s.sr);
    d.scale = s.scale;
    double A[16], P[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    state_matrix(d.kw, A);
    for (size_t e = run; e; e >>= 1) {   // A^run by squaring
        if (e & 1) matmul(P, A, P);
        matmul(A, A, A);
    }
    memcpy(d.pw[0], P, sizeof P);
    for (int k = 1; k < 8; ++k) matmul(d.pw[k - 1], d.pw[k - 1], d.pw[k]);
    fir(s.sr, d.fir);
    return 1;
}
inline size_t hops(const LoudDesc& d) { return d.hop ? d.frames / d.hop : 0; }

inline double lufs(double power) { return -0.691 + 10.0 * log10(power); }
inline double db(uint32_t bits) {
    float v;
    memcpy(&v, &bits, 4);
    return 20.0 * log10((double)v);
}
// The eight figures of one signal from its hop sums (sum[h * 2 + c]) and peak words; the 400 ms block series into *mom.
inline void figures(const double* sum, size_t nh, size_t H, const uint32_t peak[2], size_t frames, size_t sr, double out[8],
                    std::vector<double>* mom) {
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    std::vector<double> z(nh);   // sum over the channels of the hop's mean square
    bool bad = false;
    for (size_t h = 0; h < nh; ++h) {
        z[h] = sum[h * 2] / (double)H + sum[h * 2 + 1] / (double)H;
        bad |= z[h] != z[h];
    }
    float tp, sp;
    memcpy(&tp, &peak[0], 4);
    memcpy(&sp, &peak[1], 4);
    out[6] = (double)frames;
    out[7] = (double)sr;
    mom->clear();
    if (bad || tp != tp || sp != sp) {
        for (int i = 0; i < 6; ++i) out[i] = nan;
        for (size_t j = 0; j + 4 <= nh; ++j) mom->push_back(nan);
        return;
    }
    // gating blocks: hops j .. j + 3
    std::vector<double> P;
    for (size_t j = 0; j + 4 <= nh; ++j) P.push_back((z[j] + z[j + 1] + z[j + 2] + z[j + 3]) / 4.0);
    double m_max = -inf, s_max = -inf;
    for (double p : P) { mom->push_back(lufs(p)); m_max = std::max(m_max, mom->back()); }
    double acc = 0.0;
    size_t n = 0;
    for (double p : P)
        if (lufs(p) > -70.0) { acc += p; ++n; }
    double integrated = -inf;
    if (n) {
        const double rel = lufs(acc / (double)n) - 10.0;
        acc = 0.0;
        n = 0;
        for (double p : P) {
            const double l = lufs(p);
            if (l > -70.0 && l > rel) { acc += p; ++n; }
        }
        if (n) integrated = lufs(acc / (double)n);
    }
    // short-term windows: 30 hops at a step of one hop; the loudness range over them (EBU Tech 3342)
    std::vector<double> S;
    for (size_t k = 0; k + 30 <= nh; ++k) {
        double a = 0.0;
        for (size_t i = 0; i < 30; ++i) a += z[k + i];
        S.push_back(a / 30.0);
    }
    acc = 0.0;
    n = 0;
    for (double p : S) {
        s_max = std::max(s_max, lufs(p));
        if (lufs(p) > -70.0) { acc += p; ++n; }
    }
    double lra = 0.0;
    if (n) {
        const double rel = lufs(acc / (double)n) - 20.0;
        std::vector<double> v;
        for (double p : S) {
            const double l = lufs(p);
            if (l > -70.0 && l > rel) v.push_back(l);
        }
        if (!v.empty()) {
            std::sort(v.begin(), v.end());
            const double last = (double)(v.size() - 1);
            lra = v[(size_t)floor(last * 0.95 + 0.5)] - v[(size_t)floor(last * 0.10 + 0.5)];
        }
    }
    out[0] = integrated;
    out[1] = m_max;
    out[2] = s_max;
    out[3] = lra;
    out[4] = db(peak[0]);
    out[5] = db(peak[1]);
}

}  // namespace loud
}  // namespace tde
