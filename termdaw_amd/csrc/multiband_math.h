// multiband_math.h -- host arithmetic of the multiband vertex (include/termdaw_amd.h td_graph_add_multiband): the
// five coefficient sets of the Linkwitz-Riley crossover (the RBJ low-pass and high-pass of eq_math.h at lo_hz and hi_hz, Q =
// sqrt(0.5), and the all-pass A2 at hi_hz), the detectors' aA and aR, the range checks (shared by the C ABI and the Lua
// front-end), and the crossover's 18x18 one-frame operator with its powers.  No HIP call.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "eq_math.h"

namespace tde {
namespace multiband {

constexpr int kSets = 5;                       // L1, H1, L2, H2, A2: (b0, b1, b2, a1, a2) each
constexpr int kParams = 5 * kSets + 2;         // ... then aA, aR
constexpr int kBiquads = 9;                    // per channel, in the definition's order: L1 L1 A2 | H1 H1 | L2 L2 | H2 H2
constexpr int kWords = 2 * kBiquads;           // (s1, s2) of each: the crossover's state of one channel
// the coefficient set of biquad i, and the biquad whose output it filters (-1: the input x)
constexpr int kSetOf[kBiquads] = {0, 0, 4, 1, 1, 2, 2, 3, 3};
constexpr int kFeeds[kBiquads] = {-1, 0, 1, -1, 3, 4, 5, 4, 7};
// the 2x2 blocks (row biquad, column biquad) of the operator that are not zero: biquad `col` reaches biquad `row`
constexpr int kBlocks = 23;
constexpr int kBlockRow[kBlocks] = {0, 1, 1, 2, 2, 2, 3, 4, 4, 5, 5, 5, 6, 6, 6, 6, 7, 7, 7, 8, 8, 8, 8};
constexpr int kBlockCol[kBlocks] = {0, 0, 1, 0, 1, 2, 3, 3, 4, 3, 4, 5, 3, 4, 5, 6, 3, 4, 7, 3, 4, 7, 8};

// the RBJ all-pass at (f, q): b = (1 - alpha, -2 cos w0, 1 + alpha) / (1 + alpha), the low-pass' a1 and a2
inline void allpass(size_t sr, double freq_hz, double q, double out[5]) {
    const double w0 = 2.0 * M_PI * freq_hz / (double)sr;
    const double cw = cos(w0), sw = sin(w0);
    const double alpha = sw / (2.0 * q), a0 = 1.0 + alpha;
    out[0] = (1.0 - alpha) / a0; out[1] = (-2.0 * cw) / a0; out[2] = (1.0 + alpha) / a0;
    out[3] = (-2.0 * cw) / a0; out[4] = (1.0 - alpha) / a0;
}

// out[5 s .. 5 s + 4] = (b0, b1, b2, a1, a2) of set s = L1, H1, L2, H2, A2;  out[25] = aA;  out[26] = aR
inline void params(size_t sr, float lo_hz, float hi_hz, float attack_ms, float release_ms, double* out) {
    const double q = sqrt(0.5);
    eq::coefficients_f64(0, sr, (double)lo_hz, q, 0.0, out);
    eq::coefficients_f64(1, sr, (double)lo_hz, q, 0.0, out + 5);
    eq::coefficients_f64(0, sr, (double)hi_hz, q, 0.0, out + 10);
    eq::coefficients_f64(1, sr, (double)hi_hz, q, 0.0, out + 15);
    allpass(sr, (double)hi_hz, q, out + 20);
    out[25] = attack_ms > 0.0f ? exp(-1.0 / ((double)attack_ms * (double)sr / 1000.0)) : 0.0;
    out[26] = exp(-1.0 / ((double)release_ms * (double)sr / 1000.0));
}

// nullptr, or what is wrong: the message names the parameter (a NaN fails every comparison)
inline const char* check(size_t sr, float lo_hz, float hi_hz, const float threshold_db[3], const float ratio[3], float attack_ms,
                         float release_ms, float knee_db, const float makeup_db[3]) {
    if (sr == 0) return "the sample rate is 0";
    if (!(lo_hz >= 40.0f && lo_hz <= 3.0e38f)) return "lo_hz must be at least 40 Hz";
    if (!((double)hi_hz <= 0.45 * (double)sr && hi_hz >= -3.0e38f)) return "hi_hz must not exceed 0.45 of the sample rate";
    if (!((double)hi_hz >= 2.0 * (double)lo_hz)) return "hi_hz must be at least twice lo_hz";
    for (int b = 0; b < 3; ++b)
        if (!(threshold_db[b] >= -60.0f && threshold_db[b] <= 0.0f)) return "threshold_db must lie in [-60, 0] dB in every band";
    for (int b = 0; b < 3; ++b)
        if (!(ratio[b] >= 1.0f && ratio[b] <= 1000.0f)) return "ratio must lie in [1, 1000] in every band";
    if (!(attack_ms >= 0.0f && attack_ms <= 1000.0f)) return "attack_ms must lie in [0, 1000] ms";
    if (!(release_ms >= 1.0f && release_ms <= 10000.0f)) return "release_ms must lie in [1, 10000] ms";
    if (!(knee_db >= 0.0f && knee_db <= 40.0f)) return "knee_db must lie in [0, 40] dB";
    for (int b = 0; b < 3; ++b)
        if (!(makeup_db[b] >= -40.0f && makeup_db[b] <= 40.0f)) return "makeup_db must lie in [-40, 40] dB in every band";
    return nullptr;
}

// ---- the operator: z[n] = A z[n-1] + c x[n] over the 18 state words of a channel ----
struct M18 { long double m[kWords][kWords]; };

// one frame of the cascade in long double (the definition's order), from state z with input x
inline void frame(const double* co, long double z[kWords], long double x) {
    long double y[kBiquads];
    for (int i = 0; i < kBiquads; ++i) {
        const double* c = co + 5 * kSetOf[i];
        const long double u = kFeeds[i] < 0 ? x : y[kFeeds[i]];
        long double &s1 = z[2 * i], &s2 = z[2 * i + 1];
        y[i] = (long double)c[0] * u + s1;
        s1 = ((long double)c[1] * u - (long double)c[3] * y[i]) + s2;
        s2 = (long double)c[2] * u - (long double)c[4] * y[i];
    }
}
// A: column j is one frame from the unit state e_j with x = 0
inline M18 op(const double* co) {
    M18 a;
    for (int j = 0; j < kWords; ++j) {
        long double z[kWords] = {};
        z[j] = 1.0L;
        frame(co, z, 0.0L);
        for (int i = 0; i < kWords; ++i) a.m[i][j] = z[i];
    }
    return a;
}
inline M18 mul(const M18& a, const M18& b) {
    M18 r;
    for (int i = 0; i < kWords; ++i)
        for (int j = 0; j < kWords; ++j) {
            long double s = 0.0L;
            for (int k = 0; k < kWords; ++k) s += a.m[i][k] * b.m[k][j];
            r.m[i][j] = s;
        }
    return r;
}
// a^n, n >= 1: square and multiply from the lowest bit
inline M18 power(M18 a, uint32_t n) {
    M18 r = a;
    bool have = false;
    for (; n; n >>= 1) {
        if (n & 1u) { r = have ? mul(r, a) : a; have = true; }
        if (n > 1u) a = mul(a, a);
    }
    return r;
}
// the 23 blocks of p, each rounded once: out[4 b ..] = (p00, p01, p10, p11) of block b
inline void store(const M18& p, double* out) {
    for (int b = 0; b < kBlocks; ++b) {
        const int r = 2 * kBlockRow[b], c = 2 * kBlockCol[b];
        out[4 * b] = (double)p.m[r][c]; out[4 * b + 1] = (double)p.m[r][c + 1];
        out[4 * b + 2] = (double)p.m[r + 1][c]; out[4 * b + 3] = (double)p.m[r + 1][c + 1];
    }
}
// pw[k] = A^(run 2^k), k = 0 .. 7; a_tile = A^(256 run); pwc[k] = A^(256 run chunk 2^k) -- the dense matrix squared in long
// double, the blocks rounded once (eq::powers' way).  Each of the three: [..][kBlocks * 4] doubles.
inline void powers(const double* co, uint32_t run, uint32_t chunk, double (*pw)[kBlocks * 4], double* a_tile, double (*pwc)[kBlocks * 4]) {
    M18 p = power(op(co), run);
    for (int k = 0; k < 8; ++k) {
        store(p, pw[k]);
        p = mul(p, p);
    }
    store(p, a_tile);
    p = power(p, chunk);
    for (int k = 0; k < 8; ++k) {
        store(p, pwc[k]);
        p = mul(p, p);
    }
}

}  // namespace multiband
}  // namespace tde
