// eq_math.h -- host arithmetic of the parametric EQ vertex (include/termdaw_amd.h td_graph_add_eq): the RBJ
// "Audio EQ Cookbook" coefficients in f64, the largest gain of the response in closed form, and the powers of the state
// matrix the scan kernels join lanes and tiles with (long double, rounded once to f64).  No HIP call.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

namespace tde {
namespace eq {

constexpr int kKinds = 7;   // TD_EQ_LOWPASS .. TD_EQ_HIGHSHELF
inline const char* const* kind_names() {   // (the script line's names, in the constants' order)
    static const char* const n[kKinds] = {"lowpass", "highpass", "bandpass", "notch", "peak", "lowshelf", "highshelf"};
    return n;
}
inline bool kind_has_gain(int kind) { return kind >= 4; }
// nullptr: fine, otherwise the reason.  rate_free: only the ranges that do not depend on the rate -- what a script line can be held
// to, whose render rate comes with the graph (freq_hz's upper end fails when the graph is built)
inline const char* check(size_t sr, int kind, float freq_hz, float q, float gain_db, bool rate_free = false) {
    if (!(kind >= 0 && kind < kKinds)) return "kind must be one of TD_EQ_LOWPASS .. TD_EQ_HIGHSHELF (0 .. 6)";
    if (!rate_free && !sr) return "the sample rate must be positive";
    if (!(freq_hz >= 10.0f && (rate_free || 20.0 * (double)freq_hz <= 9.0 * (double)sr))) return "freq_hz must lie in [10, 0.45 sr] Hz";
    if (!(q >= 0.1f && q <= 20.0f)) return "q must lie in [0.1, 20]";
    if (kind_has_gain(kind) && !(gain_db >= -24.0f && gain_db <= 24.0f)) return "gain_db must lie in [-24, 24] dB";
    return nullptr;
}

// (b0, b1, b2, a1, a2), normalised by a0.  f64 from the f32 parameters, widened; 1 - cos w0 as 2 sin^2(w0 / 2), which has no
// cancellation at low frequencies.
// (the f64 form: the vocoder vertex' band centres are f64, vocoder_math.h; the f32 form below widens and calls it)
inline void coefficients_f64(int kind, size_t sr, double freq_hz, double q, double gain_db, double out[5]) {
    const double w0 = 2.0 * M_PI * freq_hz / (double)sr;
    const double cw = cos(w0), sw = sin(w0), sh = sin(0.5 * w0);
    const double omc = 2.0 * sh * sh;   // 1 - cos w0
    const double opc = 1.0 + cw;
    const double alpha = sw / (2.0 * q);
    const double A = kind_has_gain(kind) ? pow(10.0, gain_db / 40.0) : 1.0;
    double b0 = 1.0, b1 = 0.0, b2 = 0.0, a0 = 1.0, a1 = 0.0, a2 = 0.0;
    switch (kind) {
        case 0: b0 = omc / 2.0; b1 = omc; b2 = omc / 2.0; a0 = 1.0 + alpha; a1 = -2.0 * cw; a2 = 1.0 - alpha; break;
        case 1: b0 = opc / 2.0; b1 = -opc; b2 = opc / 2.0; a0 = 1.0 + alpha; a1 = -2.0 * cw; a2 = 1.0 - alpha; break;
        case 2: b0 = alpha; b1 = 0.0; b2 = -alpha; a0 = 1.0 + alpha; a1 = -2.0 * cw; a2 = 1.0 - alpha; break;
        case 3: b0 = 1.0; b1 = -2.0 * cw; b2 = 1.0; a0 = 1.0 + alpha; a1 = -2.0 * cw; a2 = 1.0 - alpha; break;
        case 4:
            b0 = 1.0 + alpha * A; b1 = -2.0 * cw; b2 = 1.0 - alpha * A;
            a0 = 1.0 + alpha / A; a1 = -2.0 * cw; a2 = 1.0 - alpha / A;
            break;
        case 5: {
            const double s = 2.0 * sqrt(A) * alpha, p = A + 1.0, m = A - 1.0;
            b0 = A * ((p - m * cw) + s); b1 = 2.0 * A * (m - p * cw); b2 = A * ((p - m * cw) - s);
            a0 = (p + m * cw) + s; a1 = -2.0 * (m + p * cw); a2 = (p + m * cw) - s;
            break;
        }
        default: {
            const double s = 2.0 * sqrt(A) * alpha, p = A + 1.0, m = A - 1.0;
            b0 = A * ((p + m * cw) + s); b1 = -2.0 * A * (m + p * cw); b2 = A * ((p + m * cw) - s);
            a0 = (p - m * cw) + s; a1 = 2.0 * (m - p * cw); a2 = (p - m * cw) - s;
            break;
        }
    }
    out[0] = b0 / a0; out[1] = b1 / a0; out[2] = b2 / a0; out[3] = a1 / a0; out[4] = a2 / a0;
}
inline void coefficients(int kind, size_t sr, float freq_hz, float q, float gain_db, double out[5]) {
    coefficients_f64(kind, sr, (double)freq_hz, (double)q, (double)gain_db, out);
}

// |H(e^jw)| of the normalised coefficients at s = sin^2(w / 2), in long double, from the complex form (the squared-magnitude
// polynomial cancels near z = 1)
inline long double gain_at(const double c[5], long double s) {
    if (s < 0.0L) s = 0.0L;
    if (s > 1.0L) s = 1.0L;
    const long double cw = 1.0L - 2.0L * s, sw = 2.0L * sqrtl(s * (1.0L - s));   // cos w, sin w
    const long double c2 = cw * cw - sw * sw, s2 = 2.0L * sw * cw;               // cos 2w, sin 2w
    const long double nr = c[0] + c[1] * cw + c[2] * c2, ni = -(c[1] * sw + c[2] * s2);
    const long double dr = 1.0L + c[3] * cw + c[4] * c2, di = -(c[3] * sw + c[4] * s2);
    return sqrtl((nr * nr + ni * ni) / (dr * dr + di * di));
}
// Hmax = max over w of |H(e^jw)|, closed form: with s = sin^2(w / 2), |H|^2 = N(s) / D(s), two quadratics; the maximum over
// s in [0, 1] lies at an end or at a root of N' D - N D', itself a quadratic.
inline double hmax(const double c[5]) {
    const long double b0 = c[0], b1 = c[1], b2 = c[2], a1 = c[3], a2 = c[4];
    // N(s) = (b0 + b1 + b2)^2 - 4 (b1 (b0 + b2) + 4 b0 b2) s + 16 b0 b2 s^2
    const long double n0 = (b0 + b1 + b2) * (b0 + b1 + b2), n1 = -4.0L * (b1 * (b0 + b2) + 4.0L * b0 * b2), n2 = 16.0L * b0 * b2;
    const long double d0 = (1.0L + a1 + a2) * (1.0L + a1 + a2), d1 = -4.0L * (a1 * (1.0L + a2) + 4.0L * a2), d2 = 16.0L * a2;
    const long double qa = n2 * d1 - n1 * d2, qb = 2.0L * (n2 * d0 - n0 * d2), qc = n1 * d0 - n0 * d1;
    long double best = gain_at(c, 0.0L);
    const long double at1 = gain_at(c, 1.0L);
    if (at1 > best) best = at1;
    long double roots[2];
    int nr = 0;
    if (qa == 0.0L) {
        if (qb != 0.0L) roots[nr++] = -qc / qb;
    } else {
        const long double disc = qb * qb - 4.0L * qa * qc;
        if (disc >= 0.0L) {
            const long double sq = sqrtl(disc), t = -0.5L * (qb + (qb >= 0.0L ? sq : -sq));   // the stable pair of roots
            roots[nr++] = t / qa;
            if (t != 0.0L) roots[nr++] = qc / t;
        }
    }
    for (int i = 0; i < nr; ++i)
        if (roots[i] > 0.0L && roots[i] < 1.0L) {
            const long double h = gain_at(c, roots[i]);
            if (h > best) best = h;
        }
    return (double)best;
}

// 2x2 matrices in long double, row-major
struct M2 { long double m[4]; };
inline M2 mul(const M2& x, const M2& y) {
    return M2{{x.m[0] * y.m[0] + x.m[1] * y.m[2], x.m[0] * y.m[1] + x.m[1] * y.m[3],
               x.m[2] * y.m[0] + x.m[3] * y.m[2], x.m[2] * y.m[1] + x.m[3] * y.m[3]}};
}
inline M2 power(M2 x, uint64_t e) {
    M2 r{{1.0L, 0.0L, 0.0L, 1.0L}};
    for (; e; e >>= 1) {
        if (e & 1u) r = mul(r, x);
        if (e > 1u) x = mul(x, x);
    }
    return r;
}
inline void store(const M2& x, double out[4]) {
    for (int i = 0; i < 4; ++i) out[i] = (double)x.m[i];
}
// The powers of A = [[-a1, 1], [-a2, 0]] a descriptor carries: pw[k] = A^(run 2^k), a_tile = A^(run 256),
// pwc[k] = A^(run 256 chunk 2^k).  Squared in long double, each rounded once to f64 (f64 squaring loses the cancelling
// entries of A^2048 near z = 1: DESIGN.md §3n).
inline void powers(double a1, double a2, uint32_t run, uint32_t chunk, double pw[8][4], double a_tile[4], double pwc[8][4]) {
    M2 p = power(M2{{-(long double)a1, 1.0L, -(long double)a2, 0.0L}}, run);
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

}  // namespace eq
}  // namespace tde
