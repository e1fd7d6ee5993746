// sat_math.h -- host arithmetic of the saturator vertex (include/termdaw_amd.h td_graph_add_saturator): the
// prototype low-pass both polyphase filters share (a 4-term Blackman-Harris windowed sinc, in f64), the shapers, the gains and
// the guard's gain bound Hsat.  No HIP call.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace tde {
namespace sat {

constexpr uint32_t kZ = 32;             // zero crossings of the prototype per side, in frames
constexpr uint32_t kLatency = 2 * kZ;   // both linear-phase filters together: 64 frames
constexpr uint32_t kLine = 4 * kZ;      // raw input frames an output frame can reach back to: 128
constexpr uint32_t kTileDefault = 256;  // output frames per workgroup (provisional; "debug.sat_tile" 128 | 256 | 384)

inline bool oversample_ok(int R) { return R == 1 || R == 2 || R == 4 || R == 8; }
inline const char* const* kind_names() {   // (the script line's names, TD_SAT_* in order)
    static const char* const n[3] = {"hard", "cubic", "soft"};
    return n;
}
// nullptr: fine, otherwise the reason
inline const char* check(int kind, int oversample, float drive_db, float bias, float out_db) {
    if (!(kind >= 0 && kind <= 2)) return "kind must be 0 (hard), 1 (cubic) or 2 (soft)";
    if (!oversample_ok(oversample)) return "oversample must be 1, 2, 4 or 8";
    if (!(drive_db >= -24.0f && drive_db <= 48.0f)) return "drive_db must lie in [-24, 48] dB";
    if (!(bias >= -1.0f && bias <= 1.0f)) return "bias must lie in [-1, 1]";
    if (!(out_db >= -48.0f && out_db <= 24.0f)) return "out_db must lie in [-48, 24] dB";
    return nullptr;
}
inline uint32_t n_taps(int R) { return 2u * kZ * (uint32_t)R + 1u; }

// h[0 .. 2ZR]: s w / sum(s w), every sum from 0.0 in ascending index
inline std::vector<double> make_taps(int R) {
    const uint32_t L = n_taps(R);
    const double pi = 3.14159265358979323846;
    const double fc = (0.5 - 2.0 / (double)kZ) / (double)R;
    std::vector<double> h(L);
    double sum = 0.0;
    for (uint32_t k = 0; k < L; ++k) {
        const double t = (double)k - (double)(kZ * (uint32_t)R);
        const double s = t == 0.0 ? 2.0 * fc : sin(2.0 * pi * fc * t) / (pi * t);
        const double a = 2.0 * pi * (double)k / (double)(L - 1u);
        const double w = 0.35875 - 0.48829 * cos(a) + 0.14128 * cos(2.0 * a) - 0.01168 * cos(3.0 * a);
        h[k] = s * w;
        sum += h[k];
    }
    for (uint32_t k = 0; k < L; ++k) h[k] /= sum;
    return h;
}
inline int log2r(int R) { return R == 1 ? 0 : R == 2 ? 1 : R == 4 ? 2 : 3; }
inline const std::vector<double>& taps(int R) {
    static const std::vector<double> t[4] = {make_taps(1), make_taps(2), make_taps(4), make_taps(8)};
    return t[log2r(R)];
}

// the shapers (IEEE operations only, in this order: the kernels' sat_shape is the same text)
inline double shape(int kind, double u) {
    switch (kind) {
        case 0: return fmin(fmax(u, -1.0), 1.0);
        case 1: return fabs(u) < 1.0 ? 1.5 * u - ((0.5 * u) * u) * u : copysign(1.0, u);
        default: return u / (1.0 + fabs(u));
    }
}
inline double lipschitz(int kind) { return kind == 1 ? 1.5 : 1.0; }

// Hup = sqrt(sum_r max_w |U_r|^2) over the branches U_r = R h[r::R], on a dense grid in long double.  The decimator's branches
// are G_r = U_r / R, so Hdown = Hup / R exactly.
inline double make_hup(int R) {
    if (R == 1) return 1.0;
    const std::vector<double>& h = taps(R);
    const int N = 2048;
    const long double pi = 3.14159265358979323846264338327950288L;
    long double total = 0.0L;
    for (int r = 0; r < R; ++r) {
        long double best = 0.0L;
        for (int i = 0; i <= N; ++i) {
            const long double w = pi * (long double)i / (long double)N;
            // (the rotation e^{-jw} applied tap by tap: one sincos per grid point)
            const long double cw = cosl(w), sw = sinl(w);
            long double re = 0.0L, im = 0.0L, c = 1.0L, s = 0.0L;
            for (size_t k = (size_t)r; k < h.size(); k += (size_t)R) {
                const long double u = (long double)R * (long double)h[k];
                re += u * c;
                im -= u * s;
                const long double c2 = c * cw - s * sw;
                s = s * cw + c * sw;
                c = c2;
            }
            const long double p = re * re + im * im;
            if (p > best) best = p;
        }
        total += best;
    }
    return (double)sqrtl(total);
}
inline double hup(int R) {
    static const double v[4] = {make_hup(1), make_hup(2), make_hup(4), make_hup(8)};
    return v[log2r(R)];
}

// out[0 .. 5] = g_in, g_out, f(bias), latency in frames, Lf, Hsat -- from the f32 parameters, widened
inline void params(int kind, int R, float drive_db, float bias, float out_db, double out[6]) {
    out[0] = pow(10.0, (double)drive_db / 20.0);
    out[1] = pow(10.0, (double)out_db / 20.0);
    out[2] = shape(kind, (double)bias);
    out[3] = R == 1 ? 0.0 : (double)kLatency;
    out[4] = lipschitz(kind);
    const double hu = hup(R), hd = hu / (double)R;
    out[5] = R == 1 ? out[1] * out[4] * out[0] : out[1] * hd * out[4] * out[0] * hu;
}

}  // namespace sat
}  // namespace tde
