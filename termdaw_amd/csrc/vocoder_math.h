// vocoder_math.h -- host arithmetic of the vocoder vertex (include/termdaw_amd.h td_graph_add_vocoder): the
// constants the kernels take (per band f_b and the RBJ band-pass coefficients of eq_math.h at (f_b, q); the follower's a; the
// output gain g) and the range checks (shared by the C ABI and the Lua front-end).  No HIP call.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "eq_math.h"

namespace tde {
namespace vocoder {

constexpr int kMaxBands = 16;
constexpr int kBandParams = 6;                                  // f_b, b0, b1, b2, a1, a2
constexpr int kMaxParams = kMaxBands * kBandParams + 2;         // ... per band, then a, then g
inline size_t n_params(int bands) { return (size_t)bands * kBandParams + 2; }

// f_b = lo (hi / lo)^(b / (B - 1)), in f64 from the widened f32 parameters
inline double centre(int b, int bands, float lo_hz, float hi_hz) {
    return (double)lo_hz * pow((double)hi_hz / (double)lo_hz, (double)b / (double)(bands - 1));
}

// out[6 b .. 6 b + 5] = f_b, b0, b1, b2, a1, a2;  out[6 B] = a;  out[6 B + 1] = g.  The band-pass is eq::coefficients' kind 2
// (constant 0 dB peak gain), in its f64 form at (f_b, q).
inline void params(size_t sr, int bands, float lo_hz, float hi_hz, float q, float response_ms, float out_db, double* out) {
    for (int b = 0; b < bands; ++b) {
        const double f = centre(b, bands, lo_hz, hi_hz);
        out[kBandParams * b] = f;
        eq::coefficients_f64(2, sr, f, (double)q, 0.0, out + kBandParams * b + 1);
    }
    out[kBandParams * bands] = exp(-1.0 / ((double)response_ms * (double)sr / 1000.0));
    out[kBandParams * bands + 1] = pow(10.0, (double)out_db / 20.0);
}

// nullptr, or what is wrong: the message names the parameter (a NaN fails every comparison)
inline const char* check(size_t sr, int bands, float lo_hz, float hi_hz, float q, float response_ms, float out_db) {
    if (!(bands == 4 || bands == 8 || bands == 16)) return "bands must be 4, 8 or 16";
    if (sr == 0) return "the sample rate is 0";
    if (!(lo_hz >= 40.0f && lo_hz <= 3.0e38f)) return "lo_hz must be at least 40 Hz";
    if (!((double)hi_hz <= 0.45 * (double)sr && hi_hz >= -3.0e38f)) return "hi_hz must not exceed 0.45 of the sample rate";
    if (!(lo_hz < hi_hz)) return "lo_hz must lie below hi_hz";
    if (!(q >= 0.5f && q <= 20.0f)) return "q must lie in [0.5, 20]";
    if (!(response_ms >= 0.1f && response_ms <= 1000.0f)) return "response_ms must lie in [0.1, 1000] ms";
    if (!(out_db >= -24.0f && out_db <= 48.0f)) return "out_db must lie in [-24, 48] dB";
    return nullptr;
}

}  // namespace vocoder
}  // namespace tde
