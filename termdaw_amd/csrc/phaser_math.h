// phaser_math.h -- host arithmetic of the phaser vertex (include/termdaw_amd.h td_graph_add_phaser): the
// constants the kernels take (N, a_lo, a_hi, am, ad, f, fb) and the range checks (shared by the C ABI and the Lua front-end).
// No HIP call.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

namespace tde {
namespace phaser {

constexpr int kMaxStages = 8;
constexpr int kParams = 7;

// the all-pass coefficient whose section turns the phase by 90 degrees at fc
inline double g(double fc, double sr) {
    const double pi = 3.14159265358979323846;
    const double t = tan(pi * fc / sr);
    return (t - 1.0) / (t + 1.0);
}

// out[0 .. 6] = N, a_lo, a_hi, am, ad, f, fb -- from the f32 parameters, widened
inline void params(size_t sr, int stages, float lo_hz, float hi_hz, float rate_hz, float feedback, float /*stereo*/, int /*shape*/, double out[kParams]) {
    const double a_lo = g((double)lo_hz, (double)sr), a_hi = g((double)hi_hz, (double)sr);
    out[0] = (double)stages;
    out[1] = a_lo;
    out[2] = a_hi;
    out[3] = 0.5 * (a_lo + a_hi);
    out[4] = 0.5 * (a_hi - a_lo);
    out[5] = (double)rate_hz / (double)sr;
    out[6] = (double)feedback;
}

// nullptr, or what is wrong: the message names the parameter (a NaN fails every comparison)
inline const char* check(size_t sr, int stages, float lo_hz, float hi_hz, float rate_hz, float feedback, float stereo, int shape) {
    if (!(stages == 2 || stages == 4 || stages == 6 || stages == 8)) return "stages must be 2, 4, 6 or 8";
    if (!(shape >= 0 && shape <= 1)) return "shape must be 0 (sine) or 1 (triangle)";
    if (sr == 0) return "the sample rate is 0";
    if (!(lo_hz >= 20.0f && lo_hz <= 3.0e38f)) return "lo_hz must be at least 20 Hz";
    if (!((double)hi_hz <= 0.45 * (double)sr && hi_hz >= -3.0e38f)) return "hi_hz must not exceed 0.45 of the sample rate";
    if (!(lo_hz <= hi_hz)) return "lo_hz must not exceed hi_hz";
    if (!(rate_hz >= 0.01f && rate_hz <= 20.0f)) return "rate_hz must lie in [0.01, 20] Hz";
    if (!(feedback >= -0.95f && feedback <= 0.95f)) return "feedback must lie in [-0.95, 0.95]";
    if (!(stereo >= 0.0f && stereo <= 0.5f)) return "stereo must lie in [0, 0.5]";
    return nullptr;
}

}  // namespace phaser
}  // namespace tde
