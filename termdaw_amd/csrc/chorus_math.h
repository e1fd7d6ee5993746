// chorus_math.h -- host arithmetic of the chorus vertex (include/termdaw_amd.h td_graph_add_chorus): the
// constants the kernels take (D0, A, f, H), the largest delay slope s the range check bounds, the range checks themselves (shared
// by the C ABI and the Lua front-end) and the guard's gain bound Hch.  No HIP call.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

namespace tde {
namespace chorus {

constexpr uint32_t kTileDefault = 256;   // output frames per workgroup (provisional; "debug.chorus_tile" 256 | 512 | 1024)
constexpr int kMaxVoices = 4;
// Hch: an L2 bound of the wet path (DESIGN.md §3q has the proof): sqrt(1.25 x 2.1283001 x 2) = 2.30668, rounded up
constexpr double kHch = 2.307;

// out[0 .. 5] = D0, A, f, H, s, Hch -- from the f32 parameters, widened
inline void params(size_t sr, int /*voices*/, float delay_ms, float depth_ms, float rate_hz, float /*stereo*/, int shape, double out[6]) {
    const double pi = 3.14159265358979323846;
    const double D0 = (double)delay_ms * (double)sr / 1000.0;
    const double A = (double)depth_ms * (double)sr / 1000.0;
    const double f = (double)rate_hz / (double)sr;
    const double reach = floor(D0 + A) + 3.0;
    out[0] = D0;
    out[1] = A;
    out[2] = f;
    out[3] = ceil(reach / 64.0) * 64.0;
    out[4] = shape == 0 ? 2.0 * pi * A * f : 4.0 * A * f;
    out[5] = kHch;
}

inline const char* const* shape_names() {   // (the script line's names of an LFO's shape, TD_CHORUS_* in order: the phaser's and the filter's too)
    static const char* const n[2] = {"sine", "triangle"};
    return n;
}
// nullptr, or what is wrong: the message names the parameter (a NaN fails every comparison)
inline const char* check(size_t sr, int voices, float delay_ms, float depth_ms, float rate_hz, float stereo, int shape) {
    if (!(voices >= 1 && voices <= kMaxVoices)) return "voices must be 1 .. 4";
    if (!(shape >= 0 && shape <= 1)) return "shape must be 0 (sine) or 1 (triangle)";
    if (!(delay_ms >= 0.5f && delay_ms <= 50.0f)) return "delay_ms must lie in [0.5, 50] ms";
    if (!(depth_ms >= 0.0f)) return "depth_ms must be at least 0";
    if (!((double)delay_ms + (double)depth_ms <= 50.0)) return "depth_ms: delay_ms + depth_ms must not exceed 50 ms";
    if (!(rate_hz >= 0.01f && rate_hz <= 20.0f)) return "rate_hz must lie in [0.01, 20] Hz";
    if (!(stereo >= 0.0f && stereo <= 0.5f)) return "stereo must lie in [0, 0.5]";
    if (sr == 0) return "the sample rate is 0";
    double c[6];
    params(sr, voices, delay_ms, depth_ms, rate_hz, stereo, shape, c);
    if (!(c[0] - c[1] >= 2.0)) return "depth_ms: the shortest delay, delay_ms - depth_ms, must be at least 2 frames";
    if (!(c[4] <= 0.5)) return "rate_hz: the delay may change by at most half a frame per frame (2 pi depth rate for a sine, 4 depth rate for a triangle)";
    return nullptr;
}

}  // namespace chorus
}  // namespace tde
