// reverb_math.h -- host arithmetic of the reverb vertex (include/termdaw_amd.h td_graph_add_reverb): the constants
// the kernel takes (g, d1, d2, w1, w2, the 24 line lengths), the window length B, the powers of d1 the wave scan joins lanes with
// (squared in long double, rounded once to f64), the range checks (shared by the C ABI and the Lua front-end) and the guard's gain
// bound Hrev.  No HIP call.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

namespace tde {
namespace reverb {

constexpr int kCombs = 8, kAllpass = 4;
constexpr int kLines = 2 * (kCombs + kAllpass);   // 24: left combs, right combs, left all-passes, right all-passes
constexpr int kParams = 7 + kLines;               // td_reverb_params' out[]
constexpr int kCombTuning[kCombs] = {1116, 1188, 1277, 1356, 1422, 1491, 1557, 1617};   // frames at 44.1 kHz (Freeverb, public domain)
constexpr int kAllpassTuning[kAllpass] = {556, 441, 341, 225};
constexpr int kSpread = 23;                       // the right channel's lines are this much longer (at 44.1 kHz)
constexpr uint32_t kMinLine = 64;                 // the shortest line the window scheme takes
constexpr uint32_t kFormDefault = 1;              // "debug.reverb_form": 0 serial, 1 scan (DESIGN.md §3r has the table the defaults come from)
constexpr uint32_t kBlockDefault = 256;           // "debug.reverb_block": the cap of the window length B (64 | 128 | 256)

// line i of kLines: 0 .. 7 left combs, 8 .. 15 right combs, 16 .. 19 left all-passes, 20 .. 23 right all-passes
inline uint32_t line_frames(size_t sr, float size, int i) {
    const bool right = i >= 20 || (i >= 8 && i < 16);
    const int tuning = i < 16 ? kCombTuning[i & 7] : kAllpassTuning[(i - 16) & 3];
    const double d = (double)(tuning + (right ? kSpread : 0)) * (double)size * (double)sr / 44100.0;
    const long long n = llround(d);
    return n < 0 ? 0u : (uint32_t)n;
}

// out[0 .. 4] = g, d1, d2, w1, w2;  out[5] = Hrev;  out[6] = B, the window length at the default cap;  out[7 ..] = the 24 line lengths
// (left combs, right combs, left all-passes, right all-passes) -- from the f32 parameters, widened
inline void params(size_t sr, float room, float damp, float width, float size, double out[kParams]) {
    const double g = 0.7 + 0.28 * (double)room;
    const double d1 = 0.4 * (double)damp;
    out[0] = g;
    out[1] = d1;
    out[2] = 1.0 - d1;
    out[3] = (1.0 + (double)width) / 2.0;
    out[4] = (1.0 - (double)width) / 2.0;
    // Hrev (DESIGN.md §3r has the proof): input mix 0.015 x 2, comb bank 8 / (1 - g), all-pass chain (5/3)^4, output mix 1
    const double ap = 5.0 / 3.0;
    out[5] = (0.015 * 2.0) * (8.0 / (1.0 - g)) * ((ap * ap) * (ap * ap));
    uint32_t shortest = 0xFFFFFFFFu;
    for (int i = 0; i < kLines; ++i) {
        const uint32_t d = line_frames(sr, size, i);
        out[7 + i] = (double)d;
        if (d < shortest) shortest = d;
    }
    out[6] = shortest >= 256u ? 256.0 : shortest >= 128u ? 128.0 : 64.0;
}

// the window length: the largest of 64, 128 and 256 that exceeds neither the vertex' shortest line nor `cap`
inline uint32_t window(uint32_t shortest, uint32_t cap) {
    uint32_t b = shortest >= 256u ? 256u : shortest >= 128u ? 128u : 64u;
    return b < cap ? b : cap;
}

// pw[k] = d1^(q 2^k), k = 0 .. 5: what a lane's carry is scaled by across 2^k lanes of q frames each
inline void powers(double d1, uint32_t q, double pw[6]) {
    long double p = 1.0L;
    for (uint32_t i = 0; i < q; ++i) p *= (long double)d1;
    for (int k = 0; k < 6; ++k) {
        pw[k] = (double)p;
        p = p * p;
    }
}

// nullptr, or what is wrong: the message names the parameter (a NaN fails every comparison)
inline const char* check(size_t sr, float room, float damp, float width, float size) {
    if (!(room >= 0.0f && room <= 1.0f)) return "room must lie in [0, 1]";
    if (!(damp >= 0.0f && damp <= 1.0f)) return "damp must lie in [0, 1]";
    if (!(width >= 0.0f && width <= 1.0f)) return "width must lie in [0, 1]";
    if (!(size >= 0.5f && size <= 2.0f)) return "size must lie in [0.5, 2]";
    if (sr == 0) return "the sample rate is 0";
    if (!((double)(kCombTuning[7] + kSpread) * (double)size * (double)sr / 44100.0 < 1e9)) return "size: the lines are too long at this sample rate";
    for (int i = 0; i < kLines; ++i)
        if (line_frames(sr, size, i) < kMinLine) return "size: the shortest line must be at least 64 frames at this sample rate";
    return nullptr;
}

}  // namespace reverb
}  // namespace tde
