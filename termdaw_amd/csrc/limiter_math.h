// limiter_math.h -- host arithmetic of the limiter vertex (include/termdaw_amd.h td_graph_add_limiter): the
// constants the kernels take (c, gin, L, a) with the latency they imply, and the range checks (shared by the C ABI and the Lua
// front-end).  No HIP call.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

namespace tde {
namespace limiter {

constexpr int kParams = 5;
constexpr double kMaxL = 2048.0;   // the lookahead's halo lies within one tile of the kernels (kernels.h kLimTile)

// L: the lookahead window in frames, from the f32 parameter widened
inline double frames(size_t sr, float lookahead_ms) {
    const long long l = llround((double)lookahead_ms * (double)sr / 1000.0);
    return l < 1 ? 1.0 : (double)l;
}

// out[0 .. 4] = c, gin, L, a, latency (= L - 1 frames) -- from the f32 parameters, widened
inline void params(size_t sr, float ceiling_db, float lookahead_ms, float release_ms, float drive_db, double out[kParams]) {
    out[0] = pow(10.0, (double)ceiling_db / 20.0);
    out[1] = pow(10.0, (double)drive_db / 20.0);
    out[2] = frames(sr, lookahead_ms);
    out[3] = exp(-1.0 / ((double)release_ms * (double)sr / 1000.0));
    out[4] = out[2] - 1.0;
}

// nullptr, or what is wrong: the message names the parameter (a NaN fails every comparison, an infinity the far end)
inline const char* check(size_t sr, float ceiling_db, float lookahead_ms, float release_ms, float drive_db) {
    if (sr == 0) return "the sample rate is 0";
    if (!(ceiling_db >= -24.0f && ceiling_db <= 0.0f)) return "ceiling_db must lie in [-24, 0] dB";
    if (!(lookahead_ms >= 0.0f && lookahead_ms <= 50.0f)) return "lookahead_ms must lie in [0, 50] ms";
    if (!(frames(sr, lookahead_ms) <= kMaxL)) return "lookahead_ms is more than 2048 frames at this sample rate";
    if (!(release_ms >= 1.0f && release_ms <= 10000.0f)) return "release_ms must lie in [1, 10000] ms";
    if (!(drive_db >= -24.0f && drive_db <= 24.0f)) return "drive_db must lie in [-24, 24] dB";
    return nullptr;
}

}  // namespace limiter
}  // namespace tde
