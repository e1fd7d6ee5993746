// delay_math.h -- host arithmetic of the feedback delay vertex (include/termdaw_amd.h td_graph_add_delay): the
// delay in frames, the feedback matrix G = [[gs, gc], [gc, gs]], the L2 gain of the echo path, the tiling of a chunk and the
// powers of G the carry kernel joins tiles with (eq_math.h's long-double squaring, rounded once to f64).  No HIP call.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "eq_math.h"

namespace tde {
namespace delay {

constexpr uint32_t kTileDefault = 16;   // steps per tile ("debug.delay_tile" 8 | 16 | 32 | 64)
constexpr uint32_t kCarryFold = 16;     // k_delay_carry: tiles a thread folds serially before lanes get more threads

// nullptr: fine, otherwise the reason.  rate_free: only the ranges that do not depend on the rate (a script line's: eq_math.h)
inline const char* check(size_t sr, float time_ms, float feedback, float cross, bool rate_free = false) {
    if (!rate_free && !sr) return "the sample rate must be positive";
    if (!(time_ms >= 1.0f && time_ms <= 2000.0f)) return "time_ms must lie in [1, 2000] ms";
    if (!(feedback >= 0.0f && feedback <= 0.98f)) return "feedback must lie in [0, 0.98]";
    if (!(cross >= 0.0f && cross <= 1.0f)) return "cross must lie in [0, 1]";
    if (!rate_free && (double)time_ms * (double)sr / 1000.0 > 268435456.0) return "time_ms is more than 2^28 frames at this sample rate";
    return nullptr;
}

// (D, gs, gc, Hecho) in f64 from the f32 parameters, widened
inline void params(size_t sr, float time_ms, float feedback, float cross, double out[4]) {
    const long long d = llround((double)time_ms * (double)sr / 1000.0);
    out[0] = (double)(d < 1 ? 1 : d);
    out[1] = (double)feedback * (1.0 - (double)cross);
    out[2] = (double)feedback * (double)cross;
    out[3] = 1.0 / (1.0 - (double)feedback);
}

// How a chunk of `frames` frames is tiled: lanes = min(D, frames), n_tiles = ceil(ceil(frames / D) / T); the carry gives a lane
// `seg` threads (a power of two <= 256) of `chunk` tiles each, seg the smallest that keeps chunk <= kCarryFold.
struct Tiling { uint32_t lanes, n_tiles, seg, chunk; };
inline Tiling tiling(uint64_t frames, uint64_t D, uint32_t T) {
    Tiling t;
    t.lanes = (uint32_t)(D < frames ? D : frames);
    const uint64_t steps = (frames + D - 1) / D;
    t.n_tiles = (uint32_t)((steps + T - 1) / T);
    t.seg = 1;
    while (t.seg < 256u && (uint64_t)t.seg * kCarryFold < t.n_tiles) t.seg *= 2u;
    t.chunk = (t.n_tiles + t.seg - 1) / t.seg;
    return t;
}

// g_tile = G^T, pwc[k] = G^(T chunk 2^k)
inline void powers(double gs, double gc, uint32_t T, uint32_t chunk, double g_tile[4], double pwc[8][4]) {
    eq::M2 p = eq::power(eq::M2{{(long double)gs, (long double)gc, (long double)gc, (long double)gs}}, T);
    eq::store(p, g_tile);
    p = eq::power(p, chunk);
    for (int k = 0; k < 8; ++k) {
        eq::store(p, pwc[k]);
        p = eq::mul(p, p);
    }
}

}  // namespace delay
}  // namespace tde
