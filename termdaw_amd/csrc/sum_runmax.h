// The running peak of a single-pass Normalize tile (k_sum16w, SumDesc modes 4 / 5; kernels.hip), shared by the device code and a
// stand-alone CPU test (tests/asan_sum_runmax.cpp).  Block b of a render is scaled by 1 / max_b, max_b = peak_b.max(max_{b-1})
// (`*max = buf_max.max(*max)`, extensions.rs:323): for the NB blocks of one tile that is a fold over the tile's own block peaks,
// started from the running peak ENTERING the tile -- the carried max and every lower tile's peak.  A tile folds twice: once from
// the lower tiles' peaks it can see at one look (it scales and stores with that), once from all of them; a block whose two
// running peaks are the same float has the reference's bytes in memory already, every other block is scaled and stored again.
#pragma once
#include <stdint.h>
#include <math.h>
#if defined(__HIPCC__) || defined(__CUDACC__)
#include <hip/hip_runtime.h>
#define TD_RM_HD __host__ __device__ __forceinline__
#else
#define TD_RM_HD inline
#endif

namespace tdrm {

// absmaxlen's fold (sample.rs:12-14): `if a > max {a} else {max}`; peaks are >= 0 and never NaN (kernels.hip absmax4), fmaxf agrees
TD_RM_HD float fmax2(float a, float b) { return fmaxf(a, b); }

// the running peak entering a tile: the carried max and the maximum over the lower tiles' peaks (0 where there is none)
TD_RM_HD float entering(float carried, float lower) { return fmax2(lower, carried); }

// run[b] = the running peak of the tile's block b; returns the one leaving the tile.  (NB = 1, 2 or 4, written out: with constant
// indices from the start the arrays are registers on the device, not memory)
template <int NB>
TD_RM_HD float fold(float enter, const float (&pb)[NB], float (&run)[NB]) {
    static_assert(NB == 1 || NB == 2 || NB == 4, "a tile is 1, 2 or 4 reference blocks");
    float r = fmax2(pb[0], enter);   // *max = buf_max.max(*max)
    run[0] = r;
    if constexpr (NB > 1) {
        r = fmax2(pb[1], r);
        run[1] = r;
    }
    if constexpr (NB > 2) {
        r = fmax2(pb[2], r);
        run[2] = r;
        r = fmax2(pb[3], r);
        run[3] = r;
    }
    return r;
}

TD_RM_HD uint32_t bits(float v) { return __builtin_bit_cast(uint32_t, v); }

// Was block b stored with another scale than it must have?  The PEAKS are compared, as words: equal words give the same
// reciprocal and so the same bytes; anything else is stored again.
TD_RM_HD bool differs(float spec, float fin) { return bits(spec) != bits(fin); }

// bit b: block b of the tile has to be scaled and stored again
template <int NB>
TD_RM_HD uint32_t redo_mask(const float (&spec)[NB], const float (&fin)[NB]) {
    static_assert(NB == 1 || NB == 2 || NB == 4, "a tile is 1, 2 or 4 reference blocks");
    uint32_t m = differs(spec[0], fin[0]) ? 1u : 0u;
    if constexpr (NB > 1) m |= differs(spec[1], fin[1]) ? 2u : 0u;
    if constexpr (NB > 2) m |= (differs(spec[2], fin[2]) ? 4u : 0u) | (differs(spec[3], fin[3]) ? 8u : 0u);
    return m;
}

// the running peak of block `mine` (a wave's quads are all one block's)
template <int NB>
TD_RM_HD float of_block(const float (&run)[NB], uint32_t mine) {
    static_assert(NB == 1 || NB == 2 || NB == 4, "a tile is 1, 2 or 4 reference blocks");
    if constexpr (NB == 1) return run[0];
    else if constexpr (NB == 2) return mine == 0u ? run[0] : run[1];
    else return mine == 0u ? run[0] : mine == 1u ? run[1] : mine == 2u ? run[2] : run[3];
}

}  // namespace tdrm
