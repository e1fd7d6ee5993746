// The quad-granular partition of the ragged wide packed sum (k_sum16r, kernels.hip), shared by the device code, the host
// (launch_sum, compile.cpp) and a stand-alone CPU test (tests/asan_sum_partition.cpp).  A quad is 256 frames: what one
// load instruction of a wave reads in one piece.  A timeline of M frames has Q = ceil(M / 256) quads; a grid of G workgroups
// deals them out evenly, and a workgroup deals its share out evenly to its four waves.  Nothing is tabulated: every range
// derives from (g, G, Q).
#pragma once
#include <stdint.h>
#if defined(__HIPCC__) || defined(__CUDACC__)
#include <hip/hip_runtime.h>
#define TD_SP_HD __host__ __device__ __forceinline__
#else
#define TD_SP_HD inline
#endif

namespace tdsp {

constexpr uint32_t kQuadFrames = 256;     // frames per quad
constexpr uint32_t kQuadsPerBlock = 4;    // quads per 1 024-frame reference block
constexpr uint32_t kWaves = 4;            // waves per workgroup
constexpr uint32_t kMinQuads = 4;         // per workgroup: every wave owns at least one quad, a block straddles at most two workgroups
constexpr uint32_t kMaxQuads = 16;        // per workgroup: a wave owns at most four quads

struct QuadRange { uint32_t q0, n; };     // quads [q0, q0 + n)

TD_SP_HD uint32_t quads_of(uint32_t frames) { return (frames + kQuadFrames - 1u) / kQuadFrames; }

// G workgroups can carry Q quads: every workgroup gets between kMinQuads and kMaxQuads of them
TD_SP_HD bool groups_ok(uint32_t Q, uint32_t G) {
    return G != 0u && (uint64_t)G * kMinQuads <= Q && Q <= (uint64_t)G * kMaxQuads;
}

// workgroup g of G owns quads [floor(g Q / G), floor((g + 1) Q / G))
TD_SP_HD QuadRange group_quads(uint32_t g, uint32_t G, uint32_t Q) {
    const uint32_t a = (uint32_t)((uint64_t)g * Q / G), b = (uint32_t)(((uint64_t)g + 1u) * Q / G);
    QuadRange r; r.q0 = a; r.n = b - a;
    return r;
}

// wave w of a workgroup owning n quads owns [floor(w n / 4), floor((w + 1) n / 4)) of them
TD_SP_HD QuadRange wave_quads(QuadRange wg, uint32_t w) {
    const uint32_t a = w * wg.n / kWaves, b = (w + 1u) * wg.n / kWaves;
    QuadRange r; r.q0 = wg.q0 + a; r.n = b - a;
    return r;
}

// the workgroup's last reference block continues in workgroup g + 1
TD_SP_HD bool tail_straddles(QuadRange wg, uint32_t Q) {
    const uint32_t end = wg.q0 + wg.n;
    return end % kQuadsPerBlock != 0u && end < Q;
}

// The grid the host picks for a timeline of `frames` (0: the form does not apply).  forced != 0 (engine option debug.sum_groups):
// that many workgroups, or 0 if they cannot carry the timeline's quads.  Automatic: wpc workgroups per CU on `cus` CUs, from
// `min_frames` on (where 16 frames per lane pay at all), if every workgroup then gets 4 .. 16 quads.  need_resident (a mode-5
// Normalize): only a grid of at most `capacity` workgroups, what the device holds at once.  (The grid index travels in 16 bits.)
TD_SP_HD uint32_t pick_groups(uint32_t frames, uint32_t forced, bool need_resident, uint32_t capacity, uint32_t cus, uint32_t wpc, uint32_t min_frames) {
    const uint32_t Q = quads_of(frames);
    const uint32_t G = forced ? forced : ((wpc == 0u || frames < min_frames) ? 0u : wpc * cus);
    return (groups_ok(Q, G) && G <= 65535u && (!need_resident || G <= capacity)) ? G : 0u;
}

}  // namespace tdsp
