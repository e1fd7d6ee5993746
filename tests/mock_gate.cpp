// The gate launches for the host-only sanitizer build of the engine (TEST INFRASTRUCTURE: linked only by tests/test_gate_host.py
// beside tests/mock_hip.cpp, never by the product).  Nothing is computed: every launch walks its descriptor table and both ends of
// every array a descriptor points to, so that a descriptor that points past an allocation is an AddressSanitizer report, and
// checks what the kernels rely on -- the tiling, the carry's lane chunks, the packed words' room for H + 1, that every launch of a
// vertex reads the very descriptor words the first one saw, and that the five launches of a vertex come in order (detect, carry
// (h, c), env, carry env, apply).
// The driver is tests/asan_comp.cpp as it is: its counters keep the names it declares (g_comp_*), counting gate launches here.
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <cmath>
#include <map>

#define MOCK_NAME "mock_gate"
#include "mock_util.h"

size_t g_comp_launches[5] = {0, 0, 0, 0, 0}, g_comp_vertices = 0, g_comp_fresh = 0, g_comp_carried = 0;

namespace {
struct Track { int phase; tdk::GateDesc first; };
std::map<const uint32_t*, Track> g_by_map;   // a vertex of the submission under way, by its tile-map words
}  // namespace

namespace tdk {
static void check(const GateDesc* d, int n, uint32_t max_tiles, int which) {
    touch(d, (size_t)std::max(n, 0) * sizeof(GateDesc));
    g_comp_launches[which] += 1;
    const bool carry = which == 1 || which == 3;
    for (int i = 0; i < n; ++i) {
        const GateDesc& s = d[i];
        if (!s.ins || !s.x || !s.out || !s.state || !s.map || !s.carry_hc || !s.tbits || !s.aggA || !s.aggB || !s.carry_env) die("null pointer in a GateDesc");
        if (s.init && s.init != s.state) die("entry state");
        if (!s.frames || s.n_tiles != (s.frames + kGateTile - 1) / kGateTile || (!carry && s.n_tiles > max_tiles)) die("tiling");
        if ((size_t)s.chunk * kThreads < s.n_tiles || (s.chunk > 1 && (size_t)(s.chunk - 1) * kThreads >= s.n_tiles)) die("carry lane chunks");
        if ((const void*)s.x == (const void*)s.out) die("buffers alias");
        if (!(s.wet >= 0.0001f && s.wet <= 1.0f)) die("wet");
        if (!(s.aR > 0.0 && s.aR < 1.0) || !(s.aA >= 0.0 && s.aA < 1.0) || s.oA != 1.0 - s.aA || s.oR != 1.0 - s.aR) die("coefficients");
        if (!(s.To > 0.0 && s.To <= 1.0) || !(s.Tc > 0.0 && s.Tc <= s.To) || !(s.F > 0.0 && s.F <= 1.0) || s.oF != 1.0 - s.F) die("parameters");
        if (!s.cap || s.cap > kGateK) die("hold counter's room");
        if ((((uintptr_t)s.x) | ((uintptr_t)s.out)) & 15u) die("alignment");
        if ((((uintptr_t)s.aggA) | ((uintptr_t)s.aggB) | ((uintptr_t)s.carry_env) | ((uintptr_t)s.map)) & 7u) die("tile words' alignment");
        touch_terms(s.ins, s.k, s.frames, "a gate vertex takes terms of kinds 0 .. 4 only");
        touch_w(s.x, (size_t)((s.frames + 1u) & ~1u) * sizeof(float2));   // (pairs: an odd chunk's last store covers one frame more)
        touch_w(s.out, (size_t)((s.frames + 1u) & ~1u) * sizeof(float2));
        touch_w(s.state, sizeof(GateState));
        touch_w(s.map, (size_t)s.n_tiles * 8);
        touch_w(s.carry_hc, (size_t)s.n_tiles * 4);
        touch_w(s.tbits, (size_t)s.n_tiles * kThreads);
        touch_w(s.aggA, (size_t)s.n_tiles * 8);
        touch_w(s.aggB, (size_t)s.n_tiles * 8);
        touch_w(s.carry_env, (size_t)s.n_tiles * 8);
        // the arrays of one vertex are apart
        const uintptr_t a[6] = {(uintptr_t)s.map, (uintptr_t)s.carry_hc, (uintptr_t)s.tbits, (uintptr_t)s.aggA, (uintptr_t)s.aggB, (uintptr_t)s.carry_env};
        const size_t b[6] = {(size_t)s.n_tiles * 8, (size_t)s.n_tiles * 4, (size_t)s.n_tiles * kThreads, (size_t)s.n_tiles * 8, (size_t)s.n_tiles * 8, (size_t)s.n_tiles * 8};
        for (int p = 0; p < 6; ++p)
            for (int q = p + 1; q < 6; ++q)
                if (a[p] < a[q] + b[q] && a[q] < a[p] + b[p]) die("tile words overlap");
        if (which == 0) {
            if (g_by_map.count(s.map) && g_by_map[s.map].phase != 0) die("a vertex' tile words reused before its launches finished");
            g_by_map[s.map] = Track{1, s};
            g_comp_vertices += 1;
            (s.init ? g_comp_carried : g_comp_fresh) += 1;
        } else {
            auto it = g_by_map.find(s.map);
            if (it == g_by_map.end() || it->second.phase != which) die("launch order");
            const GateDesc& f = it->second.first;
            if (f.carry_hc != s.carry_hc || f.tbits != s.tbits || f.aggA != s.aggA || f.aggB != s.aggB || f.carry_env != s.carry_env || f.x != s.x ||
                f.out != s.out || f.state != s.state || f.init != s.init || f.cap != s.cap || f.frames != s.frames)
                die("descriptor changed between launches");
            it->second.phase = which == 4 ? 0 : which + 1;
        }
    }
}
void launch_gate_detect(const GateDesc* d, int n, uint32_t max_tiles, hipStream_t) { check(d, n, max_tiles, 0); }
void launch_gate_carry(const GateDesc* d, int n, bool affine, hipStream_t) { check(d, n, 0u, affine ? 3 : 1); }
void launch_gate_env(const GateDesc* d, int n, uint32_t max_tiles, hipStream_t) { check(d, n, max_tiles, 2); }
void launch_gate_apply(const GateDesc* d, int n, uint32_t max_tiles, hipStream_t) { check(d, n, max_tiles, 4); }
}  // namespace tdk
