// The compressor launches for the host-only sanitizer build of the engine (TEST INFRASTRUCTURE: linked only by
// tests/test_compressor_host.py beside tests/mock_hip.cpp, never by the product).  Nothing is computed: every launch walks its
// descriptor table and both ends of every array a descriptor points to, so that a descriptor that points past an allocation is
// an AddressSanitizer report, and checks what the kernels rely on -- the tiling, the carry descriptors' lane chunks, that the
// carries read and write the very tile words the vertex' own descriptor names, and that the five launches of a vertex come in
// order (detect, carry y1, env, carry yL, apply).
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <cmath>
#include <map>

#define MOCK_NAME "mock_comp"
#include "mock_util.h"

size_t g_comp_launches[5] = {0, 0, 0, 0, 0}, g_comp_vertices = 0, g_comp_fresh = 0, g_comp_carried = 0;

namespace {
struct Track { int phase; const double* carry1; const double* agg2; const double* carry2; const tdk::CompState* state; uint32_t n_tiles; };
std::map<const double*, Track> g_by_agg1;          // a vertex of the submission under way, by its agg1 words
std::map<const double*, const double*> g_agg2_of;  // agg2 words -> agg1 words
}  // namespace

namespace tdk {
static void check(const CompDesc* d, int n, uint32_t max_tiles, int which) {
    touch(d, (size_t)std::max(n, 0) * sizeof(CompDesc));
    g_comp_launches[which] += 1;
    for (int i = 0; i < n; ++i) {
        const CompDesc& s = d[i];
        if (!s.ins || !s.x || !s.dy || !s.out || !s.state || !s.agg1 || !s.carry1 || !s.agg2 || !s.carry2) die("null pointer in a CompDesc");
        if (!s.frames || s.n_tiles != (s.frames + kCompTile - 1) / kCompTile || s.n_tiles > max_tiles) die("tiling");
        if ((const void*)s.x == (const void*)s.dy || (const void*)s.x == (const void*)s.out || (const void*)s.dy == (const void*)s.out) die("buffers alias");
        if (!(s.wet >= 0.0001f && s.wet <= 1.0f)) die("wet");
        if (!(s.aR > 0.0 && s.aR < 1.0) || !(s.aA >= 0.0 && s.aA < 1.0) || s.oA != 1.0 - s.aA) die("coefficients");
        if (!(s.slope >= 0.0 && s.slope < 1.0) || !(s.thr >= -80.0 && s.thr <= 0.0) || !(s.knee >= 0.0 && s.knee <= 40.0) ||
            !(s.makeup >= -40.0 && s.makeup <= 40.0))
            die("parameters");
        for (int k = 0; k < 8; ++k) {
            const double e = (double)kCompRun * (double)(1u << k);
            if (std::fabs(s.pwR[k] - std::pow(s.aR, e)) > 1e-12 || std::fabs(s.pwA[k] - std::pow(s.aA, e)) > 1e-12) die("powers");
        }
        if ((((uintptr_t)s.x) | ((uintptr_t)s.dy) | ((uintptr_t)s.out)) & 15u) die("alignment");
        touch_terms(s.ins, s.k, s.frames, "a compressor vertex takes terms of kinds 0 .. 4 only");
        touch_w(s.x, (size_t)s.frames * sizeof(float2));
        touch_w(s.dy, (size_t)((s.frames + 1u) & ~1u) * sizeof(double));   // (pairs: an odd chunk's last store covers one frame more)
        touch_w(s.out, (size_t)s.frames * sizeof(float2));
        touch_w(s.state, sizeof(CompState));
        touch_w(s.agg1, (size_t)s.n_tiles * 8);
        touch_w(s.carry1, (size_t)s.n_tiles * 8);
        touch_w(s.agg2, (size_t)s.n_tiles * 8);
        touch_w(s.carry2, (size_t)s.n_tiles * 8);
        if (which == 0) {
            if (g_by_agg1.count(s.agg1) && g_by_agg1[s.agg1].phase != 0) die("a vertex' tile words reused before its launches finished");
            g_by_agg1[s.agg1] = Track{1, s.carry1, s.agg2, s.carry2, s.state, s.n_tiles};
            g_agg2_of[s.agg2] = s.agg1;
            g_comp_vertices += 1;
        } else {
            auto it = g_by_agg1.find(s.agg1);
            const int want = which == 2 ? 2 : 4;
            if (it == g_by_agg1.end() || it->second.phase != want) die("launch order (env / apply)");
            if (it->second.carry1 != s.carry1 || it->second.agg2 != s.agg2 || it->second.carry2 != s.carry2) die("descriptor changed between launches");
            it->second.phase = which == 2 ? 3 : 0;
        }
    }
}
void launch_comp_detect(const CompDesc* d, int n, uint32_t max_tiles, hipStream_t) { check(d, n, max_tiles, 0); }
void launch_comp_env(const CompDesc* d, int n, uint32_t max_tiles, hipStream_t) { check(d, n, max_tiles, 2); }
void launch_comp_apply(const CompDesc* d, int n, uint32_t max_tiles, hipStream_t) { check(d, n, max_tiles, 4); }
// (the engine's only use of this launch in a build without the mastering mocks: a compressor vertex' two carries)
void launch_master_carry(const MasterDesc* d, int n, hipStream_t) {
    touch(d, (size_t)std::max(n, 0) * sizeof(MasterDesc));
    for (int i = 0; i < n; ++i) {
        const MasterDesc& s = d[i];
        if (!s.agg || !s.carry || !s.n_tiles || s.op > 1u) die("carry descriptor");
        if ((size_t)s.chunk * kThreads < s.n_tiles || (s.chunk > 1 && (size_t)(s.chunk - 1) * kThreads >= s.n_tiles)) die("carry lane chunks");
        const double* key = s.agg;
        if (s.op == 1u) {
            auto a = g_agg2_of.find(s.agg);
            if (a == g_agg2_of.end()) die("yL carry over unknown tile words");
            key = a->second;
        }
        auto it = g_by_agg1.find(key);
        if (it == g_by_agg1.end() || it->second.phase != (s.op ? 3 : 1)) die("launch order (carry)");
        const Track& t = it->second;
        if (s.n_tiles != t.n_tiles || s.carry != (s.op ? t.carry2 : t.carry1)) die("carry slot");
        if (s.init && s.init != (s.op ? &t.state->yL : &t.state->y1)) die("carry entry value");
        g_comp_launches[s.op ? 3 : 1] += i == 0 ? 1 : 0;
        if (!s.op) (s.init ? g_comp_carried : g_comp_fresh) += 1;
        if (!(s.a_tile >= 0.0 && s.a_tile < 1.0)) die("carry a_tile");
        for (int k = 0; k < 8; ++k)
            if (!(s.pwc[k] >= 0.0 && s.pwc[k] <= s.a_tile)) die("carry powers");
        touch(s.agg, (size_t)s.n_tiles * 8);
        touch_w(s.carry, (size_t)s.n_tiles * 8);
        if (s.init) touch(s.init, 8);
        it->second.phase += 1;
    }
}
}  // namespace tdk
