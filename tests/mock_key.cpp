// The compressor and gate launches, keyed forms included, for the host-only sanitizer build of the engine (TEST INFRASTRUCTURE:
// linked only by tests/test_key_host.py beside tests/mock_hip.cpp, never by the product; it takes the place of mock_comp.cpp AND
// mock_gate.cpp, which know nothing of key edges and stay as they are).  Nothing is computed: every launch walks its descriptor
// table and both ends of every array a descriptor points to -- the key term table and whatever the key terms point to, and a
// keyed gate's class words, among them -- so that a descriptor that points past an allocation is an AddressSanitizer report, and
// checks what the kernels rely on: the tiling, the carries' lane chunks, that every launch of a vertex reads the descriptor words
// the first one saw, that a vertex' five launches come in order, and that the keyed descriptors of a level go through the keyed
// entry points and no others do (compile_fx.cpp puts them behind the unkeyed ones: a launch is one or the other, never mixed).
// The driver is tests/asan_comp.cpp as it is; its counters keep the names it declares.  g_comp_launches[step] counts the
// DESCRIPTORS that went through each of the five steps (the driver wants the five equal: with a level's detect launch split in
// two that holds per vertex, not per launch).
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <cmath>
#include <map>

#define MOCK_NAME "mock_key"
#include "mock_util.h"

size_t g_comp_launches[5] = {0, 0, 0, 0, 0}, g_comp_vertices = 0, g_comp_fresh = 0, g_comp_carried = 0;
size_t g_key_vertices = 0;   // keyed descriptors seen by a detect launch

namespace {
struct CompTrack { int phase; const double* carry1; const double* agg2; const double* carry2; const tdk::CompState* state; uint32_t n_tiles; };
std::map<const double*, CompTrack> g_by_agg1;
std::map<const double*, const double*> g_agg2_of;
struct GateTrack { int phase; tdk::GateDesc first; };
std::map<const uint32_t*, GateTrack> g_by_map;
struct Summary { ~Summary() { printf("mock_key: %zu keyed descriptors detected\n", g_key_vertices); } } g_summary;

// the key side of a descriptor: `keyed` says which entry point the launch came through (carries and apply: either)
template <class D>
void check_key(const D& s, int keyed) {
    const bool has = s.key_ins != nullptr;
    if (has != (s.key_k != 0u)) die("key term table and key count disagree");
    if (keyed >= 0 && has != (keyed == 1)) die(keyed ? "an unkeyed descriptor in a keyed launch" : "a keyed descriptor in an unkeyed launch");
    if (!has) {
        if (s.key_term_mode != 0u) die("key term mode without key terms");
        return;
    }
    if ((const void*)s.key_ins == (const void*)s.ins) die("key terms alias the input terms");
    touch_terms(s.key_ins, s.key_k, s.frames, "a key term is of kinds 0 .. 4 only");
    for (uint32_t i = 0; i < s.key_k; ++i)
        if ((s.key_ins[i].kind == 0u || s.key_ins[i].kind == 4u) && ((const void*)s.key_ins[i].p == (const void*)s.x || (const void*)s.key_ins[i].p == (const void*)s.out))
            die("a key term reads the vertex' own buffers");
}
}  // namespace

namespace tdk {
// ---- compressor (mock_comp.cpp's checks, and the key's) ----
static void check_comp(const CompDesc* d, int n, uint32_t max_tiles, int which, int keyed) {
    touch(d, (size_t)std::max(n, 0) * sizeof(CompDesc));
    g_comp_launches[which] += (size_t)std::max(n, 0);
    for (int i = 0; i < n; ++i) {
        const CompDesc& s = d[i];
        if (!s.ins || !s.x || !s.dy || !s.out || !s.state || !s.agg1 || !s.carry1 || !s.agg2 || !s.carry2) die("null pointer in a CompDesc");
        if (!s.frames || s.n_tiles != (s.frames + kCompTile - 1) / kCompTile || s.n_tiles > max_tiles) die("tiling");
        if ((const void*)s.x == (const void*)s.dy || (const void*)s.x == (const void*)s.out || (const void*)s.dy == (const void*)s.out) die("buffers alias");
        if (!(s.wet >= 0.0001f && s.wet <= 1.0f)) die("wet");
        if (!(s.aR > 0.0 && s.aR < 1.0) || !(s.aA >= 0.0 && s.aA < 1.0) || s.oA != 1.0 - s.aA) die("coefficients");
        if ((((uintptr_t)s.x) | ((uintptr_t)s.dy) | ((uintptr_t)s.out)) & 15u) die("alignment");
        touch_terms(s.ins, s.k, s.frames, "a compressor vertex takes terms of kinds 0 .. 4 only");
        check_key(s, keyed);
        touch_w(s.x, (size_t)s.frames * sizeof(float2));
        touch_w(s.dy, (size_t)((s.frames + 1u) & ~1u) * sizeof(double));
        touch_w(s.out, (size_t)s.frames * sizeof(float2));
        touch_w(s.state, sizeof(CompState));
        touch_w(s.agg1, (size_t)s.n_tiles * 8);
        touch_w(s.carry1, (size_t)s.n_tiles * 8);
        touch_w(s.agg2, (size_t)s.n_tiles * 8);
        touch_w(s.carry2, (size_t)s.n_tiles * 8);
        if (which == 0) {
            if (g_by_agg1.count(s.agg1) && g_by_agg1[s.agg1].phase != 0) die("a vertex' tile words reused before its launches finished");
            g_by_agg1[s.agg1] = CompTrack{1, s.carry1, s.agg2, s.carry2, s.state, s.n_tiles};
            g_agg2_of[s.agg2] = s.agg1;
            g_comp_vertices += 1;
            g_key_vertices += s.key_ins ? 1 : 0;
        } else {
            auto it = g_by_agg1.find(s.agg1);
            const int want = which == 2 ? 2 : 4;
            if (it == g_by_agg1.end() || it->second.phase != want) die("launch order (env / apply)");
            if (it->second.carry1 != s.carry1 || it->second.agg2 != s.agg2 || it->second.carry2 != s.carry2) die("descriptor changed between launches");
            it->second.phase = which == 2 ? 3 : 0;
        }
    }
}
void launch_comp_detect(const CompDesc* d, int n, uint32_t max_tiles, hipStream_t) { check_comp(d, n, max_tiles, 0, 0); }
void launch_comp_detect_keyed(const CompDesc* d, int n, uint32_t max_tiles, hipStream_t) { check_comp(d, n, max_tiles, 0, 1); }
void launch_comp_env(const CompDesc* d, int n, uint32_t max_tiles, hipStream_t) { check_comp(d, n, max_tiles, 2, -1); }
void launch_comp_apply(const CompDesc* d, int n, uint32_t max_tiles, hipStream_t) { check_comp(d, n, max_tiles, 4, -1); }
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
        const CompTrack& t = it->second;
        if (s.n_tiles != t.n_tiles || s.carry != (s.op ? t.carry2 : t.carry1)) die("carry slot");
        if (s.init && s.init != (s.op ? &t.state->yL : &t.state->y1)) die("carry entry value");
        g_comp_launches[s.op ? 3 : 1] += 1;
        if (!s.op) (s.init ? g_comp_carried : g_comp_fresh) += 1;
        touch(s.agg, (size_t)s.n_tiles * 8);
        touch_w(s.carry, (size_t)s.n_tiles * 8);
        if (s.init) touch(s.init, 8);
        it->second.phase += 1;
    }
}

// ---- gate (mock_gate.cpp's checks, and the key's) ----
static void check_gate(const GateDesc* d, int n, uint32_t max_tiles, int which, int keyed) {
    touch(d, (size_t)std::max(n, 0) * sizeof(GateDesc));
    g_comp_launches[which] += (size_t)std::max(n, 0);
    const bool carry = which == 1 || which == 3;
    for (int i = 0; i < n; ++i) {
        const GateDesc& s = d[i];
        if (!s.ins || !s.x || !s.out || !s.state || !s.map || !s.carry_hc || !s.tbits || !s.aggA || !s.aggB || !s.carry_env) die("null pointer in a GateDesc");
        if (s.init && s.init != s.state) die("entry state");
        if (!s.frames || s.n_tiles != (s.frames + kGateTile - 1) / kGateTile || (!carry && s.n_tiles > max_tiles)) die("tiling");
        if ((size_t)s.chunk * kThreads < s.n_tiles || (s.chunk > 1 && (size_t)(s.chunk - 1) * kThreads >= s.n_tiles)) die("carry lane chunks");
        if ((const void*)s.x == (const void*)s.out) die("buffers alias");
        if (!(s.wet >= 0.0001f && s.wet <= 1.0f)) die("wet");
        if (!s.cap || s.cap > kGateK) die("hold counter's room");
        if ((((uintptr_t)s.x) | ((uintptr_t)s.out)) & 15u) die("alignment");
        touch_terms(s.ins, s.k, s.frames, "a gate vertex takes terms of kinds 0 .. 4 only");
        check_key(s, keyed);
        // the class words: there exactly when the vertex is keyed, one 16-bit word per lane, apart from the other tile words
        if ((s.cls != nullptr) != (s.key_ins != nullptr)) die("class words and key terms disagree");
        if (((uintptr_t)s.cls) & 1u) die("class words' alignment");
        touch_w(s.cls, (size_t)s.n_tiles * kThreads * sizeof(uint16_t));
        touch_w(s.x, (size_t)((s.frames + 1u) & ~1u) * sizeof(float2));
        touch_w(s.out, (size_t)((s.frames + 1u) & ~1u) * sizeof(float2));
        touch_w(s.state, sizeof(GateState));
        const uintptr_t a[7] = {(uintptr_t)s.map, (uintptr_t)s.carry_hc, (uintptr_t)s.tbits, (uintptr_t)s.aggA, (uintptr_t)s.aggB, (uintptr_t)s.carry_env, (uintptr_t)s.cls};
        const size_t b[7] = {(size_t)s.n_tiles * 8, (size_t)s.n_tiles * 4, (size_t)s.n_tiles * kThreads, (size_t)s.n_tiles * 8, (size_t)s.n_tiles * 8, (size_t)s.n_tiles * 8,
                             (size_t)s.n_tiles * kThreads * sizeof(uint16_t)};
        const int na = s.cls ? 7 : 6;
        for (int p = 0; p < na; ++p) {
            touch_w((void*)a[p], b[p]);
            for (int q = p + 1; q < na; ++q)
                if (a[p] < a[q] + b[q] && a[q] < a[p] + b[p]) die("tile words overlap");
        }
        if (which == 0) {
            if (g_by_map.count(s.map) && g_by_map[s.map].phase != 0) die("a vertex' tile words reused before its launches finished");
            g_by_map[s.map] = GateTrack{1, s};
            g_comp_vertices += 1;
            g_key_vertices += s.key_ins ? 1 : 0;
            (s.init ? g_comp_carried : g_comp_fresh) += 1;
        } else {
            auto it = g_by_map.find(s.map);
            if (it == g_by_map.end() || it->second.phase != which) die("launch order");
            const GateDesc& f = it->second.first;
            if (f.carry_hc != s.carry_hc || f.tbits != s.tbits || f.aggA != s.aggA || f.aggB != s.aggB || f.carry_env != s.carry_env || f.x != s.x ||
                f.out != s.out || f.state != s.state || f.init != s.init || f.cap != s.cap || f.frames != s.frames || f.cls != s.cls ||
                f.key_ins != s.key_ins || f.key_k != s.key_k)
                die("descriptor changed between launches");
            it->second.phase = which == 4 ? 0 : which + 1;
        }
    }
}
void launch_gate_detect(const GateDesc* d, int n, uint32_t max_tiles, hipStream_t) { check_gate(d, n, max_tiles, 0, 0); }
void launch_gate_detect_keyed(const GateDesc* d, int n, uint32_t max_tiles, hipStream_t) { check_gate(d, n, max_tiles, 0, 1); }
void launch_gate_carry(const GateDesc* d, int n, bool affine, hipStream_t) { check_gate(d, n, 0u, affine ? 3 : 1, -1); }
void launch_gate_env(const GateDesc* d, int n, uint32_t max_tiles, hipStream_t) { check_gate(d, n, max_tiles, 2, 0); }
void launch_gate_env_keyed(const GateDesc* d, int n, uint32_t max_tiles, hipStream_t) { check_gate(d, n, max_tiles, 2, 1); }
void launch_gate_apply(const GateDesc* d, int n, uint32_t max_tiles, hipStream_t) { check_gate(d, n, max_tiles, 4, -1); }
}  // namespace tdk
