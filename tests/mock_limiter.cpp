// The limiter launches for the host-only sanitizer build of the engine (TEST INFRASTRUCTURE: linked only by
// tests/test_limiter_host.py beside tests/mock_hip.cpp and tests/mock_guard.cpp, never by the product).  Nothing is computed: every
// launch walks its descriptor table and both ends of every array a descriptor points to, so that a descriptor that points past an
// allocation is an AddressSanitizer report, and checks what the kernels rely on: the tiling (2 048-frame tiles, the carry's lane
// chunks), the window (1 .. 2 048 frames: the halo within one tile), the constants (c, gin, a and its powers), the scratch ranges
// (x, q, agg, carry: there exactly in the three-launch form, apart from each other), the line (two halves of 2 L doubles; `fresh`
// exactly when the vertex has not run since it restarted, always right after a set_time; otherwise the half it reads is one a
// launch wrote whole), that the carry in between is k_master_carry with op 0 over the vertex' own tile words and enters with word
// 0 of the half the vertex reads, that a vertex' three launches come in order with the descriptor the first one saw, and that a
// chunk of one tile is k_lim_apply alone.
// With g_fx_force_redo set the guard's listeners (tests/mock_guard.cpp) tell every audited render to run again.  For that case
// k_lim_apply stamps the half it writes and logs the stamp it finds in the half it reads: a render done again must find what the
// first one found.
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <map>
#include <vector>

#define MOCK_NAME "mock_limiter"
#include "mock_util.h"
#include "asan_fx.h"
#include "termdaw_amd.h"

size_t g_fx_launches[3] = {0, 0, 0}, g_fx_vertices = 0, g_fx_single = 0, g_fx_fresh = 0, g_fx_carried = 0;   // [0] k_lim_detect, [1] k_master_carry, [2] k_lim_apply: descriptors
int g_fx_after_set_time = 0;
size_t g_fx_restarts = 0;
size_t g_fx_short = 0;         // (descriptors whose chunk was shorter than the halo: frames < L - 1)
std::vector<double> g_fx_entry_log;
static double g_fx_stamp = 0.0;

namespace {
enum { DETECT = 0, CARRY = 1, APPLY = 2 };
struct Track { int phase; tdk::LimDesc first; };
std::map<const double*, Track> g_by_agg;      // three-launch vertices between k_lim_detect and k_lim_apply
std::map<const double*, bool> g_line_ran;     // line -> it has been written since it restarted
}  // namespace

namespace tdk {
static void check(const LimDesc* d, int n, uint32_t n_tiles, bool single, int which) {
    touch(d, (size_t)std::max(n, 0) * sizeof(LimDesc));
    if (n <= 0) die("an empty launch");
    for (int i = 0; i < n; ++i) {
        const LimDesc& s = d[i];
        if (!s.ins || !s.out || !s.line) die("null pointer in a LimDesc");
        if (!s.frames || s.n_tiles != (s.frames + kLimTile - 1) / kLimTile || s.n_tiles != n_tiles) die("tiling");
        const bool multi = s.n_tiles > 1u;
        if (single == multi) die("the form against the tile count");
        if (!multi && which != APPLY) die("a chunk of one tile is k_lim_apply alone");
        if (!(s.wet >= 0.0001f && s.wet <= 1.0f)) die("wet");
        if (!(s.L >= 1u && s.L <= kLimTile)) die("the window: the halo lies within one tile");
        if (s.parity > 1u || s.fresh > 1u) die("parity / fresh");
        if (!(s.c > 0.063 && s.c <= 1.0) || !(s.gin > 0.063 && s.gin < 15.85) || !(s.a > 0.0 && s.a < 1.0)) die("constants");
        for (int k = 0; k < 8; ++k)
            if (std::fabs(s.pw[k] - std::pow(s.a, (double)kLimRun * (double)(1u << k))) > 1e-12) die("release powers");
        if ((((uintptr_t)s.out) & 15u) || (((uintptr_t)s.line) & 7u)) die("alignment");
        touch_terms(s.ins, s.k, s.frames, "a limiter vertex takes terms of kinds 0 .. 4 only");
        touch_w(s.out, (size_t)((s.frames + 1u) & ~1u) * sizeof(float2));
        const size_t half = (size_t)2 * s.L;
        touch_w(s.line, 2 * half * sizeof(double));
        if (!multi) {
            if (s.x || s.q || s.agg || s.carry) die("scratch in the one-launch form");
        } else {
            if (!s.x || !s.q || !s.agg || !s.carry) die("null scratch pointer in the three-launch form");
            if ((const void*)s.x == (const void*)s.out || (const void*)s.q == (const void*)s.out || (const void*)s.q == (const void*)s.x) die("buffers alias");
            if ((((uintptr_t)s.x) | ((uintptr_t)s.q)) & 15u) die("scratch alignment");
            touch_w(s.x, (size_t)((s.frames + 1u) & ~1u) * sizeof(float2));
            touch_w(s.q, (size_t)s.frames * sizeof(float));
            const size_t tb = (size_t)s.n_tiles * sizeof(double);
            const uintptr_t a = (uintptr_t)s.agg, c = (uintptr_t)s.carry;
            if ((a | c) & 7u) die("tile words' alignment");
            touch_w(s.agg, tb);
            touch_w(s.carry, tb);
            if (a < c + tb && c < a + tb) die("tile words overlap");
            // the order of a vertex' launches, with the descriptor the first one saw
            if (which == DETECT) {
                if (g_by_agg.count(s.agg) && g_by_agg[s.agg].phase != 0) die("a vertex' tile words reused before its launches finished");
                g_by_agg[s.agg] = Track{CARRY, s};
            } else {
                auto it = g_by_agg.find(s.agg);
                if (it == g_by_agg.end() || it->second.phase != APPLY) die("launch order");
                if (memcmp(&it->second.first, &s, sizeof s) != 0) die("descriptor changed between launches");
                it->second.phase = 0;
            }
        }
        if (which == DETECT) { g_fx_launches[0] += 1; continue; }
        // ---- k_lim_apply: the line's books
        g_fx_launches[2] += 1;
        g_fx_vertices += 1;
        if (single) g_fx_single += 1;
        if (s.frames + 1u < s.L) g_fx_short += 1;
        (s.fresh ? g_fx_fresh : g_fx_carried) += 1;
        if (g_fx_after_set_time) {
            if (!s.fresh) die("a vertex entered with its line after a set_time");
            g_fx_restarts += 1;
        }
        const double* lr = s.line + (size_t)s.parity * half;
        double* lw = s.line + (size_t)(s.parity ^ 1u) * half;
        if (!s.fresh) {
            if (!g_line_ran[s.line]) die("a vertex enters with a line nothing has written");
            if (!(lr[0] > 0.0) || lr[0] != lr[half - 1]) die("the half a vertex reads was not written whole by one launch");
            g_fx_entry_log.push_back(lr[0]);
        }
        g_line_ran[s.line] = true;
        g_fx_stamp += 1.0;
        for (size_t m = 0; m < half; ++m) lw[m] = g_fx_stamp;
    }
}
void launch_lim_detect(const LimDesc* d, int n, uint32_t n_tiles, hipStream_t) { check(d, n, n_tiles, false, DETECT); }
void launch_lim_apply(const LimDesc* d, int n, uint32_t n_tiles, bool single, hipStream_t) { check(d, n, n_tiles, single, APPLY); }
// (the engine's only use of this launch in a build without the mastering, compressor and filter mocks: a limiter vertex' carry)
void launch_master_carry(const MasterDesc* d, int n, hipStream_t) {
    touch(d, (size_t)std::max(n, 0) * sizeof(MasterDesc));
    if (n <= 0) die("an empty carry launch");
    for (int i = 0; i < n; ++i) {
        const MasterDesc& s = d[i];
        if (!s.agg || !s.carry || !s.n_tiles || s.op != 0u) die("carry descriptor");
        if ((size_t)s.chunk * kThreads < s.n_tiles || (s.chunk > 1 && (size_t)(s.chunk - 1) * kThreads >= s.n_tiles)) die("carry lane chunks");
        auto it = g_by_agg.find(s.agg);
        if (it == g_by_agg.end() || it->second.phase != CARRY) die("launch order (carry)");
        const LimDesc& f = it->second.first;
        if (s.n_tiles != f.n_tiles || s.carry != f.carry) die("carry slot");
        if ((s.init == nullptr) != (f.fresh != 0u) || (s.init && s.init != f.line + (size_t)f.parity * 2u * f.L)) die("carry entry value");
        if (std::fabs(s.a_tile - std::pow(f.a, (double)kLimTile)) > 1e-12) die("carry a_tile");
        for (int k = 0; k < 8; ++k)
            if (std::fabs(s.pwc[k] - std::pow(f.a, (double)kLimTile * (double)s.chunk * (double)(1u << k))) > 1e-12) die("carry powers");
        touch(s.agg, (size_t)s.n_tiles * 8);
        touch_w(s.carry, (size_t)s.n_tiles * 8);
        if (s.init) touch(s.init, 8);
        it->second.phase = APPLY;
        g_fx_launches[1] += 1;
    }
}
}  // namespace tdk

// ---- what tests/asan_fx.cpp needs to know about the kind: no debug.* options; the 4 096-frame chunks are two tiles
const FxHooks g_fx = {
    "limiter",
    [](td_state*, int, int) {},
    []() {
        if (g_fx_launches[0] == g_fx_launches[1] && g_fx_launches[2] >= g_fx_launches[0]) return true;   // (three-launch vertices pass all steps)
        fprintf(stderr, "descriptor counts: k_lim_detect %zu k_master_carry %zu k_lim_apply %zu\n", g_fx_launches[0], g_fx_launches[1], g_fx_launches[2]);
        return false;
    },
    []() {
        printf("k_lim_apply descriptors %zu (%zu vertices, %zu one-launch, %zu entered fresh, %zu entered with the line; %zu k_lim_detect descriptors; "
               "%zu restarts checked; %zu short chunks)\n",
               g_fx_launches[2], g_fx_vertices, g_fx_single, g_fx_fresh, g_fx_carried, g_fx_launches[0], g_fx_restarts, g_fx_short);
    },
};
