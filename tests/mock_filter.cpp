// The filter launches for the host-only sanitizer build of the engine (TEST INFRASTRUCTURE: linked only by
// tests/test_filter_host.py beside tests/mock_hip.cpp, never by the product).  Nothing is computed: every launch walks its
// descriptor table and both ends of every array a descriptor points to, so that a descriptor that points past an allocation is
// an AddressSanitizer report, and checks what the kernels rely on -- the tiling, the scratch sizes of the level words, the tile
// maps and the carried states, the follower's powers and its carry descriptors' lane chunks, that the carries read and write the
// very tile words the vertex' own descriptor names, that every launch of a vertex reads the descriptor words the first one saw,
// that a keyed launch holds keyed descriptors only, and that the launches of a vertex come in order: detect, carry y1, env,
// carry e (a vertex whose follower runs), local, carry, apply for a chunk of several tiles; apply alone (the single form, entered
// with the carried state) for a chunk of one.
// The driver is tests/asan_comp.cpp as it is: its counters keep the names it declares (g_comp_*), counting filter launches
// here -- one per apply launch, on every step's counter, since a one-tile chunk has no other step.
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <cmath>
#include <map>

#define MOCK_NAME "mock_filter"
#include "mock_util.h"

size_t g_comp_launches[5] = {0, 0, 0, 0, 0}, g_comp_vertices = 0, g_comp_fresh = 0, g_comp_carried = 0;

namespace {
enum { DETECT = 0, CARRY1, ENV, CARRY2, LOCAL, CARRY, APPLY };
struct Track { int phase; tdk::FiltDesc first; };
std::map<const double*, Track> g_by_agg;           // a vertex of the submission under way, by its tile maps
std::map<const double*, const double*> g_agg_of;   // agg1 / agg2 words -> the vertex' tile maps
}  // namespace

namespace tdk {
static void check(const FiltDesc* d, int n, uint32_t n_tiles, bool single, bool keyed, int which) {
    touch(d, (size_t)std::max(n, 0) * sizeof(FiltDesc));
    if (which == APPLY) for (int i = 0; i < 5; ++i) g_comp_launches[i] += 1;
    for (int i = 0; i < n; ++i) {
        const FiltDesc& s = d[i];
        if (!s.ins || !s.out || !s.state) die("null pointer in a FiltDesc");
        if (s.init && s.init != s.state) die("entry state");
        if (!s.frames || s.n_tiles != (s.frames + kFiltTile - 1) / kFiltTile) die("tiling");
        if (which != CARRY && s.n_tiles != n_tiles) die("grid");
        if (single != (s.n_tiles == 1u) || (single && which != APPLY)) die("the one-launch form is for one tile, and k_filt_apply's alone");
        if (single ? (s.x || s.lv || s.agg || s.carry || s.agg1 || s.carry1 || s.agg2 || s.carry2) : (!s.x || !s.agg || !s.carry)) die("scratch of the wrong form");
        if (!single && (s.env ? (!s.lv || !s.agg1 || !s.carry1 || !s.agg2 || !s.carry2) : (s.lv || s.agg1 || s.carry1 || s.agg2 || s.carry2))) die("the follower's scratch");
        if ((which == DETECT || which == ENV) && !s.env) die("a follower launch over a vertex whose follower does not run");
        if (s.env > 1u || (s.env != 0u) != (s.ce != 0.0)) die("env");
        if ((s.key_ins != nullptr) != (s.key_k != 0u) || (s.key_ins && !s.env)) die("key fields");
        if ((which == DETECT || (which == APPLY && single)) && keyed != (s.key_ins != nullptr)) die("a vertex in the launch of the other key form");
        if ((const void*)s.x == (const void*)s.out || (s.lv && ((const void*)s.lv == (const void*)s.x || (const void*)s.lv == (const void*)s.out))) die("buffers alias");
        if (!(s.wet >= 0.0001f && s.wet <= 1.0f)) die("wet");
        if (s.kind > 3u || s.shape > 1u || !(s.f > 0.0 && s.f <= 20.0 / 8000.0) || !(s.stereo >= 0.0 && s.stereo <= 0.5)) die("parameters");
        if (!(s.gmin > 0.0 && s.gmin <= s.g0 && s.g0 <= s.gmax * 1.000001 && s.gmax < 6.4) || !(s.kq >= 1.0 / 30.0001 && s.kq <= 2.0)) die("filter constants");
        if (!(std::fabs(s.cl) <= 2.7726) || !(std::fabs(s.ce) <= 5.5452) || !(s.S >= 1.0 && s.S <= 1000.0001)) die("sweep constants");
        if (!(s.aR > 0.0 && s.aR < 1.0) || !(s.aA >= 0.0 && s.aA < 1.0) || s.oA != 1.0 - s.aA) die("coefficients");
        for (int k = 0; k < 8; ++k) {
            const double e = (double)kFiltRun * (double)(1u << k);
            if (std::fabs(s.pwR[k] - std::pow(s.aR, e)) > 1e-12 || std::fabs(s.pwA[k] - std::pow(s.aA, e)) > 1e-12) die("powers");
        }
        if ((((uintptr_t)s.x) | ((uintptr_t)s.out) | ((uintptr_t)s.lv) | ((uintptr_t)s.carry) | ((uintptr_t)&s.state->z[0][0])) & 15u) die("alignment");
        if ((((uintptr_t)s.agg) | ((uintptr_t)s.agg1) | ((uintptr_t)s.carry1) | ((uintptr_t)s.agg2) | ((uintptr_t)s.carry2) | ((uintptr_t)s.state)) & 7u) die("doubles' alignment");
        touch_terms(s.ins, s.k, s.frames, "a filter vertex takes terms of kinds 0 .. 4 only");
        if (s.key_ins) touch_terms(s.key_ins, s.key_k, s.frames, "a filter vertex takes key terms of kinds 0 .. 4 only");
        const size_t even = (size_t)((s.frames + 1u) & ~1u);   // (pairs: an odd chunk's last store covers one frame more)
        if (s.x) touch_w(s.x, even * sizeof(float2));
        if (s.lv) touch_w(s.lv, even * sizeof(double));
        touch_w(s.out, even * sizeof(float2));
        touch_w(s.state, sizeof(FiltState));
        const size_t ab = (size_t)s.n_tiles * 12 * sizeof(double), cb = (size_t)s.n_tiles * 4 * sizeof(double), tb = (size_t)s.n_tiles * sizeof(double);
        if (!single) {
            touch_w(s.agg, ab);
            touch_w(s.carry, cb);
            const uintptr_t a = (uintptr_t)s.agg, c = (uintptr_t)s.carry;
            if (a < c + cb && c < a + ab) die("tile words overlap");
            if (s.env) {
                double* const w[4] = {s.agg1, s.carry1, s.agg2, s.carry2};
                for (int j = 0; j < 4; ++j) {
                    touch_w(w[j], tb);
                    for (int l = 0; l < j; ++l)
                        if ((uintptr_t)w[j] < (uintptr_t)w[l] + tb && (uintptr_t)w[l] < (uintptr_t)w[j] + tb) die("the follower's tile words overlap");
                }
            }
        }
        if (which == APPLY) {
            g_comp_vertices += 1;
            (s.init ? g_comp_carried : g_comp_fresh) += 1;
        }
        if (single) continue;
        const int first = s.env ? DETECT : LOCAL;
        if (which == first) {
            if (g_by_agg.count(s.agg) && g_by_agg[s.agg].phase != 0) die("a vertex' tile words reused before its launches finished");
            g_by_agg[s.agg] = Track{which + 1, s};
            if (s.env) { g_agg_of[s.agg1] = s.agg; g_agg_of[s.agg2] = s.agg; }
        } else {
            auto it = g_by_agg.find(s.agg);
            if (it == g_by_agg.end() || it->second.phase != which) die("launch order");
            const FiltDesc& f = it->second.first;
            if (f.carry != s.carry || f.x != s.x || f.lv != s.lv || f.out != s.out || f.state != s.state || f.init != s.init || f.t0 != s.t0 ||
                f.frames != s.frames || f.agg1 != s.agg1 || f.carry1 != s.carry1 || f.agg2 != s.agg2 || f.carry2 != s.carry2 || f.env != s.env)
                die("descriptor changed between launches");
            it->second.phase = which == APPLY ? 0 : which + 1;
        }
    }
}
void launch_filt_detect(const FiltDesc* d, int n, uint32_t n_tiles, bool keyed, hipStream_t) { check(d, n, n_tiles, false, keyed, DETECT); }
void launch_filt_env(const FiltDesc* d, int n, uint32_t n_tiles, hipStream_t) { check(d, n, n_tiles, false, false, ENV); }
void launch_filt_local(const FiltDesc* d, int n, uint32_t n_tiles, hipStream_t) { check(d, n, n_tiles, false, false, LOCAL); }
void launch_filt_carry(const FiltDesc* d, int n, hipStream_t) { check(d, n, 0u, false, false, CARRY); }
void launch_filt_apply(const FiltDesc* d, int n, uint32_t n_tiles, bool single, bool keyed, hipStream_t) { check(d, n, n_tiles, single, keyed, APPLY); }
// (the engine's only use of this launch in a build without the mastering and compressor mocks: a filter vertex' follower carries)
void launch_master_carry(const MasterDesc* d, int n, hipStream_t) {
    touch(d, (size_t)std::max(n, 0) * sizeof(MasterDesc));
    for (int i = 0; i < n; ++i) {
        const MasterDesc& s = d[i];
        if (!s.agg || !s.carry || !s.n_tiles || s.op > 1u) die("carry descriptor");
        if ((size_t)s.chunk * kThreads < s.n_tiles || (s.chunk > 1 && (size_t)(s.chunk - 1) * kThreads >= s.n_tiles)) die("carry lane chunks");
        auto a = g_agg_of.find(s.agg);
        if (a == g_agg_of.end()) die("a follower carry over unknown tile words");
        auto it = g_by_agg.find(a->second);
        if (it == g_by_agg.end() || it->second.phase != (s.op ? CARRY2 : CARRY1)) die("launch order (follower carry)");
        const FiltDesc& f = it->second.first;
        if (s.n_tiles != f.n_tiles || s.agg != (s.op ? f.agg2 : f.agg1) || s.carry != (s.op ? f.carry2 : f.carry1)) die("carry slot");
        if ((s.init != nullptr) != (f.init != nullptr) || (s.init && s.init != (s.op ? &f.state->e : &f.state->y1))) die("carry entry value");
        const double c = s.op ? f.aA : f.aR;
        if (std::fabs(s.a_tile - std::pow(c, (double)kFiltTile)) > 1e-12) die("carry a_tile");
        for (int k = 0; k < 8; ++k)
            if (std::fabs(s.pwc[k] - std::pow(c, (double)kFiltTile * (double)s.chunk * (double)(1u << k))) > 1e-12) die("carry powers");
        touch(s.agg, (size_t)s.n_tiles * 8);
        touch_w(s.carry, (size_t)s.n_tiles * 8);
        it->second.phase += 1;
    }
}
}  // namespace tdk
