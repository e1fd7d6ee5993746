// The multiband launches for the host-only sanitizer build of the engine (TEST INFRASTRUCTURE: linked only by
// tests/test_multiband_host.py beside tests/mock_hip.cpp and tests/mock_guard.cpp, never by the product).  Nothing is computed:
// every launch walks its descriptor table and both ends of every array a descriptor points to -- the block table among them -- so
// that a descriptor that points past an allocation is an AddressSanitizer report, and checks what the kernels rely on: the tiling
// (2 048-frame tiles, the carries' lane chunks), the constants (the five coefficient sets: L and H share their poles, A2 shares
// L2's and is the mirror image of its denominator; slopes, aA, aR and their powers), the block table (23 finite blocks per power,
// A^8 = pw[0] against eight frames of the cascade), the scratch ranges (x, the three dy, the tile words: apart from each other),
// the line (42 doubles; entered -- `init` -- exactly when the vertex has run since it restarted, never right after a set_time),
// that a vertex' seven launches come in order with the descriptor the first one saw -- the two scalar carries and k_comp_env over
// three descriptors per vertex that point into the same buffers and into the line -- and that a chunk of one tile is k_mb_apply
// alone.
// With g_fx_force_redo set the guard's listeners (tests/mock_guard.cpp) tell every audited render to run again.  For that case
// k_mb_apply stamps the line and logs the stamp it finds on entry: a render done again must find what the first one found.
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <map>
#include <vector>

#define MOCK_NAME "mock_multiband"
#include "mock_util.h"
#include "asan_fx.h"
#include "multiband_math.h"
#include "termdaw_amd.h"

size_t g_fx_launches[3] = {0, 0, 0}, g_fx_vertices = 0, g_fx_single = 0, g_fx_fresh = 0, g_fx_carried = 0;   // [0] k_mb_local, [1] k_comp_env, [2] k_mb_apply: descriptors
int g_fx_after_set_time = 0;
size_t g_fx_restarts = 0;
size_t g_fx_short = 0;         // (descriptors of one-tile chunks that carried a partial tile: frames < 2 048)
std::vector<double> g_fx_entry_log;
static double g_fx_stamp = 0.0;

namespace {
enum { LOCAL = 0, CARRY = 1, DETECT = 2, CARRY1 = 3, ENV = 4, CARRY2 = 5, APPLY = 6 };
struct Track { int phase; int seen; tdk::MbDesc first; const double* agg2[3]; };
std::map<const double*, Track> g_by_agg;                          // seven-launch vertices between k_mb_local and k_mb_apply
std::map<const double*, std::pair<const double*, int>> g_band;    // agg1[b] / agg2[b] -> (the vertex' agg, b)
std::map<const double*, bool> g_line_ran;                         // line -> it has been written since it restarted

Track& band_of(const double* agg, int phase, int* b, const char* what) {
    auto it = g_band.find(agg);
    if (it == g_band.end()) die(what);
    auto jt = g_by_agg.find(it->second.first);
    if (jt == g_by_agg.end() || jt->second.phase != phase) die(what);
    *b = it->second.second;
    return jt->second;
}
void advance(Track& t, int next) {   // (a band launch holds three descriptors per vertex)
    if (++t.seen == 3) { t.seen = 0; t.phase = next; }
}
}  // namespace

namespace tdk {
static void check(const MbDesc* d, int n, uint32_t n_tiles, bool single, int which) {
    touch(d, (size_t)std::max(n, 0) * sizeof(MbDesc));
    if (n <= 0) die("an empty launch");
    for (int i = 0; i < n; ++i) {
        const MbDesc& s = d[i];
        if (!s.ins || !s.out || !s.line || !s.pow || !s.x || !s.dy[0] || !s.dy[1] || !s.dy[2]) die("null pointer in an MbDesc");
        if (!s.frames || s.n_tiles != (s.frames + kMbTile - 1) / kMbTile || (which != CARRY && s.n_tiles != n_tiles)) die("tiling");
        if ((size_t)s.chunk * kThreads < s.n_tiles || (s.chunk > 1 && (size_t)(s.chunk - 1) * kThreads >= s.n_tiles)) die("carry lane chunks");
        const bool multi = s.n_tiles > 1u;
        if (single == multi) die("the form against the tile count");
        if (!multi && which != APPLY) die("a chunk of one tile is k_mb_apply alone");
        if (!(s.wet >= 0.0001f && s.wet <= 1.0f)) die("wet");
        // the coefficient sets: L1 H1 L2 H2 A2
        for (int p = 0; p < 2; ++p) {
            const double *lo = s.co[2 * p], *hi = s.co[2 * p + 1];
            if (lo[3] != hi[3] || lo[4] != hi[4]) die("a low-pass and its high-pass share their poles");
            if (!(lo[0] > 0.0) || lo[1] != 2.0 * lo[0] || lo[2] != lo[0] || !(hi[0] > 0.0) || hi[1] != -2.0 * hi[0] || hi[2] != hi[0]) die("crossover numerators");
            if (!(lo[4] > 0.0 && lo[4] < 1.0) || !(std::fabs(lo[3]) < 1.0 + lo[4])) die("crossover poles outside the unit circle");
        }
        if (s.co[4][3] != s.co[2][3] || s.co[4][4] != s.co[2][4] || s.co[4][0] != s.co[4][4] || s.co[4][1] != s.co[4][3] || s.co[4][2] != 1.0) die("the all-pass");
        if (!(s.aR > 0.0 && s.aR < 1.0) || !(s.aA >= 0.0 && s.aA < 1.0) || s.oA != 1.0 - s.aA || !(s.knee >= 0.0 && s.knee <= 40.0)) die("detector constants");
        for (int b = 0; b < 3; ++b)
            if (!(s.thr[b] >= -60.0 && s.thr[b] <= 0.0) || !(s.slope[b] >= 0.0 && s.slope[b] < 1.0) || !(std::fabs(s.makeup[b]) <= 40.0)) die("band constants");
        for (int k = 0; k < 8; ++k)
            if (std::fabs(s.pwR[k] - std::pow(s.aR, (double)kMbRun * (double)(1u << k))) > 1e-12 ||
                std::fabs(s.pwA[k] - std::pow(s.aA, (double)kMbRun * (double)(1u << k))) > 1e-12) die("detector powers");
        if ((((uintptr_t)s.out) & 15u) || (((uintptr_t)s.line) & 15u) || (((uintptr_t)s.pow) & 15u)) die("alignment");
        if (s.init && s.init != s.line) die("entry state");
        // the block table: finite everywhere; pw[0] is eight frames of the cascade from a unit state
        touch(s.pow, sizeof(MbPowers));
        for (int k = 0; k < 8; ++k)
            for (uint32_t e = 0; e < kMbBlocks * 4; ++e)
                if (!std::isfinite(s.pow->pw[k][e]) || !std::isfinite(s.pow->pwc[k][e]) || !std::isfinite(s.pow->a_tile[e])) die("block powers");
        {
            using namespace tde::multiband;
            long double z[kWords] = {};
            z[6] = 1.0L;   // (s1 of the first H1: reaches the five biquads behind it)
            for (uint32_t j = 0; j < kMbRun; ++j) frame(&s.co[0][0], z, 0.0L);
            for (int b = 0; b < kBlocks; ++b) {
                if (kBlockCol[b] != 3) continue;
                const int r = 2 * kBlockRow[b];
                if (std::fabs(s.pow->pw[0][4 * b] - (double)z[r]) > 1e-12 || std::fabs(s.pow->pw[0][4 * b + 2] - (double)z[r + 1]) > 1e-12) die("A^8 against the cascade");
            }
            if (z[0] != 0.0L || z[5] != 0.0L) die("the low chain hears nothing of the high one");
        }
        touch_terms(s.ins, s.k, s.frames, "a multiband vertex takes terms of kinds 0 .. 4 only");
        const size_t fb = (size_t)((s.frames + 1u) & ~1u);
        touch_w(s.out, fb * sizeof(float2));
        touch_w(s.line, (size_t)kMbState * sizeof(double));
        // x and the three dy: there in both forms, apart from each other and from out
        const uintptr_t buf[5] = {(uintptr_t)s.x, (uintptr_t)s.dy[0], (uintptr_t)s.dy[1], (uintptr_t)s.dy[2], (uintptr_t)s.out};
        for (int p = 0; p < 5; ++p) {
            if (buf[p] & 15u) die("buffer alignment");
            if (p < 4) touch_w((void*)buf[p], fb * 8);
            for (int q = p + 1; q < 5; ++q)
                if (buf[p] < buf[q] + fb * 8 && buf[q] < buf[p] + fb * 8) die("buffers overlap");
        }
        if (!multi) {
            if (s.agg || s.carry || s.agg1[0] || s.agg1[1] || s.agg1[2] || s.carry2[0] || s.carry2[1] || s.carry2[2]) die("tile words in the one-launch form");
        } else {
            if (!s.agg || !s.carry) die("null tile words in the seven-launch form");
            std::vector<std::pair<uintptr_t, size_t>> r = {{(uintptr_t)s.agg, (size_t)s.n_tiles * 2 * kMbWords * 8}, {(uintptr_t)s.carry, (size_t)s.n_tiles * 2 * kMbWords * 8}};
            for (int b = 0; b < 3; ++b) {
                if (!s.agg1[b] || !s.carry2[b]) die("null band tile words");
                r.push_back({(uintptr_t)s.agg1[b], (size_t)s.n_tiles * 8});
                r.push_back({(uintptr_t)s.carry2[b], (size_t)s.n_tiles * 8});
            }
            for (size_t p = 0; p < r.size(); ++p) {
                if (r[p].first & 15u) die("tile words' alignment");
                touch_w((void*)r[p].first, r[p].second);
                for (size_t q = p + 1; q < r.size(); ++q)
                    if (r[p].first < r[q].first + r[q].second && r[q].first < r[p].first + r[p].second) die("tile words overlap");
            }
            // the order of a vertex' launches, with the descriptor the first one saw
            if (which == LOCAL) {
                if (g_by_agg.count(s.agg) && g_by_agg[s.agg].phase != 0) die("a vertex' tile words reused before its launches finished");
                Track t{CARRY, 0, s, {nullptr, nullptr, nullptr}};
                g_by_agg[s.agg] = t;
                for (int b = 0; b < 3; ++b) g_band[s.agg1[b]] = {s.agg, b};
            } else {
                auto it = g_by_agg.find(s.agg);
                if (it == g_by_agg.end() || it->second.phase != which) die("launch order");
                if (memcmp(&it->second.first, &s, sizeof s) != 0) die("descriptor changed between launches");
                it->second.phase = which == APPLY ? 0 : which + 1;
            }
        }
        if (which == LOCAL) g_fx_launches[0] += 1;
        if (which != APPLY) continue;
        // ---- k_mb_apply: the line's books
        g_fx_launches[2] += 1;
        g_fx_vertices += 1;
        if (single) g_fx_single += 1;
        if (s.frames < kMbTile) g_fx_short += 1;
        (s.init ? g_fx_carried : g_fx_fresh) += 1;
        if (g_fx_after_set_time) {
            if (s.init) die("a vertex entered with its line after a set_time");
            g_fx_restarts += 1;
        }
        if (s.init) {
            if (!g_line_ran[s.line]) die("a vertex enters with a line nothing has written");
            g_fx_entry_log.push_back(s.line[kMbState - 1u]);
        }
        g_line_ran[s.line] = true;
        g_fx_stamp += 1.0;
        for (uint32_t m = 0; m < kMbState; ++m) s.line[m] = g_fx_stamp;
    }
}
void launch_mb_local(const MbDesc* d, int n, uint32_t n_tiles, hipStream_t) { check(d, n, n_tiles, false, LOCAL); }
void launch_mb_carry(const MbDesc* d, int n, hipStream_t) { check(d, n, 0u, false, CARRY); }
void launch_mb_detect(const MbDesc* d, int n, uint32_t n_tiles, hipStream_t) { check(d, n, n_tiles, false, DETECT); }
void launch_mb_apply(const MbDesc* d, int n, uint32_t n_tiles, bool single, hipStream_t) { check(d, n, n_tiles, single, APPLY); }
// (the engine's only use of these two launches in a build without the compressor's mocks: a multiband vertex' band detectors)
void launch_master_carry(const MasterDesc* d, int n, hipStream_t) {
    touch(d, (size_t)std::max(n, 0) * sizeof(MasterDesc));
    if (n <= 0 || n % 3) die("a carry launch holds three descriptors per vertex");
    for (int i = 0; i < n; ++i) {
        const MasterDesc& s = d[i];
        if (!s.agg || !s.carry || !s.n_tiles || s.op > 1u) die("carry descriptor");
        if ((size_t)s.chunk * kThreads < s.n_tiles || (s.chunk > 1 && (size_t)(s.chunk - 1) * kThreads >= s.n_tiles)) die("carry lane chunks");
        int b = 0;
        Track& t = band_of(s.agg, s.op ? CARRY2 : CARRY1, &b, "launch order (scalar carry)");
        const MbDesc& f = t.first;
        if (b != i % 3) die("the bands' order in a carry launch");
        if (s.n_tiles != f.n_tiles || s.chunk != f.chunk) die("carry tiling");
        if (s.op && s.carry != f.carry2[b]) die("the yL carry's slot");
        const double a = s.op ? f.aA : f.aR;
        if ((s.init == nullptr) != (f.init == nullptr) || (s.init && s.init != f.line + 2u * kMbWords + 2u * b + s.op)) die("carry entry value");
        if (std::fabs(s.a_tile - std::pow(a, (double)kMbTile)) > 1e-12) die("carry a_tile");
        for (int k = 0; k < 8; ++k)
            if (std::fabs(s.pwc[k] - std::pow(a, (double)kMbTile * (double)s.chunk * (double)(1u << k))) > 1e-12) die("carry powers");
        touch(s.agg, (size_t)s.n_tiles * 8);
        touch_w(s.carry, (size_t)s.n_tiles * 8);
        if (s.init) touch(s.init, 8);
        advance(t, s.op ? APPLY : ENV);
    }
}
void launch_comp_env(const CompDesc* d, int n, uint32_t n_tiles, hipStream_t) {
    touch(d, (size_t)std::max(n, 0) * sizeof(CompDesc));
    if (n <= 0 || n % 3) die("the env launch holds three descriptors per vertex");
    for (int i = 0; i < n; ++i) {
        const CompDesc& s = d[i];
        if (!s.dy || !s.state || !s.agg1 || !s.carry1 || !s.agg2 || !s.carry2) die("null pointer in a band's CompDesc");
        int b = 0;
        Track& t = band_of(s.agg1, ENV, &b, "launch order (env)");
        const MbDesc& f = t.first;
        if (b != i % 3) die("the bands' order in the env launch");
        if (s.frames != f.frames || s.n_tiles != f.n_tiles || s.n_tiles != n_tiles) die("env tiling");
        if (s.dy != f.dy[b] || s.agg1 != f.agg1[b] || s.carry2 != f.carry2[b]) die("a band's buffers");
        if ((const double*)s.state != f.line + 2u * kMbWords + 2u * b) die("a band's state: its (y1, yL) pair inside the line");
        if (s.aR != f.aR || s.aA != f.aA || s.oA != f.oA || memcmp(s.pwR, f.pwR, sizeof s.pwR) != 0 || memcmp(s.pwA, f.pwA, sizeof s.pwA) != 0) die("a band's constants");
        touch(s.carry1, (size_t)s.n_tiles * 8);
        touch_w(s.agg2, (size_t)s.n_tiles * 8);
        touch_w(&s.state->y1, 8);   // (k_comp_env stores y1 alone)
        t.agg2[b] = s.agg2;
        g_band[s.agg2] = {f.agg, b};
        g_fx_launches[1] += 1;
        advance(t, CARRY2);
    }
}
}  // namespace tdk

// ---- what tests/asan_fx.cpp needs to know about the kind: no debug.* options; the 4 096-frame chunks are two tiles
const FxHooks g_fx = {
    "multiband",
    [](td_state*, int, int) {},
    []() {
        if (g_fx_launches[1] == 3 * g_fx_launches[0] && g_fx_launches[2] >= g_fx_launches[0]) return true;   // (seven-launch vertices pass all steps)
        fprintf(stderr, "descriptor counts: k_mb_local %zu k_comp_env %zu k_mb_apply %zu\n", g_fx_launches[0], g_fx_launches[1], g_fx_launches[2]);
        return false;
    },
    []() {
        printf("k_mb_apply descriptors %zu (%zu vertices, %zu one-launch, %zu entered fresh, %zu entered with the line; %zu k_mb_local descriptors; "
               "%zu k_comp_env descriptors; %zu restarts checked; %zu short chunks)\n",
               g_fx_launches[2], g_fx_vertices, g_fx_single, g_fx_fresh, g_fx_carried, g_fx_launches[0], g_fx_launches[1], g_fx_restarts, g_fx_short);
    },
};
