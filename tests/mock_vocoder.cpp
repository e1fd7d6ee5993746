// The vocoder launches, keyed forms included, for the host-only sanitizer build of the engine (TEST INFRASTRUCTURE: linked only by
// tests/test_vocoder_host.py beside tests/mock_hip.cpp and tests/mock_guard.cpp, never by the product).  Nothing is computed: every
// launch walks its descriptor table and both ends of every array a descriptor points to -- the band table, the key term table and
// whatever the key terms point to among them -- so that a descriptor that points past an allocation is an AddressSanitizer
// report, and checks what the kernels rely on: the tiling (2 048-frame tiles, the carries' lane chunks), the band count against
// the launch's, the constants (a band-pass has b1 = 0 and b2 = -b0; c0, c1; a, 1 - a, g), the scratch ranges (x, kx, the four
// tile-word arrays: there exactly in the five-launch form, apart from each other), the line (7 doubles per band; entered --
// `init` -- exactly when the vertex has run since it restarted, never right after a set_time), that a vertex' five launches come
// in order with the descriptor the first one saw, that a chunk of one tile is k_voc_apply alone, and that the keyed descriptors go
// through the keyed entry points and no others do.
// With g_fx_force_redo set the guard's listeners (tests/mock_guard.cpp) tell every audited render to run again.  For that case
// k_voc_apply stamps the line and logs the stamp it finds on entry: a render done again must find what the first one found.
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <map>
#include <vector>

#define MOCK_NAME "mock_vocoder"
#include "mock_util.h"
#include "asan_fx.h"
#include "termdaw_amd.h"

size_t g_fx_launches[3] = {0, 0, 0}, g_fx_vertices = 0, g_fx_single = 0, g_fx_fresh = 0, g_fx_carried = 0;   // [0] k_voc_local, [1] k_voc_env, [2] k_voc_apply: descriptors
int g_fx_after_set_time = 0;
size_t g_fx_restarts = 0;
size_t g_fx_short = 0;         // (descriptors of one-tile chunks that carried a partial tile: frames < 2 048)
std::vector<double> g_fx_entry_log;
static double g_fx_stamp = 0.0;
static size_t g_keyed = 0, g_keyed_single = 0;

namespace {
struct Track { int phase; tdk::VocDesc first; };
std::map<const double*, Track> g_by_agg;      // five-launch vertices between k_voc_local and k_voc_apply
std::map<const double*, bool> g_line_ran;     // line -> it has been written since it restarted
struct Summary { ~Summary() { printf("mock_vocoder: %zu keyed descriptors, %zu of them in the one-launch form\n", g_keyed, g_keyed_single); } } g_summary;
}  // namespace

namespace tdk {
// which: 0 k_voc_local, 1 k_voc_carry (mode 0), 2 k_voc_env, 3 k_voc_carry (mode 1), 4 k_voc_apply; keyed: the entry point (-1: either)
static void check(const VocDesc* d, int n, uint32_t bands, uint32_t n_tiles, int which, bool single, int keyed) {
    touch(d, (size_t)std::max(n, 0) * sizeof(VocDesc));
    if (n <= 0) die("an empty launch");
    if (bands != 4u && bands != 8u && bands != 16u) die("the launch's band count");
    const bool carry = which == 1 || which == 3;
    for (int i = 0; i < n; ++i) {
        const VocDesc& s = d[i];
        if (!s.ins || !s.out || !s.line || !s.band) die("null pointer in a VocDesc");
        if (s.bands != bands) die("a vertex in another band count's launch");
        if (!s.frames || s.n_tiles != (s.frames + kVocTile - 1) / kVocTile || (!carry && s.n_tiles != n_tiles)) die("tiling");
        if ((size_t)s.chunk * kThreads < s.n_tiles || (s.chunk > 1 && (size_t)(s.chunk - 1) * kThreads >= s.n_tiles)) die("carry lane chunks");
        const bool multi = s.n_tiles > 1u;
        if (single == multi) die("the form against the tile count");
        if (!multi && which != 4) die("a chunk of one tile is k_voc_apply alone");
        if (!(s.wet >= 0.0001f && s.wet <= 1.0f)) die("wet");
        if (!(s.a > 0.0 && s.a < 1.0) || s.oa != 1.0 - s.a || !(s.g > 0.06 && s.g < 252.0)) die("follower / gain");
        if (!(s.a_tile >= 0.0 && s.a_tile < 1.0) || !(s.pwa[0] > 0.0 && s.pwa[0] < 1.0)) die("follower powers");
        if ((((uintptr_t)s.out) & 15u) || (((uintptr_t)s.line) & 7u) || (((uintptr_t)s.band) & 7u)) die("alignment");
        if (s.init && s.init != s.line) die("entry state");
        touch(s.band, (size_t)s.bands * sizeof(VocBand));
        for (uint32_t b = 0; b < s.bands; ++b) {
            const VocBand& y = s.band[b];
            if (!(y.b0 > 0.0 && y.b0 < 1.0) || y.b1 != 0.0 || y.b2 != -y.b0) die("band-pass numerator");
            if (!(y.a2 > 0.0 && y.a2 < 1.0) || !(std::fabs(y.a1) < 1.0 + y.a2)) die("band-pass poles outside the unit circle");
            if (y.c0 != y.b1 - y.a1 * y.b0 || y.c1 != y.b2 - y.a2 * y.b0) die("c0 / c1");
            for (int k = 0; k < 8; ++k)
                for (int e = 0; e < 4; ++e)
                    if (!std::isfinite(y.pw[k][e]) || !std::isfinite(y.pwc[k][e])) die("matrix powers");
        }
        touch_terms(s.ins, s.k, s.frames, "a vocoder vertex takes terms of kinds 0 .. 4 only");
        // the key side
        const bool has = s.key_ins != nullptr;
        if (has != (s.key_k != 0u)) die("key term table and key count disagree");
        if (!has && s.key_term_mode != 0u) die("key term mode without key terms");
        if (keyed >= 0 && has != (keyed == 1)) die(keyed ? "an unkeyed descriptor in a keyed launch" : "a keyed descriptor in an unkeyed launch");
        if (has) {
            if ((const void*)s.key_ins == (const void*)s.ins) die("key terms alias the input terms");
            touch_terms(s.key_ins, s.key_k, s.frames, "a key term is of kinds 0 .. 4 only");
            for (uint32_t t = 0; t < s.key_k; ++t)
                if ((s.key_ins[t].kind == 0u || s.key_ins[t].kind == 4u) &&
                    ((const void*)s.key_ins[t].p == (const void*)s.x || (const void*)s.key_ins[t].p == (const void*)s.kx || (const void*)s.key_ins[t].p == (const void*)s.out))
                    die("a key term reads the vertex' own buffers");
        }
        touch_w(s.out, (size_t)((s.frames + 1u) & ~1u) * sizeof(float2));
        touch_w(s.line, (size_t)s.bands * kVocState * sizeof(double));
        if (!multi) {
            if (s.x || s.kx || s.agg || s.carry || s.agge || s.carrye) die("scratch in the one-launch form");
        } else {
            if (!s.x || !s.kx || !s.agg || !s.carry || !s.agge || !s.carrye) die("null scratch pointer in the five-launch form");
            if (has == ((const void*)s.kx == (const void*)s.x)) die("the key sum's buffer: its own exactly when the vertex is keyed");
            if ((const void*)s.x == (const void*)s.out || (const void*)s.kx == (const void*)s.out) die("buffers alias");
            if ((((uintptr_t)s.x) | ((uintptr_t)s.kx)) & 15u) die("scratch alignment");
            touch_w(s.x, (size_t)((s.frames + 1u) & ~1u) * sizeof(float2));
            touch_w(const_cast<float2*>(s.kx), (size_t)((s.frames + 1u) & ~1u) * sizeof(float2));
            const size_t tb = (size_t)s.n_tiles * s.bands * sizeof(double);
            const uintptr_t a[4] = {(uintptr_t)s.agg, (uintptr_t)s.carry, (uintptr_t)s.agge, (uintptr_t)s.carrye};
            const size_t b[4] = {6 * tb, 6 * tb, tb, tb};
            for (int p = 0; p < 4; ++p) {
                if (a[p] & 15u) die("tile words' alignment");
                touch_w((void*)a[p], b[p]);
                for (int q = p + 1; q < 4; ++q)
                    if (a[p] < a[q] + b[q] && a[q] < a[p] + b[p]) die("tile words overlap");
            }
        }
        // the order of a vertex' launches, with the descriptor the first one saw
        if (multi) {
            if (which == 0) {
                if (g_by_agg.count(s.agg) && g_by_agg[s.agg].phase != 0) die("a vertex' tile words reused before its launches finished");
                g_by_agg[s.agg] = Track{1, s};
            } else {
                auto it = g_by_agg.find(s.agg);
                if (it == g_by_agg.end() || it->second.phase != which) die("launch order");
                if (memcmp(&it->second.first, &s, sizeof s) != 0) die("descriptor changed between launches");
                it->second.phase = which == 4 ? 0 : which + 1;
            }
        }
        if (which == 0) g_fx_launches[0] += 1;
        if (which == 2) g_fx_launches[1] += 1;
        if (which != 4) continue;
        // ---- k_voc_apply: the line's books
        g_fx_launches[2] += 1;
        g_fx_vertices += 1;
        if (single) g_fx_single += 1;
        if (s.frames < kVocTile) g_fx_short += 1;
        if (has) { g_keyed += 1; g_keyed_single += single ? 1 : 0; }
        (s.init ? g_fx_carried : g_fx_fresh) += 1;
        if (g_fx_after_set_time) {
            if (s.init) die("a vertex entered with its line after a set_time");
            g_fx_restarts += 1;
        }
        if (s.init) {
            if (!g_line_ran[s.line]) die("a vertex enters with a line nothing has written");
            g_fx_entry_log.push_back(s.line[kVocState * s.bands - 1u]);
        }
        g_line_ran[s.line] = true;
        g_fx_stamp += 1.0;
        for (uint32_t m = 0; m < kVocState * s.bands; ++m) s.line[m] = g_fx_stamp;
    }
}
void launch_voc_local(const VocDesc* d, int n, uint32_t bands, uint32_t n_tiles, hipStream_t) { check(d, n, bands, n_tiles, 0, false, 0); }
void launch_voc_local_keyed(const VocDesc* d, int n, uint32_t bands, uint32_t n_tiles, hipStream_t) { check(d, n, bands, n_tiles, 0, false, 1); }
void launch_voc_carry(const VocDesc* d, int n, uint32_t bands, bool env, hipStream_t) { check(d, n, bands, 0u, env ? 3 : 1, false, -1); }
void launch_voc_env(const VocDesc* d, int n, uint32_t bands, uint32_t n_tiles, hipStream_t) { check(d, n, bands, n_tiles, 2, false, -1); }
void launch_voc_apply(const VocDesc* d, int n, uint32_t bands, uint32_t n_tiles, bool single, hipStream_t) { check(d, n, bands, n_tiles, 4, single, single ? 0 : -1); }
void launch_voc_apply_keyed(const VocDesc* d, int n, uint32_t bands, uint32_t n_tiles, hipStream_t) { check(d, n, bands, n_tiles, 4, true, 1); }
}  // namespace tdk

// ---- what tests/asan_fx.cpp needs to know about the kind: no debug.* options; the 4 096-frame chunks are two tiles
const FxHooks g_fx = {
    "vocoder",
    [](td_state*, int, int) {},
    []() {
        if (g_fx_launches[0] == g_fx_launches[1] && g_fx_launches[2] >= g_fx_launches[0]) return true;   // (five-launch vertices pass all steps)
        fprintf(stderr, "descriptor counts: k_voc_local %zu k_voc_env %zu k_voc_apply %zu\n", g_fx_launches[0], g_fx_launches[1], g_fx_launches[2]);
        return false;
    },
    []() {
        printf("k_voc_apply descriptors %zu (%zu vertices, %zu one-launch, %zu entered fresh, %zu entered with the line; %zu k_voc_local descriptors; "
               "%zu restarts checked; %zu short chunks)\n",
               g_fx_launches[2], g_fx_vertices, g_fx_single, g_fx_fresh, g_fx_carried, g_fx_launches[0], g_fx_restarts, g_fx_short);
    },
};
