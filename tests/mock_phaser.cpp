// The phaser launches for the host-only sanitizer build of the engine (TEST INFRASTRUCTURE: linked only by
// tests/test_phaser_host.py beside tests/mock_hip.cpp, never by the product).  Nothing is computed: every launch walks its
// descriptor table and both ends of every array a descriptor points to, so that a descriptor that points past an allocation is
// an AddressSanitizer report, and checks what the kernels rely on -- the tiling, the stage count a launch's template is chosen
// by, the scratch sizes of the maps and the carried states, that every launch of a vertex reads the very descriptor words the
// first one saw, and that the launches of a vertex come in order: local, carry, apply for a chunk of several tiles, apply alone
// (the single form, entered with the carried state) for a chunk of one.
// The driver is tests/asan_comp.cpp as it is: its counters keep the names it declares (g_comp_*), counting phaser launches
// here -- one per apply launch, on every step's counter, since a one-tile chunk has no other step.
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <cmath>
#include <map>

#define MOCK_NAME "mock_phaser"
#include "mock_util.h"

size_t g_comp_launches[5] = {0, 0, 0, 0, 0}, g_comp_vertices = 0, g_comp_fresh = 0, g_comp_carried = 0;

namespace {
struct Track { int phase; tdk::PhaserDesc first; };
std::map<const double*, Track> g_by_agg;   // a vertex of the submission under way, by its tile maps
}  // namespace

namespace tdk {
static void check(const PhaserDesc* d, int n, uint32_t stages, uint32_t n_tiles, bool single, int which) {
    touch(d, (size_t)std::max(n, 0) * sizeof(PhaserDesc));
    if (!(stages == 2u || stages == 4u || stages == 6u || stages == 8u)) die("a launch's stage count");
    if (which == 2) for (int i = 0; i < 5; ++i) g_comp_launches[i] += 1;
    for (int i = 0; i < n; ++i) {
        const PhaserDesc& s = d[i];
        const size_t D = (size_t)s.stages + 1;
        if (s.stages != stages) die("a vertex in the launch of another stage count");
        if (!s.ins || !s.out || !s.state) die("null pointer in a PhaserDesc");
        if (s.init && s.init != s.state) die("entry state");
        if (!s.frames || s.n_tiles != (s.frames + kPhaserTile - 1) / kPhaserTile) die("tiling");
        if (which != 1 && s.n_tiles != n_tiles) die("grid");
        if (single != (s.n_tiles == 1u) || (single && which != 2)) die("the one-launch form is for one tile, and k_phaser_apply's alone");
        if (single ? (s.x || s.agg || s.carry) : (!s.x || !s.agg || !s.carry)) die("scratch of the wrong form");
        if ((const void*)s.x == (const void*)s.out) die("buffers alias");
        if (!(s.wet >= 0.0001f && s.wet <= 1.0f)) die("wet");
        if (!(std::fabs(s.fb) <= 0.9500001) || !(s.f > 0.0 && s.f <= 20.0 / 8000.0) || !(s.stereo >= 0.0 && s.stereo <= 0.5) || s.shape > 1u) die("parameters");
        if (!(s.ad >= 0.0) || !(s.am - s.ad > -1.0) || !(s.am + s.ad < 1.0)) die("coefficient sweep");
        if ((((uintptr_t)s.x) | ((uintptr_t)s.out)) & 15u) die("alignment");
        if ((((uintptr_t)s.agg) | ((uintptr_t)s.carry) | ((uintptr_t)s.state)) & 7u) die("doubles' alignment");
        touch_terms(s.ins, s.k, s.frames, "a phaser vertex takes terms of kinds 0 .. 4 only");
        if (s.x) touch_w(s.x, (size_t)((s.frames + 1u) & ~1u) * sizeof(float2));   // (pairs: an odd chunk's last store covers one frame more)
        touch_w(s.out, (size_t)((s.frames + 1u) & ~1u) * sizeof(float2));
        touch_w(s.state, sizeof(PhaserState));
        const size_t ab = (size_t)s.n_tiles * 2 * D * (D + 1) * sizeof(double), cb = (size_t)s.n_tiles * 2 * D * sizeof(double);
        if (!single) {
            touch_w(s.agg, ab);
            touch_w(s.carry, cb);
            const uintptr_t a = (uintptr_t)s.agg, c = (uintptr_t)s.carry;
            if (a < c + cb && c < a + ab) die("tile words overlap");
        }
        if (which == 2) {
            g_comp_vertices += 1;
            (s.init ? g_comp_carried : g_comp_fresh) += 1;
        }
        if (single) continue;
        if (which == 0) {
            if (g_by_agg.count(s.agg) && g_by_agg[s.agg].phase != 0) die("a vertex' tile words reused before its launches finished");
            g_by_agg[s.agg] = Track{1, s};
        } else {
            auto it = g_by_agg.find(s.agg);
            if (it == g_by_agg.end() || it->second.phase != which) die("launch order");
            const PhaserDesc& f = it->second.first;
            if (f.carry != s.carry || f.x != s.x || f.out != s.out || f.state != s.state || f.init != s.init || f.t0 != s.t0 || f.frames != s.frames ||
                f.stages != s.stages)
                die("descriptor changed between launches");
            it->second.phase = which == 2 ? 0 : which + 1;
        }
    }
}
void launch_phaser_local(const PhaserDesc* d, int n, uint32_t stages, uint32_t n_tiles, hipStream_t) { check(d, n, stages, n_tiles, false, 0); }
void launch_phaser_carry(const PhaserDesc* d, int n, uint32_t stages, hipStream_t) { check(d, n, stages, 0u, false, 1); }
void launch_phaser_apply(const PhaserDesc* d, int n, uint32_t stages, uint32_t n_tiles, bool single, hipStream_t) { check(d, n, stages, n_tiles, single, 2); }
}  // namespace tdk
