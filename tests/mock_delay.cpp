// The delay launches for the host-only sanitizer build of the engine (TEST INFRASTRUCTURE: linked only by
// tests/test_delay_host.py beside tests/mock_hip.cpp, never by the product).  Nothing is computed: every launch walks its
// descriptor table and both ends of every array a descriptor points to, so that a descriptor that points past an allocation is
// an AddressSanitizer report, and checks what the kernels rely on -- the tiling (lanes, tiles, the carry's threads per lane and
// tiles per thread), that the carry reads and writes the very tile words the vertex' descriptor named at k_delay_local, the line
// (16 D bytes, the rotation below D, no more words read than the vertex has written; none after a set_time), that every matrix
// power is within 2 ulp of a long-double recomputation done here, that the launches of a vertex come in order (local, carry,
// apply) and that a vertex takes k_delay_apply alone exactly when one tile covers its chunk.
// With g_fx_force_redo set the guard's listeners (tests/mock_guard.cpp) tell every audited render to run again.  For that case
// k_delay_apply stamps the line words it rewrites and logs the stamp
// its lane 0 finds on entry: a render done again must find what the first one found, not what the first one left.
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <cmath>
#include <map>
#include <vector>

#define MOCK_NAME "mock_delay"
#include "mock_util.h"
#include "asan_fx.h"
#include "termdaw_amd.h"

size_t g_fx_launches[3] = {0, 0, 0}, g_fx_vertices = 0, g_fx_single = 0, g_fx_fresh = 0, g_fx_carried = 0;
int g_fx_after_set_time = 0;   // the driver has called td_graph_set_time and not submitted since: every vertex must enter with nothing of its line
size_t g_fx_restarts = 0;      // descriptors checked under that flag
std::vector<double> g_fx_entry_log;   // per k_delay_apply descriptor whose lane 0 enters with a written word: the stamp found there
size_t g_fx_short = 0;         // (none counted: the delay has no short-chunk form)
static double g_fx_stamp = 0.0;

namespace {
struct Track { int phase; const double* carry; const double* line; uint32_t n_tiles, lanes, pos, filled; };
std::map<const double*, Track> g_by_agg;   // a vertex of the submission under way, by its tile words

struct M2 { long double m[4]; };
M2 mul(const M2& x, const M2& y) {
    M2 r;
    r.m[0] = x.m[0] * y.m[0] + x.m[1] * y.m[2];
    r.m[1] = x.m[0] * y.m[1] + x.m[1] * y.m[3];
    r.m[2] = x.m[2] * y.m[0] + x.m[3] * y.m[2];
    r.m[3] = x.m[2] * y.m[1] + x.m[3] * y.m[3];
    return r;
}
M2 power(M2 x, uint64_t e) {
    M2 r{{1.0L, 0.0L, 0.0L, 1.0L}};
    while (e) {
        if (e & 1u) r = mul(r, x);
        e >>= 1;
        if (e) x = mul(x, x);
    }
    return r;
}
void near(const double (&got)[4], const M2& want, const char* what) {
    for (int i = 0; i < 4; ++i) {
        const double w = (double)want.m[i];
        const double ulp = std::fabs(std::nextafter(std::fabs(w), INFINITY) - std::fabs(w));
        if (!(std::fabs(got[i] - w) <= 2.0 * ulp)) die(what);
    }
}
}  // namespace

namespace tdk {
static void check(const DelayDesc* d, int n, uint32_t max_groups, int which, bool single_launch = false) {
    touch(d, (size_t)std::max(n, 0) * sizeof(DelayDesc));
    g_fx_launches[which] += 1;
    if (n <= 0 || !max_groups) die("an empty launch");
    for (int i = 0; i < n; ++i) {
        const DelayDesc& s = d[i];
        if (!s.ins || !s.out || !s.line) die("null pointer in a DelayDesc");
        if (s.T != 8u && s.T != 16u && s.T != 32u && s.T != 64u) die("steps per tile");
        if (!s.frames || !s.D) die("frames / D");
        const uint64_t steps = ((uint64_t)s.frames + s.D - 1) / s.D;
        if (s.lanes != std::min(s.D, s.frames) || s.n_tiles != (steps + s.T - 1) / s.T) die("tiling");
        if ((uint64_t)s.frames + (uint64_t)(s.T + 4u) * s.D > 0xFFFF0000ull) die("frame indices leave 32 bits");
        const bool single = steps <= s.T;
        if (single != (s.n_tiles == 1u)) die("single-launch form");
        if (single && which != 2) die("a vertex one tile covers in k_delay_local / k_delay_carry");
        if (which == 2 && single != single_launch) die("k_delay_apply: a vertex in the other instantiation's launch");
        const uint64_t threads = (uint64_t)s.n_tiles * s.lanes;
        if (which != 1 && (threads + kThreads - 1) / kThreads > max_groups) die("grid too small");
        if (s.pos >= s.D || s.filled > s.D) die("line rotation / fill");
        if (!(s.wet >= 0.0001f && s.wet <= 1.0f)) die("wet");
        if (!(s.gs >= 0.0 && s.gc >= 0.0 && s.gs + s.gc <= 0.98 + 1e-7)) die("feedback");
        if ((((uintptr_t)s.out) | ((uintptr_t)s.line)) & 15u) die("alignment");
        touch_terms(s.ins, s.k, s.frames, "a delay vertex takes terms of kinds 0 .. 4 only");
        touch_w(s.out, (size_t)s.frames * sizeof(float2));
        touch_w(s.line, (size_t)s.D * 16);
        if (!single) {
            if (!s.x || !s.agg || !s.carry) die("null pointer in a DelayDesc");
            if ((const void*)s.x == (const void*)s.out || s.agg == s.carry) die("buffers alias");
            if ((((uintptr_t)s.x) | ((uintptr_t)s.agg) | ((uintptr_t)s.carry)) & 15u) die("alignment");
            if (!s.seg || (s.seg & (s.seg - 1u)) || s.seg > (uint32_t)kThreads) die("carry threads per lane");
            // (the fewest threads per lane that leave a thread at most 16 tiles, 256 at the most)
            if (s.chunk != (s.n_tiles + s.seg - 1u) / s.seg || (s.seg < 256u && s.seg * 16u < s.n_tiles) || (s.seg > 1u && (s.seg / 2u) * 16u >= s.n_tiles))
                die("carry chunks");
            if (which == 1 && ((uint64_t)s.lanes + kThreads / s.seg - 1) / (kThreads / s.seg) > max_groups) die("carry grid too small");
            touch_w(s.x, (size_t)s.frames * sizeof(float2));
            touch_w(s.agg, (size_t)threads * 16);
            touch_w(s.carry, (size_t)threads * 16);
        }
        if (which == 0 || (which == 2 && single)) {
            // the matrices: G = [[gs, gc], [gc, gs]] squared in long double, each power rounded once
            M2 p = power(M2{{(long double)s.gs, (long double)s.gc, (long double)s.gc, (long double)s.gs}}, s.T);
            near(s.g_tile, p, "tile power");
            p = power(p, s.chunk);
            for (int k = 0; k < 8; ++k) {
                near(s.pwc[k], p, "carry powers");
                p = mul(p, p);
            }
            g_fx_vertices += 1;
            if (single) g_fx_single += 1;
            (s.filled ? g_fx_carried : g_fx_fresh) += 1;
            if (g_fx_after_set_time) {   // none of the line after a set_time: no word holds a value, the rotation starts over
                if (s.filled != 0u || s.pos != 0u) die("a vertex entered with its line after a set_time");
                g_fx_restarts += 1;
            }
        }
        if (which == 0) {
            if (g_by_agg.count(s.agg) && g_by_agg[s.agg].phase != 0) die("a vertex' tile words reused before its launches finished");
            g_by_agg[s.agg] = Track{1, s.carry, s.line, s.n_tiles, s.lanes, s.pos, s.filled};
        } else if (!single) {
            auto it = g_by_agg.find(s.agg);
            if (it == g_by_agg.end() || it->second.phase != which) die("launch order (local, carry, apply)");
            const Track& t = it->second;
            if (t.carry != s.carry || t.line != s.line || t.n_tiles != s.n_tiles || t.lanes != s.lanes || t.pos != s.pos || t.filled != s.filled)
                die("descriptor changed between launches");
            it->second.phase = which == 1 ? 2 : 0;
        }
        if (which == 2) {
            if (s.pos < s.filled) g_fx_entry_log.push_back(s.line[2u * (size_t)s.pos]);
            // (the words of the chunk's last D frames are rewritten, as the kernel does)
            g_fx_stamp += 1.0;
            for (uint32_t m = 0; m < s.lanes; ++m) {
                const size_t w = 2u * (size_t)(((uint64_t)s.pos + m) % s.D);
                s.line[w] = g_fx_stamp;
                s.line[w + 1u] = g_fx_stamp;
            }
        }
    }
}
void launch_delay_local(const DelayDesc* d, int n, uint32_t max_groups, hipStream_t) { check(d, n, max_groups, 0); }
void launch_delay_carry(const DelayDesc* d, int n, uint32_t max_groups, hipStream_t) { check(d, n, max_groups, 1); }
void launch_delay_apply(const DelayDesc* d, int n, uint32_t max_groups, bool single, hipStream_t) {
    if (max_groups & kDelaySingleBit) die("the instantiation bit reached the launch");
    check(d, n, max_groups, 2, single);
}
}  // namespace tdk

// ---- what tests/asan_fx.cpp needs to know about the kind: 16 and (chunked, odd modes) 8 steps per tile
const FxHooks g_fx = {
    "delay",
    [](td_state* s, int mode, int chunked) {
        if (chunked && (mode & 1)) td_state_set_option(s, "debug.delay_tile", 8);
    },
    []() {
        if (g_fx_launches[1] == g_fx_launches[0] && g_fx_launches[2] >= g_fx_launches[0]) return true;
        fprintf(stderr, "launch counts: local %zu carry %zu apply %zu\n", g_fx_launches[0], g_fx_launches[1], g_fx_launches[2]);
        return false;
    },
    []() {
        printf("k_delay_apply launches %zu (%zu vertices, %zu single-launch, %zu entered fresh, %zu entered with the line; %zu k_delay_local launches; "
               "%zu restarts checked)\n",
               g_fx_launches[2], g_fx_vertices, g_fx_single, g_fx_fresh, g_fx_carried, g_fx_launches[0], g_fx_restarts);
    },
};
