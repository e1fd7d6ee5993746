// The EQ launches for the host-only sanitizer build of the engine (TEST INFRASTRUCTURE: linked only by tests/test_eq_host.py
// beside tests/mock_hip.cpp, never by the product).  Nothing is computed: every launch walks its descriptor table and both ends
// of every array a descriptor points to, so that a descriptor that points past an allocation is an AddressSanitizer report,
// and checks what the kernels rely on -- the tiling, the carry's lane chunks, that the carry reads and writes the very tile
// words the vertex' descriptor named at k_eq_local, the entry state (the vertex' own slot, or none after a set_time), that every
// matrix power is within 2 ulp of a long-double recomputation done here, and that the three launches of a vertex come in order
// (local, carry, apply).
// (The guard's listeners, which keep the static gain the engine carried from a guarded launch to the graph's output for the driver
// to print, are tests/mock_guard.cpp's.)
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <cmath>
#include <map>

#define MOCK_NAME "mock_eq"
#include "mock_util.h"

size_t g_eq_launches[3] = {0, 0, 0}, g_eq_vertices = 0, g_eq_fresh = 0, g_eq_carried = 0;

namespace {
struct Track { int phase; const double* carry; const tdk::EqState* state; const tdk::EqState* init; uint32_t n_tiles; };
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
static void check(const EqDesc* d, int n, uint32_t max_tiles, int which) {
    touch(d, (size_t)std::max(n, 0) * sizeof(EqDesc));
    g_eq_launches[which] += 1;
    for (int i = 0; i < n; ++i) {
        const EqDesc& s = d[i];
        if (!s.ins || !s.x || !s.out || !s.state || !s.agg || !s.carry) die("null pointer in an EqDesc");
        if (!s.frames || s.n_tiles != (s.frames + kEqTile - 1) / kEqTile || (which != 1 && s.n_tiles > max_tiles)) die("tiling");
        if ((size_t)s.chunk * kThreads < s.n_tiles || (s.chunk > 1 && (size_t)(s.chunk - 1) * kThreads >= s.n_tiles)) die("carry lane chunks");
        if ((const void*)s.x == (const void*)s.out || s.agg == s.carry) die("buffers alias");
        if (s.init && s.init != s.state) die("entry state");
        if (!(s.wet >= 0.0001f && s.wet <= 1.0f)) die("wet");
        if (!(std::fabs(s.a2) < 1.0 && std::fabs(s.a1) < 1.0 + s.a2)) die("an unstable filter");
        if (s.c0 != s.b1 - s.a1 * s.b0 || s.c1 != s.b2 - s.a2 * s.b0) die("c");
        if ((((uintptr_t)s.x) | ((uintptr_t)s.out) | ((uintptr_t)s.agg) | ((uintptr_t)s.carry) | ((uintptr_t)s.state)) & 15u) die("alignment");
        touch_terms(s.ins, s.k, s.frames, "an eq vertex takes terms of kinds 0 .. 4 only");
        touch_w(s.x, (size_t)s.frames * sizeof(float2));
        touch_w(s.out, (size_t)s.frames * sizeof(float2));
        touch_w(s.state, sizeof(EqState));
        touch_w(s.agg, (size_t)s.n_tiles * 32);
        touch_w(s.carry, (size_t)s.n_tiles * 32);
        if (which == 0) {
            // the matrices: A = [[-a1, 1], [-a2, 0]] squared in long double, each power rounded once
            M2 p = power(M2{{-(long double)s.a1, 1.0L, -(long double)s.a2, 0.0L}}, kEqRun);
            for (int k = 0; k < 8; ++k) {
                near(s.pw[k], p, "lane powers");
                p = mul(p, p);
            }
            near(s.a_tile, p, "tile power");
            p = power(p, s.chunk);
            for (int k = 0; k < 8; ++k) {
                near(s.pwc[k], p, "carry powers");
                p = mul(p, p);
            }
            if (g_by_agg.count(s.agg) && g_by_agg[s.agg].phase != 0) die("a vertex' tile words reused before its launches finished");
            g_by_agg[s.agg] = Track{1, s.carry, s.state, s.init, s.n_tiles};
            g_eq_vertices += 1;
            (s.init ? g_eq_carried : g_eq_fresh) += 1;
        } else {
            auto it = g_by_agg.find(s.agg);
            if (it == g_by_agg.end() || it->second.phase != which) die("launch order (local, carry, apply)");
            const Track& t = it->second;
            if (t.carry != s.carry || t.state != s.state || t.init != s.init || t.n_tiles != s.n_tiles) die("descriptor changed between launches");
            it->second.phase = which == 1 ? 2 : 0;
        }
    }
}
void launch_eq_local(const EqDesc* d, int n, uint32_t max_tiles, hipStream_t) { check(d, n, max_tiles, 0); }
void launch_eq_carry(const EqDesc* d, int n, hipStream_t) { check(d, n, 0u, 1); }
void launch_eq_apply(const EqDesc* d, int n, uint32_t max_tiles, hipStream_t) { check(d, n, max_tiles, 2); }
}  // namespace tdk
