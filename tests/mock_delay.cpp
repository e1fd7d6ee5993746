// The delay launches for the host-only sanitizer build of the engine (TEST INFRASTRUCTURE: linked only by
// tests/test_delay_host.py beside tests/mock_hip.cpp, never by the product).  Nothing is computed: every launch walks its
// descriptor table and both ends of every array a descriptor points to, so that a descriptor that points past an allocation is
// an AddressSanitizer report, and checks what the kernels rely on -- the tiling (lanes, tiles, the carry's threads per lane and
// tiles per thread), that the carry reads and writes the very tile words the vertex' descriptor named at k_delay_local, the line
// (16 D bytes, the rotation below D, no more words read than the vertex has written; none after a set_time), that every matrix
// power is within 2 ulp of a long-double recomputation done here, that the launches of a vertex come in order (local, carry,
// apply) and that a vertex takes k_delay_apply alone exactly when one tile covers its chunk.
// It also listens to the guard: the audit launches of mock_hip.cpp are wrapped at link time (-Wl,--wrap); the static gain the
// engine carried from a guarded launch to the graph's output is kept for the driver to print, and with g_delay_force_redo set
// every audited render is told to run again.  For that case k_delay_apply stamps the line words it rewrites and logs the stamp
// its lane 0 finds on entry: a render done again must find what the first one found, not what the first one left.
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <cmath>
#include <map>
#include <vector>

#include "kernels.h"

static volatile unsigned char g_delay_sink;
static void touch(const void* p, size_t bytes) {
    if (!p || !bytes) return;
    const volatile unsigned char* b = (const volatile unsigned char*)p;
    g_delay_sink ^= b[0];
    g_delay_sink ^= b[bytes - 1];
}
static void touch_w(void* p, size_t bytes) {
    if (!p || !bytes) return;
    volatile unsigned char* b = (volatile unsigned char*)p;
    b[0] = b[0];
    b[bytes - 1] = b[bytes - 1];
}
[[noreturn]] static void die(const char* what) {
    fprintf(stderr, "mock_delay: %s\n", what);
    abort();
}

size_t g_delay_launches[3] = {0, 0, 0}, g_delay_vertices = 0, g_delay_single = 0, g_delay_fresh = 0, g_delay_carried = 0;
double g_delay_path_gain = 0.0;   // the last guarded launch's static gain to the output (0: none since the driver cleared it)
int g_delay_force_redo = 0;       // every audited render is to be done again
int g_delay_after_set_time = 0;   // the driver has called td_graph_set_time and not submitted since: every vertex must enter with nothing of its line
size_t g_delay_restarts = 0;      // descriptors checked under that flag
std::vector<double> g_delay_entry_log;   // per k_delay_apply descriptor whose lane 0 enters with a written word: the stamp found there
static double g_delay_stamp = 0.0;

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
static void touch_delay_terms(const InTerm* ins, uint32_t k, uint32_t frames) {
    touch(ins, (size_t)k * sizeof(InTerm));
    for (uint32_t i = 0; i < k; ++i) {
        const InTerm& t = ins[i];
        if (t.kind == 0u || t.kind == 4u) touch(t.p, (size_t)frames * sizeof(float2));
        else if (t.kind == 3u) touch(t.p, ((size_t)t.len + 15) * 4);
        else if (t.kind == 1u || t.kind == 2u) touch(t.p, ((size_t)t.len + 15) * sizeof(float2));
        else die("a delay vertex takes terms of kinds 0 .. 4 only");
    }
}
static void check(const DelayDesc* d, int n, uint32_t max_groups, int which, bool single_launch = false) {
    touch(d, (size_t)std::max(n, 0) * sizeof(DelayDesc));
    g_delay_launches[which] += 1;
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
        touch_delay_terms(s.ins, s.k, s.frames);
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
            g_delay_vertices += 1;
            if (single) g_delay_single += 1;
            (s.filled ? g_delay_carried : g_delay_fresh) += 1;
            if (g_delay_after_set_time) {   // none of the line after a set_time: no word holds a value, the rotation starts over
                if (s.filled != 0u || s.pos != 0u) die("a vertex entered with its line after a set_time");
                g_delay_restarts += 1;
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
            if (s.pos < s.filled) g_delay_entry_log.push_back(s.line[2u * (size_t)s.pos]);
            // (the words of the chunk's last D frames are rewritten, as the kernel does)
            g_delay_stamp += 1.0;
            for (uint32_t m = 0; m < s.lanes; ++m) {
                const size_t w = 2u * (size_t)(((uint64_t)s.pos + m) % s.D);
                s.line[w] = g_delay_stamp;
                s.line[w + 1u] = g_delay_stamp;
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

// ---- the guard's launches, wrapped (ld --wrap: the engine's calls arrive here, __real_ is mock_hip.cpp's) ----
void real_band_audit(const AuditHead* h, int n, hipStream_t s) asm("__real__ZN3tdk17launch_band_auditEPKNS_9AuditHeadEiP12ihipStream_t");
void wrap_band_audit(const AuditHead* h, int n, hipStream_t s) asm("__wrap__ZN3tdk17launch_band_auditEPKNS_9AuditHeadEiP12ihipStream_t");
void wrap_band_audit(const AuditHead* h, int n, hipStream_t s) {
    for (int i = 0; i < n; ++i) {
        for (uint32_t j = 0; j < h[i].n; ++j) g_delay_path_gain = (double)h[i].descs[j].gain;
        if (g_delay_force_redo) h[i].host_word[0] = 1u;
    }
    real_band_audit(h, n, s);
}
void real_band_chain(const BandScanDesc* d, int n, uint32_t frames, uint32_t a, bool guarded, hipStream_t s)
    asm("__real__ZN3tdk17launch_band_chainEPKNS_12BandScanDescEijjbP12ihipStream_t");
void wrap_band_chain(const BandScanDesc* d, int n, uint32_t frames, uint32_t a, bool guarded, hipStream_t s)
    asm("__wrap__ZN3tdk17launch_band_chainEPKNS_12BandScanDescEijjbP12ihipStream_t");
void wrap_band_chain(const BandScanDesc* d, int n, uint32_t frames, uint32_t a, bool guarded, hipStream_t s) {
    // (a chain launch that gives its own verdict: nz_scale = gain^2 / frames)
    if (guarded)
        for (int i = 0; i < n; ++i)
            if (d[i].nz_scale > 0.0f) {
                g_delay_path_gain = std::sqrt((double)d[i].nz_scale * (double)frames);
                if (g_delay_force_redo && d[i].nz_host) d[i].nz_host[0] = 1u;
            }
    real_band_chain(d, n, frames, a, guarded, s);
}
}  // namespace tdk
