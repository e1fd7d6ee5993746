// The saturator launches for the host-only sanitizer build of the engine (TEST INFRASTRUCTURE: linked only by
// tests/test_saturator_host.py beside tests/mock_hip.cpp, never by the product).  Nothing is computed: every launch walks its
// descriptor table and both ends of every array a descriptor points to, so that a descriptor that points past an allocation is
// an AddressSanitizer report, and checks what the kernels rely on -- the tiling (F, n_tiles, the LDS the launch would ask for),
// the taps (length by the launch's factor, symmetric, summing to 1), the constants (g_in, g_out and f(bias) in their ranges), the
// line (2 KB, `filled` <= 128 and equal to the frames the vertex has run since it restarted, the half a launch reads being the half
// a launch before it wrote; nothing after a set_time), chunks shorter than the line, that k_sat_sum comes first exactly when the
// chunk is longer than kSatInlineFrames, and that a launch holds vertices of one oversampling factor only.
// It also listens to the guard: the audit launches of mock_hip.cpp are wrapped at link time (-Wl,--wrap); the static gain the
// engine carried from a guarded launch to the graph's output is kept for the driver to print, and with g_sat_force_redo set
// every audited render is told to run again.  For that case k_sat stamps the half of the line it writes and logs the stamp it finds
// in the half it reads: a render done again must find what the first one found, not what the first one left.
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <cmath>
#include <map>
#include <vector>

#include "kernels.h"

static volatile unsigned char g_sat_sink;
static void touch(const void* p, size_t bytes) {
    if (!p || !bytes) return;
    const volatile unsigned char* b = (const volatile unsigned char*)p;
    g_sat_sink ^= b[0];
    g_sat_sink ^= b[bytes - 1];
}
static void touch_w(void* p, size_t bytes) {
    if (!p || !bytes) return;
    volatile unsigned char* b = (volatile unsigned char*)p;
    b[0] = b[0];
    b[bytes - 1] = b[bytes - 1];
}
[[noreturn]] static void die(const char* what) {
    fprintf(stderr, "mock_sat: %s\n", what);
    abort();
}

size_t g_sat_launches[3] = {0, 0, 0}, g_sat_vertices = 0, g_sat_single = 0, g_sat_fresh = 0, g_sat_carried = 0;
double g_sat_path_gain = 0.0;   // the last guarded launch's static gain to the output (0: none since the driver cleared it)
int g_sat_force_redo = 0;       // every audited render is to be done again
int g_sat_after_set_time = 0;   // the driver has called td_graph_set_time and not submitted since: every vertex must enter with nothing of its line
size_t g_sat_restarts = 0;      // descriptors checked under that flag
size_t g_sat_short = 0;         // descriptors whose chunk was shorter than the line
std::vector<double> g_sat_entry_log;   // per k_sat descriptor that enters with the line: the stamp found in the half it reads
static float g_sat_stamp = 0.0f;

namespace {
struct LineBook { uint64_t total; uint32_t written; };   // frames since the restart; the half the last launch wrote
// per line: the states it has been in since it restarted, oldest first.  A launch must enter with one of them: the latest, or --
// a guarded render done again, whose line and books the guard has put back -- an earlier one, which then becomes the latest.
std::map<const float2*, std::vector<LineBook>> g_lines;
std::map<const float2*, uint32_t> g_summed;   // x buffers k_sat_sum has filled and k_sat has not read yet -> frames
}  // namespace

namespace tdk {
static void touch_sat_terms(const InTerm* ins, uint32_t k, uint32_t frames) {
    touch(ins, (size_t)k * sizeof(InTerm));
    for (uint32_t i = 0; i < k; ++i) {
        const InTerm& t = ins[i];
        if (t.kind == 0u || t.kind == 4u) touch(t.p, (size_t)frames * sizeof(float2));
        else if (t.kind == 3u) touch(t.p, ((size_t)t.len + 15) * 4);
        else if (t.kind == 1u || t.kind == 2u) touch(t.p, ((size_t)t.len + 15) * sizeof(float2));
        else die("a saturator vertex takes terms of kinds 0 .. 4 only");
    }
}
// which: 0 k_sat_sum, 1 k_sat, 2 k_sat1
static void check(const SatDesc* d, int n, int which, uint32_t R, uint32_t n_tiles, uint32_t F, bool terms, uint32_t frames) {
    touch(d, (size_t)std::max(n, 0) * sizeof(SatDesc));
    g_sat_launches[which] += 1;
    if (n <= 0) die("an empty launch");
    for (int i = 0; i < n; ++i) {
        const SatDesc& s = d[i];
        if (!s.ins || !s.out) die("null pointer in a SatDesc");
        if (!s.frames || (which != 1 && s.frames != frames)) die("frames");
        if (((uintptr_t)s.out) & 15u) die("alignment");
        if (!(s.wet >= 0.0001f && s.wet <= 1.0f)) die("wet");
        if (s.kind > 2u) die("kind");
        // 10^(-24 / 20) .. 10^(48 / 20), 10^(-48 / 20) .. 10^(24 / 20), |f(bias)| <= 1
        if (!(s.g_in >= 0.0630 && s.g_in <= 251.19) || !(s.g_out >= 0.00398 && s.g_out <= 15.85)) die("gains");
        if (!(s.bias >= -1.0 && s.bias <= 1.0) || !(std::fabs(s.fb) <= 1.0)) die("bias");
        if ((s.kind == 0u && s.fb != s.bias) || (s.kind == 2u && s.fb != s.bias / (1.0 + std::fabs(s.bias)))) die("f(bias)");
        touch_sat_terms(s.ins, s.k, s.frames);
        touch_w(s.out, (size_t)s.frames * sizeof(float2));
        if (which == 2) {
            if (s.line || s.taps || s.x) die("k_sat1 has no line, no taps and no scratch buffer");
            g_sat_vertices += 1;
            continue;
        }
        if (!s.line || !s.taps) die("null pointer in a SatDesc");
        if (s.F != 128u && s.F != 256u && s.F != 384u) die("frames per tile");
        if (s.n_tiles != (s.frames + s.F - 1u) / s.F || s.n_tiles >= (1u << 20)) die("tiling");
        if (s.filled > 128u || s.parity > 1u) die("line fill / parity");
        if ((((uintptr_t)s.line) | ((uintptr_t)s.taps)) & 7u) die("alignment");
        touch_w(s.line, 2 * 128 * sizeof(float2));
        const bool multi = s.frames > kSatInlineFrames;
        if (multi != (s.x != nullptr)) die("scratch buffer against the form");
        if (multi) {
            if ((const void*)s.x == (const void*)s.out || (((uintptr_t)s.x) & 15u)) die("scratch buffer");
            touch_w(s.x, (size_t)s.frames * sizeof(float2));
        }
        if (which == 0) {
            if (!multi) die("k_sat_sum in front of a chunk the one-launch form takes");
            if (g_summed.count(s.x)) die("a scratch buffer summed twice before k_sat read it");
            g_summed[s.x] = s.frames;
            continue;
        }
        // ---- k_sat
        if (R != 2u && R != 4u && R != 8u) die("oversampling factor");
        if (s.F != F || s.n_tiles != n_tiles) die("the launch's tiling is not the descriptor's");
        if (terms == multi) die("k_sat: a vertex in the other instantiation's launch");
        if ((size_t)(F + 128u) * sizeof(float2) + (size_t)2 * R * (F + 64u) * sizeof(double) > 65536u) die("LDS above 64 KB");
        if (multi) {
            auto it = g_summed.find(s.x);
            if (it == g_summed.end() || it->second != s.frames) die("k_sat streams a buffer k_sat_sum has not filled");
            g_summed.erase(it);
        }
        // the taps: 2 Z R + 1 of them (the bytes behind them are the staging arena's: a wrong factor shows as asymmetry)
        const uint32_t L = 64u * R + 1u;
        touch(s.taps, (size_t)L * sizeof(double));
        double sum = 0.0;
        for (uint32_t k = 0; k < L; ++k) {
            if (!(std::fabs(s.taps[k] - s.taps[L - 1u - k]) <= 1e-16)) die("taps not symmetric over 2 Z R + 1");
            sum += s.taps[k];
        }
        if (!(std::fabs(sum - 1.0) <= 1e-14) || !(s.taps[L / 2u] > 0.7 / R && s.taps[L / 2u] < 0.9 / R)) die("taps");
        // the line's books: filled = min(frames since the restart, 128), the half read is the half the last launch wrote
        g_sat_vertices += 1;
        if (terms) g_sat_single += 1;
        if (s.frames < 128u) g_sat_short += 1;
        (s.filled ? g_sat_carried : g_sat_fresh) += 1;
        if (g_sat_after_set_time) {
            if (s.filled != 0u) die("a vertex entered with its line after a set_time");
            g_sat_restarts += 1;
        }
        std::vector<LineBook>& hist = g_lines[s.line];
        uint64_t total = 0;
        if (s.filled) {
            while (!hist.empty() && !(s.filled == std::min<uint64_t>(hist.back().total, 128u) && s.parity == hist.back().written)) hist.pop_back();
            if (hist.empty()) die("filled / parity: the vertex enters with no state its line has been in since it restarted");
            total = hist.back().total;
            g_sat_entry_log.push_back((double)s.line[s.parity * 128u + 127u].x);
        } else {
            hist.clear();
        }
        hist.push_back(LineBook{total + s.frames, s.parity ^ 1u});
        g_sat_stamp += 1.0f;
        for (uint32_t m = 0; m < 128u; ++m) s.line[(s.parity ^ 1u) * 128u + m] = make_float2(g_sat_stamp, g_sat_stamp);
    }
}
void launch_sat_sum(const SatDesc* d, int n, uint32_t frames, hipStream_t) { check(d, n, 0, 0, 0, 0, false, frames); }
void launch_sat(const SatDesc* d, int n, uint32_t R, uint32_t n_tiles, uint32_t F, bool terms, hipStream_t) { check(d, n, 1, R, n_tiles, F, terms, 0); }
void launch_sat1(const SatDesc* d, int n, uint32_t frames, hipStream_t) { check(d, n, 2, 1, 0, 0, false, frames); }

// ---- the guard's launches, wrapped (ld --wrap: the engine's calls arrive here, __real_ is mock_hip.cpp's) ----
void real_band_audit(const AuditHead* h, int n, hipStream_t s) asm("__real__ZN3tdk17launch_band_auditEPKNS_9AuditHeadEiP12ihipStream_t");
void wrap_band_audit(const AuditHead* h, int n, hipStream_t s) asm("__wrap__ZN3tdk17launch_band_auditEPKNS_9AuditHeadEiP12ihipStream_t");
void wrap_band_audit(const AuditHead* h, int n, hipStream_t s) {
    for (int i = 0; i < n; ++i) {
        for (uint32_t j = 0; j < h[i].n; ++j) g_sat_path_gain = (double)h[i].descs[j].gain;
        if (g_sat_force_redo) h[i].host_word[0] = 1u;
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
                g_sat_path_gain = std::sqrt((double)d[i].nz_scale * (double)frames);
                if (g_sat_force_redo && d[i].nz_host) d[i].nz_host[0] = 1u;
            }
    real_band_chain(d, n, frames, a, guarded, s);
}
}  // namespace tdk
