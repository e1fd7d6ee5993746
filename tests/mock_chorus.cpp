// The chorus launches for the host-only sanitizer build of the engine (TEST INFRASTRUCTURE: linked only by
// tests/test_chorus_host.py beside tests/mock_hip.cpp, never by the product).  Nothing is computed: every launch walks its
// descriptor table and both ends of every array a descriptor points to, so that a descriptor that points past an allocation is
// an AddressSanitizer report, and checks what the kernels rely on -- the tiling (F, n_tiles, the LDS the launch would ask for),
// the constants (D0, A, f in their ranges, D0 - A >= 2, H a multiple of 64 that holds floor(D0 + A) + 3, the slope bound), the
// absolute time, the line (2 H frames, `filled` <= H and equal to the frames the vertex has run since it restarted, the half a
// launch reads being the half a launch before it wrote; nothing after a set_time), chunks shorter than the line, and that
// k_chorus_sum comes first exactly when the chunk is longer than kSatInlineFrames.
// It also listens to the guard: the audit launches of mock_hip.cpp are wrapped at link time (-Wl,--wrap); the static gain the
// engine carried from a guarded launch to the graph's output is kept for the driver to print, and with g_cho_force_redo set
// every audited render is told to run again.  For that case k_chorus stamps the half of the line it writes and logs the stamp it
// finds in the half it reads: a render done again must find what the first one found, not what the first one left.
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <cmath>
#include <map>
#include <vector>

#include "kernels.h"

static volatile unsigned char g_cho_sink;
static void touch(const void* p, size_t bytes) {
    if (!p || !bytes) return;
    const volatile unsigned char* b = (const volatile unsigned char*)p;
    g_cho_sink ^= b[0];
    g_cho_sink ^= b[bytes - 1];
}
static void touch_w(void* p, size_t bytes) {
    if (!p || !bytes) return;
    volatile unsigned char* b = (volatile unsigned char*)p;
    b[0] = b[0];
    b[bytes - 1] = b[bytes - 1];
}
[[noreturn]] static void die(const char* what) {
    fprintf(stderr, "mock_chorus: %s\n", what);
    abort();
}

size_t g_cho_launches[2] = {0, 0}, g_cho_vertices = 0, g_cho_single = 0, g_cho_fresh = 0, g_cho_carried = 0;
double g_cho_path_gain = 0.0;   // the last guarded launch's static gain to the output (0: none since the driver cleared it)
int g_cho_force_redo = 0;       // every audited render is to be done again
int g_cho_after_set_time = 0;   // the driver has called td_graph_set_time and not submitted since: every vertex must enter with nothing of its line
size_t g_cho_restarts = 0;      // descriptors checked under that flag
size_t g_cho_short = 0;         // descriptors whose chunk was shorter than the line
std::vector<double> g_cho_entry_log;   // per k_chorus descriptor that enters with the line: the stamp found in the half it reads
static float g_cho_stamp = 0.0f;

namespace {
struct LineBook { uint64_t total; uint32_t written; };   // frames since the restart; the half the last launch wrote
// per line: the states it has been in since it restarted, oldest first.  A launch must enter with one of them: the latest, or --
// a guarded render done again, whose line and books the guard has put back -- an earlier one, which then becomes the latest.
std::map<const float2*, std::vector<LineBook>> g_lines;
std::map<const float2*, uint32_t> g_summed;   // x buffers k_chorus_sum has filled and k_chorus has not read yet -> frames
}  // namespace

namespace tdk {
static void touch_chorus_terms(const InTerm* ins, uint32_t k, uint32_t frames) {
    touch(ins, (size_t)k * sizeof(InTerm));
    for (uint32_t i = 0; i < k; ++i) {
        const InTerm& t = ins[i];
        if (t.kind == 0u || t.kind == 4u) touch(t.p, (size_t)frames * sizeof(float2));
        else if (t.kind == 3u) touch(t.p, ((size_t)t.len + 15) * 4);
        else if (t.kind == 1u || t.kind == 2u) touch(t.p, ((size_t)t.len + 15) * sizeof(float2));
        else die("a chorus vertex takes terms of kinds 0 .. 4 only");
    }
}
// which: 0 k_chorus_sum, 1 k_chorus
static void check(const ChorusDesc* d, int n, int which, uint32_t n_tiles, bool terms, uint32_t frames) {
    touch(d, (size_t)std::max(n, 0) * sizeof(ChorusDesc));
    g_cho_launches[which] += 1;
    if (n <= 0) die("an empty launch");
    for (int i = 0; i < n; ++i) {
        const ChorusDesc& s = d[i];
        if (!s.ins || !s.out || !s.line) die("null pointer in a ChorusDesc");
        if (!s.frames || s.frames != frames) die("frames");
        if ((((uintptr_t)s.out) & 15u) || (((uintptr_t)s.line) & 7u)) die("alignment");
        if (!(s.wet >= 0.0001f && s.wet <= 1.0f)) die("wet");
        if (s.shape > 1u || s.voices < 1u || s.voices > 4u || s.inv_v != 1.0 / (double)s.voices) die("shape / voices");
        // 48 kHz: 0.5 .. 50 ms
        if (!(s.D0 >= 24.0 && s.D0 <= 2400.0) || !(s.A >= 0.0 && s.D0 - s.A >= 2.0 && s.D0 + s.A <= 2400.0 + 1e-9)) die("delay / depth");
        if (!(s.f >= 0.01 / 48000.0 * 0.999 && s.f <= 20.0 / 48000.0 * 1.001) || !(s.stereo >= 0.0 && s.stereo <= 0.5)) die("rate / stereo");
        if (!((s.shape == 0u ? 6.283185307179586 : 4.0) * s.A * s.f <= 0.5 + 1e-12)) die("the delay slope");
        if (s.H % 64u || (double)s.H < std::floor(s.D0 + s.A) + 3.0 || s.H > 2432u) die("H");
        if (s.F != 256u && s.F != 512u && s.F != 1024u) die("frames per tile");
        if (s.n_tiles != (s.frames + s.F - 1u) / s.F || s.n_tiles >= (1u << 20)) die("tiling");
        if (s.filled > s.H || s.parity > 1u) die("line fill / parity");
        if (s.t0 > (1ull << 40)) die("the absolute time");
        touch_chorus_terms(s.ins, s.k, s.frames);
        touch_w(s.out, (size_t)s.frames * sizeof(float2));
        touch_w(s.line, (size_t)2 * s.H * sizeof(float2));
        const bool multi = s.frames > kSatInlineFrames;
        if (multi != (s.x != nullptr)) die("scratch buffer against the form");
        if (multi) {
            if ((const void*)s.x == (const void*)s.out || (((uintptr_t)s.x) & 15u)) die("scratch buffer");
            touch_w(s.x, (size_t)s.frames * sizeof(float2));
        }
        if (which == 0) {
            if (!multi) die("k_chorus_sum in front of a chunk the one-launch form takes");
            if (g_summed.count(s.x)) die("a scratch buffer summed twice before k_chorus read it");
            g_summed[s.x] = s.frames;
            continue;
        }
        // ---- k_chorus
        if (s.n_tiles != n_tiles) die("the launch's tiling is not the descriptor's");
        if (terms == multi) die("k_chorus: a vertex in the other instantiation's launch");
        if (terms && (size_t)((frames + 1u) & ~1u) * sizeof(float2) > 32768u) die("LDS above 32 KB");
        if (multi) {
            auto it = g_summed.find(s.x);
            if (it == g_summed.end() || it->second != s.frames) die("k_chorus streams a buffer k_chorus_sum has not filled");
            g_summed.erase(it);
        }
        // the line's books: filled = min(frames since the restart, H), the half read is the half the last launch wrote
        g_cho_vertices += 1;
        if (terms) g_cho_single += 1;
        if (s.frames < s.H) g_cho_short += 1;
        (s.filled ? g_cho_carried : g_cho_fresh) += 1;
        if (g_cho_after_set_time) {
            if (s.filled != 0u) die("a vertex entered with its line after a set_time");
            g_cho_restarts += 1;
        }
        std::vector<LineBook>& hist = g_lines[s.line];
        uint64_t total = 0;
        if (s.filled) {
            while (!hist.empty() && !(s.filled == std::min<uint64_t>(hist.back().total, s.H) && s.parity == hist.back().written)) hist.pop_back();
            if (hist.empty()) die("filled / parity: the vertex enters with no state its line has been in since it restarted");
            total = hist.back().total;
            g_cho_entry_log.push_back((double)s.line[(size_t)s.parity * s.H + s.H - 1u].x);
        } else {
            hist.clear();
        }
        hist.push_back(LineBook{total + s.frames, s.parity ^ 1u});
        g_cho_stamp += 1.0f;
        for (uint32_t m = 0; m < s.H; ++m) s.line[(size_t)(s.parity ^ 1u) * s.H + m] = make_float2(g_cho_stamp, g_cho_stamp);
    }
}
void launch_chorus_sum(const ChorusDesc* d, int n, uint32_t frames, hipStream_t) { check(d, n, 0, 0, false, frames); }
void launch_chorus(const ChorusDesc* d, int n, uint32_t n_tiles, uint32_t frames, bool terms, hipStream_t) { check(d, n, 1, n_tiles, terms, frames); }

// ---- the guard's launches, wrapped (ld --wrap: the engine's calls arrive here, __real_ is mock_hip.cpp's) ----
void real_band_audit(const AuditHead* h, int n, hipStream_t s) asm("__real__ZN3tdk17launch_band_auditEPKNS_9AuditHeadEiP12ihipStream_t");
void wrap_band_audit(const AuditHead* h, int n, hipStream_t s) asm("__wrap__ZN3tdk17launch_band_auditEPKNS_9AuditHeadEiP12ihipStream_t");
void wrap_band_audit(const AuditHead* h, int n, hipStream_t s) {
    for (int i = 0; i < n; ++i) {
        for (uint32_t j = 0; j < h[i].n; ++j) g_cho_path_gain = (double)h[i].descs[j].gain;
        if (g_cho_force_redo) h[i].host_word[0] = 1u;
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
                g_cho_path_gain = std::sqrt((double)d[i].nz_scale * (double)frames);
                if (g_cho_force_redo && d[i].nz_host) d[i].nz_host[0] = 1u;
            }
    real_band_chain(d, n, frames, a, guarded, s);
}
}  // namespace tdk
