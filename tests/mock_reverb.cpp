// The reverb launches for the host-only sanitizer build of the engine (TEST INFRASTRUCTURE: linked only by
// tests/test_reverb_host.py beside tests/mock_hip.cpp, never by the product).  Nothing is computed: every launch walks its
// descriptor table and both ends of every array a descriptor points to, so that a descriptor that points past an allocation is
// an AddressSanitizer report, and checks what the kernels rely on -- the window length (64 | 128 | 256, no longer than the
// shortest line), the constants (g, d1, d2, w1, w2 in their ranges, the scan's powers the squares of one another), the lines (at
// least 64 frames each, back to back behind the 16 one-pole words, every slot index below its line's length), the books (`pos`,
// `skip` and `fresh` of all 24 lines the ones of ONE count of frames run since the restart, and that count the one the launch
// before left; nothing after a set_time), chunks shorter than the window, and that k_reverb_sum has filled the buffer k_reverb reads.
// It also listens to the guard: the audit launches of mock_hip.cpp are wrapped at link time (-Wl,--wrap); the static gain the
// engine carried from a guarded launch to the graph's output is kept for the driver to print, and with g_rev_force_redo set
// every audited render is told to run again.  For that case k_reverb stamps the state block's first word and logs the stamp it
// finds there on entry: a render done again must find what the first one found, not what the first one left.
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <cmath>
#include <map>
#include <vector>

#include "kernels.h"

static volatile unsigned char g_rev_sink;
static void touch(const void* p, size_t bytes) {
    if (!p || !bytes) return;
    const volatile unsigned char* b = (const volatile unsigned char*)p;
    g_rev_sink ^= b[0];
    g_rev_sink ^= b[bytes - 1];
}
static void touch_w(void* p, size_t bytes) {
    if (!p || !bytes) return;
    volatile unsigned char* b = (volatile unsigned char*)p;
    b[0] = b[0];
    b[bytes - 1] = b[bytes - 1];
}
[[noreturn]] static void die(const char* what) {
    fprintf(stderr, "mock_reverb: %s\n", what);
    abort();
}

size_t g_rev_launches[2] = {0, 0}, g_rev_vertices = 0, g_rev_serial = 0, g_rev_fresh = 0, g_rev_carried = 0;
double g_rev_path_gain = 0.0;   // the last guarded launch's static gain to the output (0: none since the driver cleared it)
int g_rev_force_redo = 0;       // every audited render is to be done again
int g_rev_after_set_time = 0;   // the driver has called td_graph_set_time and not submitted since: every vertex must enter with nothing of its state
size_t g_rev_restarts = 0;      // descriptors checked under that flag
size_t g_rev_short = 0;         // descriptors whose chunk was shorter than the window
std::vector<double> g_rev_entry_log;   // per k_reverb descriptor that enters with its state: the stamp found in the block's first word
static double g_rev_stamp = 0.0;

namespace {
// per state block: the counts of frames run since the restart it has stood at, oldest first.  A launch must enter with one of them:
// the latest, or -- a guarded render done again, whose block and books the guard has put back -- an earlier one, which then
// becomes the latest.
std::map<const double*, std::vector<uint64_t>> g_books;
std::map<const float2*, uint32_t> g_summed;   // x buffers k_reverb_sum has filled and k_reverb has not read yet -> frames
}  // namespace

namespace tdk {
static void touch_reverb_terms(const InTerm* ins, uint32_t k, uint32_t frames) {
    touch(ins, (size_t)k * sizeof(InTerm));
    for (uint32_t i = 0; i < k; ++i) {
        const InTerm& t = ins[i];
        if (t.kind == 0u || t.kind == 4u) touch(t.p, (size_t)frames * sizeof(float2));
        else if (t.kind == 3u) touch(t.p, ((size_t)t.len + 15) * 4);
        else if (t.kind == 1u || t.kind == 2u) touch(t.p, ((size_t)t.len + 15) * sizeof(float2));
        else die("a reverb vertex takes terms of kinds 0 .. 4 only");
    }
}
static bool books_match(const ReverbDesc& s, uint64_t total) {
    for (int i = 0; i < 24; ++i) {
        if (s.pos[i] != (uint32_t)(total % s.len[i])) return false;
        if (s.skip[i] != (total < s.len[i] ? (uint32_t)(s.len[i] - total) : 0u)) return false;
    }
    return true;
}
// which: 0 k_reverb_sum, 1 k_reverb
static void check(const ReverbDesc* d, int n, int which, uint32_t frames, uint32_t form) {
    touch(d, (size_t)std::max(n, 0) * sizeof(ReverbDesc));
    g_rev_launches[which] += 1;
    if (n <= 0) die("an empty launch");
    if (which == 1 && form > 1u) die("form");
    for (int i = 0; i < n; ++i) {
        const ReverbDesc& s = d[i];
        if (!s.ins || !s.out || !s.state || !s.x) die("null pointer in a ReverbDesc");
        if (!s.frames || (which == 0 && s.frames != frames)) die("frames");
        if ((((uintptr_t)s.out) & 15u) || (((uintptr_t)s.x) & 15u) || (((uintptr_t)s.state) & 7u) || (const void*)s.x == (const void*)s.out) die("alignment / scratch buffer");
        if (!(s.wet >= 0.0001f && s.wet <= 1.0f)) die("wet");
        if (!(s.g >= 0.7 && s.g <= 0.98 + 1e-12) || !(s.d1 >= 0.0 && s.d1 <= 0.4 + 1e-12) || s.d2 != 1.0 - s.d1) die("g / d1 / d2");
        if (!(s.w1 >= 0.5 && s.w1 <= 1.0) || !(s.w2 >= 0.0 && s.w2 <= 0.5) || std::fabs(s.w1 + s.w2 - 1.0) > 1e-15) die("w1 / w2");
        if (s.B != 64u && s.B != 128u && s.B != 256u) die("frames per window");
        uint32_t at = 16, shortest = 0xFFFFFFFFu;
        for (int l = 0; l < 24; ++l) {
            if (s.len[l] < 64u || s.len[l] > 8192u) die("a line's length");   // (48 kHz, size <= 2: 1640 x 2 x 48 / 44.1 = 3 570)
            if (s.off[l] != at) die("the lines do not lie back to back");
            if (s.pos[l] >= s.len[l] || s.skip[l] > s.len[l]) die("a slot index beyond its line");
            at += s.len[l];
            shortest = std::min(shortest, s.len[l]);
        }
        if (s.B > shortest) die("a window longer than the shortest line");
        if (s.len[0] < 2u * s.B) die("a comb line shorter than two windows");
        // the scan's powers: pw[0] = d1^(B / 64), each the square of the one before (to a rounding)
        if (std::fabs(s.pw[0] - std::pow(s.d1, (double)(s.B / 64u))) > 1e-15) die("pw[0]");
        for (int k = 1; k < 6; ++k)
            if (std::fabs(s.pw[k] - s.pw[k - 1] * s.pw[k - 1]) > 1e-14 * s.pw[k] + 1e-300) die("pw[k] is not the square of pw[k - 1]");
        touch_reverb_terms(s.ins, s.k, s.frames);
        touch_w(s.out, (size_t)s.frames * sizeof(float2));
        touch_w(s.x, (size_t)s.frames * sizeof(float2));
        touch_w(s.state, (size_t)at * sizeof(double));
        if (which == 0) {
            if (g_summed.count(s.x)) die("a scratch buffer summed twice before k_reverb read it");
            g_summed[s.x] = s.frames;
            continue;
        }
        // ---- k_reverb
        {
            auto it = g_summed.find(s.x);
            if (it == g_summed.end() || it->second != s.frames) die("k_reverb reads a buffer k_reverb_sum has not filled");
            g_summed.erase(it);
        }
        g_rev_vertices += 1;
        if (form == 0u) g_rev_serial += 1;
        if (s.frames < s.B) g_rev_short += 1;
        (s.fresh ? g_rev_fresh : g_rev_carried) += 1;
        if (g_rev_after_set_time) {
            if (!s.fresh) die("a vertex entered with its state after a set_time");
            g_rev_restarts += 1;
        }
        std::vector<uint64_t>& hist = g_books[s.state];
        uint64_t total = 0;
        if (!s.fresh) {
            while (!hist.empty() && !(hist.back() > 0 && books_match(s, hist.back()))) hist.pop_back();
            if (hist.empty()) die("pos / skip: the vertex enters with no count of frames its state block has stood at since it restarted");
            total = hist.back();
            g_rev_entry_log.push_back(s.state[0]);
        } else {
            if (!books_match(s, 0)) die("a fresh vertex whose books are not those of frame 0");
            hist.clear();
        }
        hist.push_back(total + s.frames);
        g_rev_stamp += 1.0;
        s.state[0] = g_rev_stamp;
    }
}
void launch_reverb_sum(const ReverbDesc* d, int n, uint32_t frames, hipStream_t) { check(d, n, 0, frames, 0); }
void launch_reverb(const ReverbDesc* d, int n, uint32_t form, hipStream_t) { check(d, n, 1, 0, form); }

// ---- the guard's launches, wrapped (ld --wrap: the engine's calls arrive here, __real_ is mock_hip.cpp's) ----
void real_band_audit(const AuditHead* h, int n, hipStream_t s) asm("__real__ZN3tdk17launch_band_auditEPKNS_9AuditHeadEiP12ihipStream_t");
void wrap_band_audit(const AuditHead* h, int n, hipStream_t s) asm("__wrap__ZN3tdk17launch_band_auditEPKNS_9AuditHeadEiP12ihipStream_t");
void wrap_band_audit(const AuditHead* h, int n, hipStream_t s) {
    for (int i = 0; i < n; ++i) {
        for (uint32_t j = 0; j < h[i].n; ++j) g_rev_path_gain = (double)h[i].descs[j].gain;
        if (g_rev_force_redo) h[i].host_word[0] = 1u;
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
                g_rev_path_gain = std::sqrt((double)d[i].nz_scale * (double)frames);
                if (g_rev_force_redo && d[i].nz_host) d[i].nz_host[0] = 1u;
            }
    real_band_chain(d, n, frames, a, guarded, s);
}
}  // namespace tdk
