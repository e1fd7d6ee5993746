// The reverb launches for the host-only sanitizer build of the engine (TEST INFRASTRUCTURE: linked only by
// tests/test_reverb_host.py beside tests/mock_hip.cpp, never by the product).  Nothing is computed: every launch walks its
// descriptor table and both ends of every array a descriptor points to, so that a descriptor that points past an allocation is
// an AddressSanitizer report, and checks what the kernels rely on -- the window length (64 | 128 | 256, no longer than the
// shortest line), the constants (g, d1, d2, w1, w2 in their ranges, the scan's powers the squares of one another), the lines (at
// least 64 frames each, back to back behind the 16 one-pole words, every slot index below its line's length), the books (`pos`,
// `skip` and `fresh` of all 24 lines the ones of ONE count of frames run since the restart, and that count the one the launch
// before left; nothing after a set_time), chunks shorter than the window, and that k_reverb_sum has filled the buffer k_reverb reads.
// With g_fx_force_redo set the guard's listeners (tests/mock_guard.cpp) tell every audited render to run again.  For that case
// k_reverb stamps the state block's first word and logs the stamp it
// finds there on entry: a render done again must find what the first one found, not what the first one left.
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <cmath>
#include <map>
#include <vector>

#define MOCK_NAME "mock_reverb"
#include "mock_util.h"
#include "asan_fx.h"
#include "termdaw_amd.h"

size_t g_fx_launches[3] = {0, 0, 0}, g_fx_vertices = 0, g_fx_single = 0 /* the serial form */, g_fx_fresh = 0, g_fx_carried = 0;
int g_fx_after_set_time = 0;   // the driver has called td_graph_set_time and not submitted since: every vertex must enter with nothing of its state
size_t g_fx_restarts = 0;      // descriptors checked under that flag
size_t g_fx_short = 0;         // descriptors whose chunk was shorter than the window
std::vector<double> g_fx_entry_log;   // per k_reverb descriptor that enters with its state: the stamp found in the block's first word
static double g_fx_stamp = 0.0;

namespace {
// per state block: the counts of frames run since the restart it has stood at, oldest first.  A launch must enter with one of them:
// the latest, or -- a guarded render done again, whose block and books the guard has put back -- an earlier one, which then
// becomes the latest.
std::map<const double*, std::vector<uint64_t>> g_books;
std::map<const float2*, uint32_t> g_summed;   // x buffers k_reverb_sum has filled and k_reverb has not read yet -> frames
}  // namespace

namespace tdk {
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
    g_fx_launches[which] += 1;
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
        touch_terms(s.ins, s.k, s.frames, "a reverb vertex takes terms of kinds 0 .. 4 only");
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
        g_fx_vertices += 1;
        if (form == 0u) g_fx_single += 1;
        if (s.frames < s.B) g_fx_short += 1;
        (s.fresh ? g_fx_fresh : g_fx_carried) += 1;
        if (g_fx_after_set_time) {
            if (!s.fresh) die("a vertex entered with its state after a set_time");
            g_fx_restarts += 1;
        }
        std::vector<uint64_t>& hist = g_books[s.state];
        uint64_t total = 0;
        if (!s.fresh) {
            while (!hist.empty() && !(hist.back() > 0 && books_match(s, hist.back()))) hist.pop_back();
            if (hist.empty()) die("pos / skip: the vertex enters with no count of frames its state block has stood at since it restarted");
            total = hist.back();
            g_fx_entry_log.push_back(s.state[0]);
        } else {
            if (!books_match(s, 0)) die("a fresh vertex whose books are not those of frame 0");
            hist.clear();
        }
        hist.push_back(total + s.frames);
        g_fx_stamp += 1.0;
        s.state[0] = g_fx_stamp;
    }
}
void launch_reverb_sum(const ReverbDesc* d, int n, uint32_t frames, hipStream_t) { check(d, n, 0, frames, 0); }
void launch_reverb(const ReverbDesc* d, int n, uint32_t form, hipStream_t) { check(d, n, 1, 0, form); }
}  // namespace tdk

// ---- what tests/asan_fx.cpp needs to know about the kind: the window length capped at 64 (chunked, odd modes), the serial form in
// the modes with bit 1
const FxHooks g_fx = {
    "reverb",
    [](td_state* s, int mode, int chunked) {
        if (chunked && (mode & 1)) td_state_set_option(s, "debug.reverb_block", 64);
        if (mode & 2) td_state_set_option(s, "debug.reverb_form", 0);
    },
    []() {
        if (g_fx_launches[1] == g_fx_launches[0]) return true;   // (every k_reverb_sum is followed by a k_reverb)
        fprintf(stderr, "launch counts: k_reverb_sum %zu k_reverb %zu\n", g_fx_launches[0], g_fx_launches[1]);
        return false;
    },
    []() {
        printf("k_reverb launches %zu (%zu vertices, %zu serial-form, %zu entered fresh, %zu entered with the state; %zu k_reverb_sum launches; "
               "%zu restarts checked; %zu short chunks)\n",
               g_fx_launches[1], g_fx_vertices, g_fx_single, g_fx_fresh, g_fx_carried, g_fx_launches[0], g_fx_restarts, g_fx_short);
    },
};
