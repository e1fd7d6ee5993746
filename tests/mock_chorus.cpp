// The chorus launches for the host-only sanitizer build of the engine (TEST INFRASTRUCTURE: linked only by
// tests/test_chorus_host.py beside tests/mock_hip.cpp, never by the product).  Nothing is computed: every launch walks its
// descriptor table and both ends of every array a descriptor points to, so that a descriptor that points past an allocation is
// an AddressSanitizer report, and checks what the kernels rely on -- the tiling (F, n_tiles, the LDS the launch would ask for),
// the constants (D0, A, f in their ranges, D0 - A >= 2, H a multiple of 64 that holds floor(D0 + A) + 3, the slope bound), the
// absolute time, the line (2 H frames, `filled` <= H and equal to the frames the vertex has run since it restarted, the half a
// launch reads being the half a launch before it wrote; nothing after a set_time), chunks shorter than the line, and that
// k_chorus_sum comes first exactly when the chunk is longer than kSatInlineFrames.
// With g_fx_force_redo set the guard's listeners (tests/mock_guard.cpp) tell every audited render to run again.  For that case
// k_chorus stamps the half of the line it writes and logs the stamp it
// finds in the half it reads: a render done again must find what the first one found, not what the first one left.
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <cmath>
#include <map>
#include <vector>

#define MOCK_NAME "mock_chorus"
#include "mock_util.h"
#include "asan_fx.h"
#include "termdaw_amd.h"

size_t g_fx_launches[3] = {0, 0, 0}, g_fx_vertices = 0, g_fx_single = 0, g_fx_fresh = 0, g_fx_carried = 0;
int g_fx_after_set_time = 0;   // the driver has called td_graph_set_time and not submitted since: every vertex must enter with nothing of its line
size_t g_fx_restarts = 0;      // descriptors checked under that flag
size_t g_fx_short = 0;         // descriptors whose chunk was shorter than the line
std::vector<double> g_fx_entry_log;   // per k_chorus descriptor that enters with the line: the stamp found in the half it reads
static float g_fx_stamp = 0.0f;

namespace {
struct LineBook { uint64_t total; uint32_t written; };   // frames since the restart; the half the last launch wrote
// per line: the states it has been in since it restarted, oldest first.  A launch must enter with one of them: the latest, or --
// a guarded render done again, whose line and books the guard has put back -- an earlier one, which then becomes the latest.
std::map<const float2*, std::vector<LineBook>> g_lines;
std::map<const float2*, uint32_t> g_summed;   // x buffers k_chorus_sum has filled and k_chorus has not read yet -> frames
}  // namespace

namespace tdk {
// which: 0 k_chorus_sum, 1 k_chorus
static void check(const ChorusDesc* d, int n, int which, uint32_t n_tiles, bool terms, uint32_t frames) {
    touch(d, (size_t)std::max(n, 0) * sizeof(ChorusDesc));
    g_fx_launches[which] += 1;
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
        touch_terms(s.ins, s.k, s.frames, "a chorus vertex takes terms of kinds 0 .. 4 only");
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
        g_fx_vertices += 1;
        if (terms) g_fx_single += 1;
        if (s.frames < s.H) g_fx_short += 1;
        (s.filled ? g_fx_carried : g_fx_fresh) += 1;
        if (g_fx_after_set_time) {
            if (s.filled != 0u) die("a vertex entered with its line after a set_time");
            g_fx_restarts += 1;
        }
        std::vector<LineBook>& hist = g_lines[s.line];
        uint64_t total = 0;
        if (s.filled) {
            while (!hist.empty() && !(s.filled == std::min<uint64_t>(hist.back().total, s.H) && s.parity == hist.back().written)) hist.pop_back();
            if (hist.empty()) die("filled / parity: the vertex enters with no state its line has been in since it restarted");
            total = hist.back().total;
            g_fx_entry_log.push_back((double)s.line[(size_t)s.parity * s.H + s.H - 1u].x);
        } else {
            hist.clear();
        }
        hist.push_back(LineBook{total + s.frames, s.parity ^ 1u});
        g_fx_stamp += 1.0f;
        for (uint32_t m = 0; m < s.H; ++m) s.line[(size_t)(s.parity ^ 1u) * s.H + m] = make_float2(g_fx_stamp, g_fx_stamp);
    }
}
void launch_chorus_sum(const ChorusDesc* d, int n, uint32_t frames, hipStream_t) { check(d, n, 0, 0, false, frames); }
void launch_chorus(const ChorusDesc* d, int n, uint32_t n_tiles, uint32_t frames, bool terms, hipStream_t) { check(d, n, 1, n_tiles, terms, frames); }
}  // namespace tdk

// ---- what tests/asan_fx.cpp needs to know about the kind: 256 and (chunked, odd modes) 512 frames per tile; the 4 096-frame chunks
// are the one-launch form
const FxHooks g_fx = {
    "chorus",
    [](td_state* s, int mode, int chunked) {
        if (chunked && (mode & 1)) td_state_set_option(s, "debug.chorus_tile", 512);
    },
    []() {
        if (g_fx_launches[1] >= g_fx_launches[0]) return true;   // (every k_chorus_sum is followed by a k_chorus)
        fprintf(stderr, "launch counts: k_chorus_sum %zu k_chorus %zu\n", g_fx_launches[0], g_fx_launches[1]);
        return false;
    },
    []() {
        printf("k_chorus launches %zu (%zu vertices, %zu one-launch, %zu entered fresh, %zu entered with the line; %zu k_chorus_sum launches; "
               "%zu restarts checked; %zu short chunks)\n",
               g_fx_launches[1], g_fx_vertices, g_fx_single, g_fx_fresh, g_fx_carried, g_fx_launches[0], g_fx_restarts, g_fx_short);
    },
};
