// The saturator launches for the host-only sanitizer build of the engine (TEST INFRASTRUCTURE: linked only by
// tests/test_saturator_host.py beside tests/mock_hip.cpp, never by the product).  Nothing is computed: every launch walks its
// descriptor table and both ends of every array a descriptor points to, so that a descriptor that points past an allocation is
// an AddressSanitizer report, and checks what the kernels rely on -- the tiling (F, n_tiles, the LDS the launch would ask for),
// the taps (length by the launch's factor, symmetric, summing to 1), the constants (g_in, g_out and f(bias) in their ranges), the
// line (2 KB, `filled` <= 128 and equal to the frames the vertex has run since it restarted, the half a launch reads being the half
// a launch before it wrote; nothing after a set_time), chunks shorter than the line, that k_sat_sum comes first exactly when the
// chunk is longer than kSatInlineFrames, and that a launch holds vertices of one oversampling factor only.
// With g_fx_force_redo set the guard's listeners (tests/mock_guard.cpp) tell every audited render to run again.  For that case
// k_sat stamps the half of the line it writes and logs the stamp it finds
// in the half it reads: a render done again must find what the first one found, not what the first one left.
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <cmath>
#include <map>
#include <vector>

#define MOCK_NAME "mock_sat"
#include "mock_util.h"
#include "asan_fx.h"
#include "termdaw_amd.h"

size_t g_fx_launches[3] = {0, 0, 0}, g_fx_vertices = 0, g_fx_single = 0, g_fx_fresh = 0, g_fx_carried = 0;
int g_fx_after_set_time = 0;   // the driver has called td_graph_set_time and not submitted since: every vertex must enter with nothing of its line
size_t g_fx_restarts = 0;      // descriptors checked under that flag
size_t g_fx_short = 0;         // descriptors whose chunk was shorter than the line
std::vector<double> g_fx_entry_log;   // per k_sat descriptor that enters with the line: the stamp found in the half it reads
static float g_fx_stamp = 0.0f;

namespace {
struct LineBook { uint64_t total; uint32_t written; };   // frames since the restart; the half the last launch wrote
// per line: the states it has been in since it restarted, oldest first.  A launch must enter with one of them: the latest, or --
// a guarded render done again, whose line and books the guard has put back -- an earlier one, which then becomes the latest.
std::map<const float2*, std::vector<LineBook>> g_lines;
std::map<const float2*, uint32_t> g_summed;   // x buffers k_sat_sum has filled and k_sat has not read yet -> frames
}  // namespace

namespace tdk {
// which: 0 k_sat_sum, 1 k_sat, 2 k_sat1
static void check(const SatDesc* d, int n, int which, uint32_t R, uint32_t n_tiles, uint32_t F, bool terms, uint32_t frames) {
    touch(d, (size_t)std::max(n, 0) * sizeof(SatDesc));
    g_fx_launches[which] += 1;
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
        touch_terms(s.ins, s.k, s.frames, "a saturator vertex takes terms of kinds 0 .. 4 only");
        touch_w(s.out, (size_t)s.frames * sizeof(float2));
        if (which == 2) {
            if (s.line || s.taps || s.x) die("k_sat1 has no line, no taps and no scratch buffer");
            g_fx_vertices += 1;
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
        g_fx_vertices += 1;
        if (terms) g_fx_single += 1;
        if (s.frames < 128u) g_fx_short += 1;
        (s.filled ? g_fx_carried : g_fx_fresh) += 1;
        if (g_fx_after_set_time) {
            if (s.filled != 0u) die("a vertex entered with its line after a set_time");
            g_fx_restarts += 1;
        }
        std::vector<LineBook>& hist = g_lines[s.line];
        uint64_t total = 0;
        if (s.filled) {
            while (!hist.empty() && !(s.filled == std::min<uint64_t>(hist.back().total, 128u) && s.parity == hist.back().written)) hist.pop_back();
            if (hist.empty()) die("filled / parity: the vertex enters with no state its line has been in since it restarted");
            total = hist.back().total;
            g_fx_entry_log.push_back((double)s.line[s.parity * 128u + 127u].x);
        } else {
            hist.clear();
        }
        hist.push_back(LineBook{total + s.frames, s.parity ^ 1u});
        g_fx_stamp += 1.0f;
        for (uint32_t m = 0; m < 128u; ++m) s.line[(s.parity ^ 1u) * 128u + m] = make_float2(g_fx_stamp, g_fx_stamp);
    }
}
void launch_sat_sum(const SatDesc* d, int n, uint32_t frames, hipStream_t) { check(d, n, 0, 0, 0, 0, false, frames); }
void launch_sat(const SatDesc* d, int n, uint32_t R, uint32_t n_tiles, uint32_t F, bool terms, hipStream_t) { check(d, n, 1, R, n_tiles, F, terms, 0); }
void launch_sat1(const SatDesc* d, int n, uint32_t frames, hipStream_t) { check(d, n, 2, 1, 0, 0, false, frames); }
}  // namespace tdk

// ---- what tests/asan_fx.cpp needs to know about the kind: 256 and (chunked, odd modes) 128 frames per tile; the 4 096-frame chunks
// are the one-launch form
const FxHooks g_fx = {
    "sat",
    [](td_state* s, int mode, int chunked) {
        if (chunked && (mode & 1)) td_state_set_option(s, "debug.sat_tile", 128);
    },
    []() {
        if (g_fx_launches[1] >= g_fx_launches[0]) return true;   // (every k_sat_sum is followed by at least one k_sat)
        fprintf(stderr, "launch counts: k_sat_sum %zu k_sat %zu k_sat1 %zu\n", g_fx_launches[0], g_fx_launches[1], g_fx_launches[2]);
        return false;
    },
    []() {
        printf("k_sat launches %zu (%zu vertices, %zu one-launch, %zu entered fresh, %zu entered with the line; %zu k_sat_sum launches; "
               "%zu k_sat1 launches; %zu restarts checked; %zu short chunks)\n",
               g_fx_launches[1], g_fx_vertices, g_fx_single, g_fx_fresh, g_fx_carried, g_fx_launches[0], g_fx_launches[2], g_fx_restarts, g_fx_short);
    },
};
