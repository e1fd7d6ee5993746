// The convolution launches for the host-only sanitizer build of the engine (TEST INFRASTRUCTURE: linked only by
// tests/test_convolution_host.py beside tests/mock_hip.cpp and tests/mock_guard.cpp, never by the product).  Nothing is computed:
// every launch walks its descriptor table and both ends of every array a descriptor points to, so that a descriptor that points
// past an allocation is an AddressSanitizer report, and checks what the kernels rely on: the tiling (1 024-frame tiles, the
// partition count P = ceil((D + Lh) / 1 024), the window count n_tiles + P - 1 against the launch's grid), the line (two halves
// of D + Lh - 1 frames; `fresh` exactly when the vertex has not run since it restarted, always right after a set_time; otherwise
// the half it reads is one a launch wrote whole), the extents of the window spectra, the products and the partition spectra
// (apart from each other), the response inside its sample, the twiddle table, that the spectra a k_conv_fwd uses are ones
// k_conv_ir has built from the same response (address, length, pre-delay, norm), and that a vertex' three launches come in order
// with the descriptor the first one saw.
// With g_fx_force_redo set the guard's listeners (tests/mock_guard.cpp) tell every audited render to run again.  For that case
// k_conv_inv stamps the half it writes and logs the stamp it finds in the half it reads: a render done again must find what the
// first one found.
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <map>
#include <vector>

#define MOCK_NAME "mock_conv"
#include "mock_util.h"
#include "asan_fx.h"
#include "termdaw_amd.h"

size_t g_fx_launches[3] = {0, 0, 0}, g_fx_vertices = 0, g_fx_single = 0, g_fx_fresh = 0, g_fx_carried = 0;   // [0] k_conv_fwd, [1] k_conv_mac, [2] k_conv_inv: descriptors
int g_fx_after_set_time = 0;
size_t g_fx_restarts = 0;
size_t g_fx_short = 0;         // (descriptors whose chunk was shorter than the line: frames < D + Lh - 1)
std::vector<double> g_fx_entry_log;
static float g_fx_stamp = 0.0f;
static size_t g_ir_built = 0, g_many_partitions = 0;

namespace {
enum { FWD = 0, MAC = 1, INV = 2 };
struct Track { int phase; tdk::ConvDesc first; };
std::map<const double*, Track> g_by_xs;                                  // vertices between k_conv_fwd and k_conv_inv
std::map<const float2*, bool> g_line_ran;                                // line -> it has been written since it restarted
std::map<const double*, std::pair<const float2*, uint64_t>> g_built;     // spectra block -> the response (address, shape) it was built from
uint64_t shape(const tdk::ConvDesc& s) { return ((uint64_t)s.Lh << 32) ^ ((uint64_t)s.D << 8) ^ s.norm; }
}  // namespace

namespace tdk {
static void check_common(const ConvDesc& s) {
    if (!s.ir || !s.spec || !s.tw) die("null pointer in a ConvDesc");
    if (!(s.Lh >= 1u && s.Lh <= 262144u)) die("the response's length");
    if (s.D > 48000u) die("the pre-delay");
    if (s.P != (s.D + s.Lh + kConvB - 1u) / kConvB || s.hist != s.D + s.Lh - 1u) die("partitions / line length");
    if (s.norm > 1u || s.parity > 1u || s.fresh > 1u) die("norm / parity / fresh");
    if (!(s.g >= 0.00099 && s.g <= 15.85)) die("the trim");
    if (((uintptr_t)s.spec & 15u) || ((uintptr_t)s.tw & 15u) || ((uintptr_t)s.ir & 7u)) die("alignment");
    touch(s.ir, (size_t)s.Lh * sizeof(float2));
    touch(s.tw, (size_t)kConvN * sizeof(double));
    if (s.tw[0] != 1.0 || s.tw[1] != 0.0 || std::fabs(s.tw[2 * 512] - 0.0) > 1e-15 || s.tw[2 * 512 + 1] != -1.0) die("the twiddle table");
    touch_w(s.spec, (kConvHead + (size_t)s.P * kConvBins * 4u) * sizeof(double));
}
void launch_conv_ir(const ConvDesc* d, int n, uint32_t grid_x, hipStream_t) {
    touch(d, (size_t)std::max(n, 0) * sizeof(ConvDesc));
    if (n <= 0) die("an empty launch");
    uint32_t need = 0;
    for (int i = 0; i < n; ++i) {
        const ConvDesc& s = d[i];
        check_common(s);
        need = std::max(need, s.P);
        g_built[s.spec] = std::make_pair(s.ir, shape(s));
        s.spec[0] = s.spec[1] = 1.0;   // (the sums a response with energy leaves; the bank's samples are all zero here)
        s.spec[2] = s.g;
        g_ir_built += 1;
    }
    if (grid_x != need) die("k_conv_ir's grid");
}
static void check(const ConvDesc* d, int n, uint32_t grid_x, int which) {
    touch(d, (size_t)std::max(n, 0) * sizeof(ConvDesc));
    if (n <= 0) die("an empty launch");
    uint32_t need = 0;
    for (int i = 0; i < n; ++i) {
        const ConvDesc& s = d[i];
        check_common(s);
        if (!s.ins || !s.out || !s.x || !s.xs || !s.ys) die("null pointer in a ConvDesc");
        if (s.hist && !s.line) die("no line");
        if (!s.frames || s.n_tiles != (s.frames + kConvB - 1u) / kConvB) die("tiling");
        if (!(s.wet >= 0.0001f && s.wet <= 1.0f)) die("wet");
        if (s.hist_groups != std::min<uint32_t>(kConvHistGroups, (s.hist + kConvHistFrames - 1u) / kConvHistFrames)) die("the line's workgroups");
        const uint32_t W = s.n_tiles + s.P - 1u;
        need = std::max(need, which == FWD ? W : which == MAC ? ((s.n_tiles + kConvTT - 1u) / kConvTT) * kConvMacGroups : s.n_tiles + s.hist_groups);
        if ((((uintptr_t)s.out) | ((uintptr_t)s.x) | ((uintptr_t)s.xs) | ((uintptr_t)s.ys)) & 15u) die("buffer alignment");
        if ((const void*)s.x == (const void*)s.out) die("buffers alias");
        auto bt = g_built.find(s.spec);
        if (bt == g_built.end() || bt->second != std::make_pair(s.ir, shape(s))) die("spectra used that k_conv_ir has not built from this response");
        touch_terms(s.ins, s.k, s.frames, "a convolution vertex takes terms of kinds 0 .. 4 only");
        touch_w(s.out, (size_t)((s.frames + 1u) & ~1u) * sizeof(float2));
        touch_w(s.x, (size_t)((s.frames + 1u) & ~1u) * sizeof(float2));
        const size_t xb = (size_t)W * kConvN * 2u * sizeof(double), yb = (size_t)s.n_tiles * kConvN * 2u * sizeof(double);
        touch_w(s.xs, xb);
        touch_w(s.ys, yb);
        const uintptr_t a = (uintptr_t)s.xs, c = (uintptr_t)s.ys;
        if (a < c + yb && c < a + xb) die("window spectra and products overlap");
        if (s.hist) touch_w(s.line, 2 * (size_t)s.hist * sizeof(float2));
        // the order of a vertex' launches, with the descriptor the first one saw
        if (which == FWD) {
            if (g_by_xs.count(s.xs) && g_by_xs[s.xs].phase != 0) die("a vertex' scratch reused before its launches finished");
            g_by_xs[s.xs] = Track{MAC, s};
        } else {
            auto it = g_by_xs.find(s.xs);
            if (it == g_by_xs.end() || it->second.phase != which) die("launch order");
            if (memcmp(&it->second.first, &s, sizeof s) != 0) die("descriptor changed between launches");
            it->second.phase = which == MAC ? INV : 0;
        }
        g_fx_launches[which] += 1;
        if (which != INV) continue;
        // ---- k_conv_inv: the line's books
        g_fx_vertices += 1;
        if (s.n_tiles == 1u) g_fx_single += 1;
        if (s.frames < s.hist) g_fx_short += 1;
        if (s.P > 64u) g_many_partitions += 1;
        (s.fresh ? g_fx_fresh : g_fx_carried) += 1;
        if (g_fx_after_set_time) {
            if (!s.fresh) die("a vertex entered with its line after a set_time");
            g_fx_restarts += 1;
        }
        if (!s.hist) continue;
        const float2* lr = s.line + (size_t)s.parity * s.hist;
        float2* lw = s.line + (size_t)(s.parity ^ 1u) * s.hist;
        if (!s.fresh) {
            if (!g_line_ran[s.line]) die("a vertex enters with a line nothing has written");
            if (!(lr[0].x > 0.0f) || lr[0].x != lr[s.hist - 1u].x) die("the half a vertex reads was not written whole by one launch");
            g_fx_entry_log.push_back((double)lr[0].x);
        }
        g_line_ran[s.line] = true;
        g_fx_stamp += 1.0f;
        for (size_t m = 0; m < s.hist; ++m) lw[m] = make_float2(g_fx_stamp, g_fx_stamp);
    }
    if (grid_x != need) die("the launch's grid against its descriptors");
}
void launch_conv_fwd(const ConvDesc* d, int n, uint32_t grid_x, hipStream_t) { check(d, n, grid_x, FWD); }
void launch_conv_mac(const ConvDesc* d, int n, uint32_t grid_x, hipStream_t) { check(d, n, grid_x, MAC); }
void launch_conv_inv(const ConvDesc* d, int n, uint32_t grid_x, hipStream_t) { check(d, n, grid_x, INV); }
}  // namespace tdk

// ---- what tests/asan_fx.cpp needs to know about the kind: no debug.* options
const FxHooks g_fx = {
    "conv",
    [](td_state*, int, int) {},
    []() {
        if (g_fx_launches[0] == g_fx_launches[1] && g_fx_launches[1] == g_fx_launches[2]) return true;   // (every vertex passes all three steps)
        fprintf(stderr, "descriptor counts: k_conv_fwd %zu k_conv_mac %zu k_conv_inv %zu\n", g_fx_launches[0], g_fx_launches[1], g_fx_launches[2]);
        return false;
    },
    []() {
        printf("k_conv_inv descriptors %zu (%zu vertices, %zu one-tile, %zu entered fresh, %zu entered with the line; %zu k_conv_ir descriptors; "
               "%zu restarts checked; %zu short chunks; %zu over 64 partitions)\n",
               g_fx_launches[2], g_fx_vertices, g_fx_single, g_fx_fresh, g_fx_carried, g_ir_built, g_fx_restarts, g_fx_short, g_many_partitions);
    },
};
