// The loudness and mastering launches for the host-only sanitizer build of the engine (TEST INFRASTRUCTURE: linked only by
// tests/test_master_host.py beside tests/mock_hip.cpp and tests/mock_stems.cpp, never by the product).  Nothing is computed:
// every launch walks its descriptor table and both ends of every array a descriptor points to, so that a descriptor that
// points past an allocation is an AddressSanitizer report, and checks the tiling the kernels rely on.  The meter writes a
// non-zero hop energy (a steady -20 LUFS-ish signal) and a true peak of 0.5, so the engine's pass loop runs its passes; the
// apply launch copies the words through unchanged and reports a smallest gain of 1.
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <cmath>

#include "kernels.h"

static volatile unsigned char g_master_sink;
static void touch(const void* p, size_t bytes) {
    if (!p || !bytes) return;
    const volatile unsigned char* b = (const volatile unsigned char*)p;
    g_master_sink ^= b[0];
    g_master_sink ^= b[bytes - 1];
}

size_t g_loud_launches = 0, g_master_launches[4] = {0, 0, 0, 0}, g_master_signals = 0;

namespace tdk {
void launch_loudness(const LoudDesc* d, int n, uint32_t max_tiles, hipStream_t) {
    touch(d, (size_t)std::max(n, 0) * sizeof(LoudDesc));
    g_loud_launches += 1;
    for (int i = 0; i < n; ++i) {
        const LoudDesc& s = d[i];
        if (!s.pcm || !s.peak || !s.energy || s.kind > 2u || !s.hop || s.tile % s.hop || s.n_tiles > max_tiles ||
            (size_t)s.n_tiles * s.tile < s.frames || s.fir[0][5] != 1.0f)
            abort();
        touch(s.pcm, (size_t)s.frames * (s.kind == 0u ? 4 : 8));
        const size_t hops = s.frames / s.hop;
        for (size_t h = 0; h < 2 * hops; ++h) s.energy[h] = 0.01 * s.hop;
        const float half = 0.5f;
        memcpy(&s.peak[0], &half, 4);
        memcpy(&s.peak[1], &half, 4);
    }
}
static void check(const MasterDesc* d, int n, uint32_t max_tiles, int which) {
    touch(d, (size_t)std::max(n, 0) * sizeof(MasterDesc));
    g_master_launches[which] += 1;
    for (int i = 0; i < n; ++i) {
        const MasterDesc& s = d[i];
        const size_t word = s.kind == 0u ? 4 : 8;
        const bool ints = s.kind < 2u;
        if (!s.src || !s.dst || !s.q || !s.agg || !s.carry || !s.gmin || s.kind > 2u || !s.frames || !s.W ||
            s.n_tiles != (s.frames + kMasterTile - 1) / kMasterTile || (max_tiles && s.n_tiles > max_tiles) ||
            (size_t)s.chunk * kThreads < s.n_tiles || (s.chunk > 1 && (size_t)(s.chunk - 1) * kThreads >= s.n_tiles) ||
            !(s.phases == 1u || s.phases == 2u || s.phases == 4u) || s.fir[0][5] != 1.0f ||
            (ints && (s.lo != -s.hi - 1 || !(s.hi == 127 || s.hi == 32767 || s.hi == 8388607 || s.hi == 2147483647))) ||
            !(s.g > 0.0 && std::isfinite(s.g)) || !(s.cp > 0.0 && s.cp <= 1.0) || !(s.a > 0.0 && s.a < 1.0) ||
            ((uintptr_t)s.q & 15u) != 0u)
            abort();
        touch(s.src, s.frames * word);
        touch(s.dst, s.frames * word);
        touch(s.q, (size_t)s.frames * 4);
        touch(s.agg, (size_t)s.n_tiles * 8);
        touch(s.carry, (size_t)s.n_tiles * 8);
        touch(s.gmin, 4);
        if (which == 0) memset(s.q, 0, (size_t)s.frames * 4);
        if (which == 1) memset(s.agg, 0, (size_t)s.n_tiles * 8);
        if (which == 2) memset(s.carry, 0, (size_t)s.n_tiles * 8);
        if (which == 3) {
            memmove(s.dst, s.src, s.frames * word);
            const float one = 1.0f;
            uint32_t b;
            memcpy(&b, &one, 4);
            *s.gmin = std::min(*s.gmin, b);
            g_master_signals += 1;
        }
    }
}
void launch_master_detect(const MasterDesc* d, int n, uint32_t max_tiles, hipStream_t) { check(d, n, max_tiles, 0); }
void launch_master_scan(const MasterDesc* d, int n, uint32_t max_tiles, hipStream_t) { check(d, n, max_tiles, 1); }
void launch_master_carry(const MasterDesc* d, int n, hipStream_t) { check(d, n, 0, 2); }
void launch_master_apply(const MasterDesc* d, int n, uint32_t max_tiles, hipStream_t) { check(d, n, max_tiles, 3); }
}  // namespace tdk
