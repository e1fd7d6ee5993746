// The loudness launch for the host-only sanitizer build of the engine (TEST INFRASTRUCTURE: linked only by
// tests/test_loudness_host.py beside tests/mock_hip.cpp and tests/mock_stems.cpp, never by the product).  Like the other mock
// launches it computes nothing: it walks the descriptor table and both ends of every array a descriptor points to -- the
// signal's PCM, its hop-energy slab, its two peak words -- and writes zero energies, so that a descriptor that points past an
// allocation is an AddressSanitizer report.  It also checks the tiling the kernel relies on and counts what it saw.
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>

#include "kernels.h"

static volatile unsigned char g_loud_sink;
static void touch(const void* p, size_t bytes) {
    if (!p || !bytes) return;
    const volatile unsigned char* b = (const volatile unsigned char*)p;
    g_loud_sink ^= b[0];
    g_loud_sink ^= b[bytes - 1];
}

size_t g_loud_launches = 0, g_loud_signals = 0, g_loud_hops = 0;

namespace tdk {
void launch_loudness(const LoudDesc* d, int n, uint32_t max_tiles, hipStream_t) {
    touch(d, (size_t)std::max(n, 0) * sizeof(LoudDesc));
    g_loud_launches += 1;
    for (int i = 0; i < n; ++i) {
        const LoudDesc& s = d[i];
        if (!s.pcm || !s.peak || !s.energy || s.kind > 2u || !s.hop || s.tile % s.hop || s.tile / s.hop > 128u || !s.run ||
            s.run > s.hop || (size_t)kThreads * s.run < s.tile || s.n_tiles > max_tiles ||
            (size_t)s.n_tiles * s.tile < s.frames || (s.n_tiles && (size_t)(s.n_tiles - 1) * s.tile >= s.frames) ||
            !(s.phases == 1u || s.phases == 2u || s.phases == 4u) || s.fir[0][5] != 1.0f)
            abort();
        touch(s.pcm, (size_t)s.frames * (s.kind == 0u ? 4 : 8));
        const size_t hops = s.frames / s.hop;
        if (hops) memset(s.energy, 0, hops * 2 * sizeof(double));
        s.peak[0] = s.peak[0];
        s.peak[1] = s.peak[1];
        g_loud_signals += 1;
        g_loud_hops += hops;
    }
}
}  // namespace tdk
