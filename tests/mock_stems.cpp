// The stem launch for the host-only sanitizer build of the engine (TEST INFRASTRUCTURE: linked only by
// tests/test_stems_host.py beside tests/mock_hip.cpp, never by the product).  Like the other mock launches it computes
// nothing: it walks both ends of the descriptor table, of every array a descriptor points to -- the materialised frames or
// the loop source's table, the chunk's PCM slice, the f32 copy, the peak word -- so that a stem descriptor that points past
// an allocation is an AddressSanitizer report.  It also counts what it saw, for the driver's summary.
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include <stdio.h>

#include <algorithm>

#include "kernels.h"

static volatile unsigned char g_stem_sink;
static void touch(const void* p, size_t bytes) {
    if (!p || !bytes) return;
    const volatile unsigned char* b = (const volatile unsigned char*)p;
    g_stem_sink ^= b[0];
    g_stem_sink ^= b[bytes - 1];
}
static void touch_w(void* p, size_t bytes) {
    if (!p || !bytes) return;
    volatile unsigned char* b = (volatile unsigned char*)p;
    b[0] = b[0];
    b[bytes - 1] = b[bytes - 1];
}

size_t g_stem_launches = 0, g_stem_buffers = 0, g_stem_loops = 0, g_stem_f32 = 0;

namespace tdk {
void launch_stems(const StemDesc* d, int n, uint32_t frames, hipStream_t) {
    touch(d, (size_t)std::max(n, 0) * sizeof(StemDesc));
    g_stem_launches += 1;
    for (int i = 0; i < n; ++i) {
        const InTerm& t = d[i].src;
        if (!t.p || !d[i].peak) abort();
        if (t.kind == 0u) { touch(t.p, (size_t)frames * sizeof(float2)); g_stem_buffers += 1; }
        else if (t.kind == 3u) { touch(t.p, ((size_t)t.len + 15) * 4); g_stem_loops += 1; }
        else if (t.kind == 1u || t.kind == 2u) { touch(t.p, ((size_t)t.len + 15) * sizeof(float2)); g_stem_loops += 1; }
        else abort();   // (a stem is a buffer or a loop source: never a read-through term)
        if (d[i].qmode) touch_w(d[i].pcm, (size_t)frames * 2 * (d[i].qmode == 1u ? 2 : 4));
        if (d[i].f32) { touch_w(d[i].f32, (size_t)frames * sizeof(float2)); g_stem_f32 += 1; }
        touch_w(d[i].peak, 4);
    }
}
}  // namespace tdk
