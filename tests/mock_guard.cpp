// Listens to the guard for the host-only sanitizer builds of the effect vertices (TEST INFRASTRUCTURE: linked by
// tests/test_{eq,delay,saturator,chorus,reverb}_host.py beside tests/mock_hip.cpp, never by the product).  The guard's launches
// of mock_hip.cpp are wrapped at link time (-Wl,--wrap: the engine's calls arrive here, __real_ is mock_hip.cpp's): the static
// gain the engine carried from a guarded launch to the graph's output is kept for the driver to print, and with g_fx_force_redo
// set every audited render is told to run again.
#include <hip/hip_runtime_api.h>

#include <cmath>

#include "kernels.h"

double g_fx_path_gain = 0.0;   // the last guarded launch's static gain to the output (0: none since the driver cleared it)
int g_fx_force_redo = 0;       // every audited render is to be done again

namespace tdk {
void real_band_audit(const AuditHead* h, int n, hipStream_t s) asm("__real__ZN3tdk17launch_band_auditEPKNS_9AuditHeadEiP12ihipStream_t");
void wrap_band_audit(const AuditHead* h, int n, hipStream_t s) asm("__wrap__ZN3tdk17launch_band_auditEPKNS_9AuditHeadEiP12ihipStream_t");
void wrap_band_audit(const AuditHead* h, int n, hipStream_t s) {
    for (int i = 0; i < n; ++i) {
        for (uint32_t j = 0; j < h[i].n; ++j) g_fx_path_gain = (double)h[i].descs[j].gain;
        if (g_fx_force_redo) h[i].host_word[0] = 1u;
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
                g_fx_path_gain = std::sqrt((double)d[i].nz_scale * (double)frames);
                if (g_fx_force_redo && d[i].nz_host) d[i].nz_host[0] = 1u;
            }
    real_band_chain(d, n, frames, a, guarded, s);
}
}  // namespace tdk
