// filter_math.h -- host arithmetic of the filter vertex (include/termdaw_amd.h td_graph_add_filter): the
// constants the kernels take (g0, k, gmin, gmax, cl, ce, f, S, aA, 1 - aA, aR), the sweep's E(t) restated for the host, and the
// range checks (shared by the C ABI and the Lua front-end).  No HIP call.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

namespace tde {
namespace filter {

constexpr int kParams = 11;

// E(t): the header's fixed sequence of IEEE multiplies and adds, within 7.2e-9 relative of exp(t) over |t| <= 10.5 -- the
// degree-10 Taylor polynomial of exp at t / 16 in Horner form, squared four times.  k_filt_* run the same sequence (filt_exp).
inline double E(double t) {
    const double x = t * 0.0625;
    double p = 1.0;
    p = 1.0 + p * (x * (1.0 / 10.0));
    p = 1.0 + p * (x * (1.0 / 9.0));
    p = 1.0 + p * (x * (1.0 / 8.0));
    p = 1.0 + p * (x * (1.0 / 7.0));
    p = 1.0 + p * (x * (1.0 / 6.0));
    p = 1.0 + p * (x * (1.0 / 5.0));
    p = 1.0 + p * (x * (1.0 / 4.0));
    p = 1.0 + p * (x * (1.0 / 3.0));
    p = 1.0 + p * (x * (1.0 / 2.0));
    p = 1.0 + p * (x * 1.0);
    p = p * p;
    p = p * p;
    p = p * p;
    p = p * p;
    return p;
}

// a one-pole's coefficient over `ms` (the compressor's): exp(-1 / (ms sr / 1000)), 0 for ms = 0
inline double pole(double ms, double sr) { return ms > 0.0 ? exp(-1.0 / (ms * sr / 1000.0)) : 0.0; }

// out[0 .. 10] = g0, k, gmin, gmax, cl, ce, f, S, aA, 1 - aA, aR -- from the f32 parameters, widened
inline void params(size_t sr, int /*kind*/, float freq_hz, float q, float lfo_oct, float rate_hz, float /*stereo*/, int /*shape*/,
                   float env_oct, float sens_db, float attack_ms, float release_ms, double out[kParams]) {
    const double pi = 3.14159265358979323846, ln2 = 0.69314718055994530942, r = (double)sr;
    out[0] = tan(pi * (double)freq_hz / r);
    out[1] = 1.0 / (double)q;
    out[2] = tan(pi * 20.0 / r);
    out[3] = tan(0.45 * pi);
    out[4] = ln2 * (double)lfo_oct;
    out[5] = ln2 * (double)env_oct;
    out[6] = (double)rate_hz / r;
    out[7] = pow(10.0, (double)sens_db / 20.0);
    out[8] = pole((double)attack_ms, r);
    out[9] = 1.0 - out[8];
    out[10] = pole((double)release_ms, r);
}

inline const char* const* kind_names() {   // (the script line's names, TD_FILTER_* in order)
    static const char* const n[4] = {"lowpass", "highpass", "bandpass", "notch"};
    return n;
}
// nullptr, or what is wrong: the message names the parameter (a NaN fails every comparison, an infinity the far end)
inline const char* check(size_t sr, int kind, float freq_hz, float q, float lfo_oct, float rate_hz, float stereo, int shape,
                         float env_oct, float sens_db, float attack_ms, float release_ms) {
    if (!(kind >= 0 && kind <= 3)) return "kind must be 0 (lowpass), 1 (highpass), 2 (bandpass) or 3 (notch)";
    if (!(shape >= 0 && shape <= 1)) return "shape must be 0 (sine) or 1 (triangle)";
    if (sr == 0) return "the sample rate is 0";
    if (!(freq_hz >= 20.0f && (double)freq_hz <= 0.45 * (double)sr)) return "freq_hz must lie between 20 Hz and 0.45 of the sample rate";
    if (!(q >= 0.5f && q <= 30.0f)) return "q must lie in [0.5, 30]";
    if (!(lfo_oct >= 0.0f && lfo_oct <= 4.0f)) return "lfo_oct must lie in [0, 4]";
    if (!(rate_hz >= 0.01f && rate_hz <= 20.0f)) return "rate_hz must lie in [0.01, 20] Hz";
    if (!(stereo >= 0.0f && stereo <= 0.5f)) return "stereo must lie in [0, 0.5]";
    if (!(env_oct >= -8.0f && env_oct <= 8.0f)) return "env_oct must lie in [-8, 8]";
    if (!(sens_db >= 0.0f && sens_db <= 60.0f)) return "sens_db must lie in [0, 60]";
    if (!(attack_ms >= 0.0f && attack_ms <= 1000.0f)) return "attack_ms must lie in [0, 1000]";
    if (!(release_ms >= 1.0f && release_ms <= 10000.0f)) return "release_ms must lie in [1, 10000]";
    return nullptr;
}

}  // namespace filter
}  // namespace tde
