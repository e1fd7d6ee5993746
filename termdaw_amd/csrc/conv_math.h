// conv_math.h -- host arithmetic of the convolution vertex (include/termdaw_amd.h td_graph_add_convolution): the
// frame counts the kernels take (Lh, D, P, the line's length), the trim g, the twiddle table, and the range checks (shared by
// the C ABI and the Lua front-end).  No HIP call.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

namespace tde {
namespace conv {

constexpr int kParams = 6;
constexpr double kMaxLh = 262144.0;   // frames of response
constexpr double kB = 1024.0;         // the kernels' partition (kernels.h kConvB)
constexpr int kN = 2048;              // points per transform (kernels.h kConvN)

// Lh: the response's frames, from the f32 parameter widened (0: the bank's sample has none, or length_ms rounds to none)
inline double response_frames(size_t sr, size_t sample_len, float length_ms) {
    if (length_ms == 0.0f) return (double)sample_len;
    const long long l = llround((double)length_ms * (double)sr / 1000.0);
    return l < 0 ? 0.0 : (double)((unsigned long long)l < (unsigned long long)sample_len ? (size_t)l : sample_len);
}

// out[0 .. 5] = Lh, D, g (before `norm`), P = ceil((D + Lh) / B), the line's frames D + Lh - 1, B
inline void params(size_t sr, size_t sample_len, float length_ms, float predelay_ms, float out_db, double out[kParams]) {
    out[0] = response_frames(sr, sample_len, length_ms);
    out[1] = (double)llround((double)predelay_ms * (double)sr / 1000.0);
    out[2] = pow(10.0, (double)out_db / 20.0);
    out[3] = ceil((out[1] + out[0]) / kB);
    out[4] = out[1] + out[0] - 1.0;
    out[5] = kB;
}

// nullptr, or what is wrong with the parameters the vertex keeps: the message names the parameter (a NaN fails every
// comparison, an infinity the far end)
inline const char* check(size_t sr, float length_ms, float predelay_ms, float out_db, int norm) {
    if (sr == 0) return "the sample rate is 0";
    if (!(length_ms >= 0.0f && length_ms <= 60000.0f)) return "length_ms must lie in [0, 60000] ms (0: the whole sample)";
    if (!(predelay_ms >= 0.0f && predelay_ms <= 500.0f)) return "predelay_ms must lie in [0, 500] ms";
    if (!(out_db >= -60.0f && out_db <= 24.0f)) return "out_db must lie in [-60, 24] dB";
    if (norm != 0 && norm != 1) return "norm must be 0 or 1";
    return nullptr;
}
// ... and with the response once the bank's sample is known
inline const char* check_len(size_t sr, size_t sample_len, float length_ms) {
    const double lh = response_frames(sr, sample_len, length_ms);
    if (!(lh >= 1.0)) return "length_ms leaves no frame of the sample: the response is empty";
    if (!(lh <= kMaxLh)) return "length_ms: the response is longer than 262144 frames (set length_ms to trim it)";
    return nullptr;
}

// the forward twiddles (cos, -sin)(2 pi j / N), j = 0 .. N / 2 - 1, computed in long double and rounded once
inline void twiddles(double* out) {
    const long double two_pi = 6.283185307179586476925286766559005768L;
    for (int j = 0; j < kN / 2; ++j) {
        const long double a = two_pi * (long double)j / (long double)kN;
        out[2 * j] = (double)cosl(a);
        out[2 * j + 1] = (double)-sinl(a);
    }
}

}  // namespace conv
}  // namespace tde
