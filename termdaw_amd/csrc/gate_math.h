// gate_math.h -- host arithmetic of the gate vertex (include/termdaw_amd.h td_graph_add_gate): the six constants
// the kernels take (To, Tc, H, aA, aR, F) and the range checks (shared by the C ABI and the Lua front-end).  No HIP call.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

namespace tde {
namespace gate {

// the hold counter c lives in the low 30 bits of a packed word (kernels.h GateDesc): H + 1 must fit
constexpr double kMaxHold = 1073741822.0;

// out[0 .. 5] = To, Tc, H, aA, aR, F -- from the f32 parameters, widened
inline void params(size_t sr, float threshold_db, float hysteresis_db, float hold_ms, float attack_ms, float release_ms, float range_db,
                   double out[6]) {
    out[0] = pow(10.0, (double)threshold_db / 20.0);
    out[1] = pow(10.0, ((double)threshold_db - (double)hysteresis_db) / 20.0);
    out[2] = (double)llround((double)hold_ms * (double)sr / 1000.0);
    out[3] = attack_ms > 0.0f ? exp(-1.0 / ((double)attack_ms * (double)sr / 1000.0)) : 0.0;
    out[4] = exp(-1.0 / ((double)release_ms * (double)sr / 1000.0));
    out[5] = pow(10.0, (double)range_db / 20.0);
}

// nullptr, or what is wrong: the message names the parameter (a NaN fails every comparison)
inline const char* check(float threshold_db, float hysteresis_db, float hold_ms, float attack_ms, float release_ms, float range_db) {
    if (!(threshold_db >= -80.0f && threshold_db <= 0.0f)) return "threshold_db must lie in [-80, 0] dB";
    if (!(hysteresis_db >= 0.0f && hysteresis_db <= 24.0f)) return "hysteresis_db must lie in [0, 24] dB";
    if (!(hold_ms >= 0.0f && hold_ms <= 2000.0f)) return "hold_ms must lie in [0, 2000] ms";
    if (!(attack_ms >= 0.0f && attack_ms <= 1000.0f)) return "attack_ms must lie in [0, 1000] ms";
    if (!(release_ms >= 1.0f && release_ms <= 10000.0f)) return "release_ms must lie in [1, 10000] ms";
    if (!(range_db >= -120.0f && range_db <= 0.0f)) return "range_db must lie in [-120, 0] dB";
    return nullptr;
}

}  // namespace gate
}  // namespace tde
