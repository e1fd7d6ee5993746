// comp_math.h -- host arithmetic of the compressor vertex (include/termdaw_amd.h td_graph_add_compressor): its
// ranges.  (Its coefficients are two exponentials, computed where the descriptors are filled: compile_fx.cpp lower_comp.)
#pragma once

namespace tde {
namespace comp {

// nullptr: fine, otherwise the reason
inline const char* check(float threshold_db, float ratio, float attack_ms, float release_ms, float knee_db, float makeup_db) {
    if (!(threshold_db >= -80.0f && threshold_db <= 0.0f)) return "threshold_db must lie in [-80, 0] dB";
    if (!(ratio >= 1.0f && ratio <= 1000.0f)) return "ratio must lie in [1, 1000]";
    if (!(attack_ms >= 0.0f && attack_ms <= 1000.0f)) return "attack_ms must lie in [0, 1000] ms";
    if (!(release_ms >= 1.0f && release_ms <= 10000.0f)) return "release_ms must lie in [1, 10000] ms";
    if (!(knee_db >= 0.0f && knee_db <= 40.0f)) return "knee_db must lie in [0, 40] dB";
    if (!(makeup_db >= -40.0f && makeup_db <= 40.0f)) return "makeup_db must lie in [-40, 40] dB";
    return nullptr;
}

}  // namespace comp
}  // namespace tde
