// master.h -- the host side of loudness mastering (include/termdaw_amd.h td_graph_master): the parameter
// checks, the lookahead window and release coefficient, a signal's MasterDesc for k_master_*, and the pass loop's
// decisions in double from the meter's figures.  Header-only, beside loudness.h: the host engine (engine.cpp) includes it, and
// project.cpp for the parameter checks of td_state_set_master.
#pragma once
#include <math.h>
#include <string.h>

#include <string>

#include "loudness.h"

namespace tde {
namespace mst {
using namespace tdk;

constexpr int kFields = 15;       // TD_MASTER_FIELDS
constexpr int kAimedPasses = 4;   // passes that aim at both targets; one more may follow for the ceiling alone
constexpr double kTolLU = 0.1;    // |I - T| counted as met

// The parameter ranges of the definition; "" when they hold, else a message that names the parameter.
inline std::string check(double target, double ceiling, double lookahead_ms, double release_ms) {
    if (!(target >= -60.0 && target <= 0.0)) return "master: target_lufs must lie in [-60, 0] LUFS";
    if (!(ceiling >= -30.0 && ceiling <= 0.0)) return "master: ceiling_dbtp must lie in [-30, 0] dBTP";
    if (!(lookahead_ms >= 0.1 && lookahead_ms <= 100.0)) return "master: lookahead_ms must lie in [0.1, 100] ms";
    if (!(release_ms >= 1.0 && release_ms <= 10000.0)) return "master: release_ms must lie in [1, 10000] ms";
    return "";
}
// W = max(1, round(lookahead fs / 1000)), half away from zero; a = exp(-1 / (release fs / 1000))
inline uint32_t window(double lookahead_ms, size_t sr) {
    const long long w = llround(lookahead_ms * (double)sr / 1000.0);
    return (uint32_t)(w < 1 ? 1 : w);
}
inline double release_coef(double release_ms, size_t sr) { return exp(-1.0 / (release_ms * (double)sr / 1000.0)); }

// A signal to master: the words as rendered (src, never written), where the mastered words go (dst), how to read them.
struct Signal {
    const void* src = nullptr;
    void* dst = nullptr;
    uint32_t kind = 0;   // 0 int16, 1 int32, 2 f32
    int bits = 16;       // the bit depth (kinds 0 and 1): the saturation range
    size_t frames = 0, sr = 0;
};
inline size_t tiles(size_t frames) { return (frames + kMasterTile - 1) / kMasterTile; }

// Everything of d but the device pointers and this pass' g and cp.
inline void describe(const Signal& s, uint32_t W, double a, MasterDesc& d) {
    memset(&d, 0, sizeof d);
    d.kind = s.kind;
    d.frames = (uint32_t)s.frames;
    d.n_tiles = (uint32_t)tiles(s.frames);
    d.W = W;
    d.chunk = (uint32_t)std::max<size_t>(1, (d.n_tiles + kThreads - 1) / kThreads);
    d.phases = (uint32_t)loud::phases(s.sr);
    d.lo = s.kind == 2u ? 0 : -(int32_t)(((int64_t)1 << (s.bits - 1)));
    d.hi = s.kind == 2u ? 0 : (int32_t)(((int64_t)1 << (s.bits - 1)) - 1);
    d.scale = s.kind == 2u ? 1.0 : loud::word_scale(s.bits);
    d.a = a;
    for (int k = 0; k < 8; ++k) {
        d.pw[k] = pow(a, (double)kMasterRun * (double)(1u << k));
        d.pwc[k] = pow(a, (double)kMasterTile * (double)d.chunk * (double)(1u << k));
    }
    d.a_tile = pow(a, (double)kMasterTile);
    loud::fir(s.sr, d.fir);
}

// One signal's pass loop (the definition's "pass loop"), driven by the figures of each pass.
struct Loop {
    double T = 0.0, C = 0.0;   // targets: LUFS, dBTP
    double g = 1.0, cp = 1.0;  // the next (or last) pass' gain and internal ceiling
    int passes = 0;
    bool done = false, met = false, failed = false;
    void start(double target, double ceiling, double L_in) {
        T = target;
        C = ceiling;
        g = pow(10.0, (T - L_in) / 20.0);
        cp = pow(10.0, C / 20.0);
    }
    // After a pass measured I (LUFS) and TP (dBTP): done, or the next pass' g and cp.
    void after(double I, double TP) {
        ++passes;
        const bool over = !(TP <= C);
        met = fabs(I - T) <= kTolLU && !over;
        if (met) { done = true; return; }
        if (passes < kAimedPasses) {
            if (std::isfinite(I)) g *= pow(10.0, (T - I) / 20.0);
            if (over) cp *= pow(10.0, (C - TP - 0.01) / 20.0);
            return;
        }
        if (!over) { done = true; return; }      // the ceiling holds; the loudness target is missed
        if (passes == kAimedPasses) {            // one more pass for the ceiling alone: g held
            cp *= pow(10.0, (C - TP - 0.01) / 20.0);
            return;
        }
        done = failed = true;
    }
};

}  // namespace mst
}  // namespace tde
