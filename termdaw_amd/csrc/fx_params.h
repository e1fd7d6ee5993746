// fx_params.h -- the parameters of the effect kinds, declared once per kind: a block of the vertex (Vertex::fx) with the field
// names of include/termdaw_amd.h in the order of the script line, and the type of the schema (compile.h FxKind::params, rows in
// compile_fx.cpp) that the script line's binder, its dump and its checks are derived from (project.cpp).  Host only.
#pragma once
#include <cstddef>
#include <cstdint>

namespace tde {

struct CompParams { float threshold_db, ratio, attack_ms, release_ms, knee_db, makeup_db; };
struct EqParams { int kind; float freq_hz, q, gain_db; };   // TD_EQ_*
struct DelayParams { float time_ms, feedback, cross; };
struct SatParams { int kind; float drive_db, bias, out_db; int oversample; };   // TD_SAT_*, R
struct ChorusParams { int voices; float delay_ms, depth_ms, rate_hz, stereo; int shape; };   // V, TD_CHORUS_*
struct ReverbParams { float room, damp, width, size; };
struct GateParams { float threshold_db, hysteresis_db, hold_ms, attack_ms, release_ms, range_db; };
struct PhaserParams { int stages; float lo_hz, hi_hz, rate_hz, feedback, stereo; int shape; };   // N, TD_CHORUS_*
struct VocoderParams { int bands; float lo_hz, hi_hz, q, response_ms, out_db; };   // B
struct FilterParams { int kind; float freq_hz, q, lfo_oct, rate_hz, stereo; int shape; float env_oct, sens_db, attack_ms, release_ms; };   // TD_FILTER_*, TD_CHORUS_*
struct LimiterParams { float ceiling_db, lookahead_ms, release_ms, drive_db; };
struct MbParams { float lo_hz, hi_hz, threshold_db[3], ratio[3], attack_ms, release_ms, knee_db, makeup_db[3]; };   // per band: low, mid, high
struct ConvParams { float length_ms, predelay_ms, out_db; int norm; };   // (the response: Vertex::sample_index)

// A vertex holds the block of its own kind only; nothing reads another kind's.  The largest block first: FxParams{} is all-zero.
union FxParams {
    MbParams mb;
    CompParams comp;
    EqParams eq;
    DelayParams delay;
    SatParams sat;
    ChorusParams chorus;
    ReverbParams reverb;
    GateParams gate;
    PhaserParams phaser;
    VocoderParams vocoder;
    FilterParams filter;
    LimiterParams limiter;
    ConvParams conv;
};
static_assert(sizeof(FxParams) == sizeof(MbParams), "FxParams{}: the multiband's block covers the union");

// One argument of a kind's script line behind (name, gain, angle, wet), in the line's order.
struct FxParam {
    enum Type {
        F32,
        INT,      // a number in the script that must be one of `allowed`, an int in the block
        NAME,     // a string in the script, its index in `names` in the block
        SAMPLE,   // a load_sample name in the script, resolved to Vertex::sample_index when the graph is built; not in the block
    };
    const char* name;
    Type type;
    size_t offset;               // of the field in the kind's block
    const char* const* names;    // NAME: the names, in the order of their constants
    int n_names;
    uint32_t allowed;            // INT: bit v is set for every value v the parameter takes
    const char* domain;          // INT: as in "<name> must be <domain>"
};
#define FX_PARAM(S, field, type, names, n_names, allowed, domain) {#field, FxParam::type, offsetof(S, field), names, n_names, allowed, domain}
#define FX_F32(S, field) FX_PARAM(S, field, F32, nullptr, 0, 0, nullptr)
#define FX_SCHEMA(p) p, (int)(sizeof p / sizeof *p)   // FxKind::params, n_params

}  // namespace tde
