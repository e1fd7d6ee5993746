// compile.h -- what the host compiler (compile.cpp) and the device side of the engine (engine.cpp) share.
#pragma once
#include <chrono>
#include <map>
#include <string>
#include <vector>

#include "engine.h"

namespace tde {

enum Family { F_LOOP, F_MULTI, F_LERP, F_SINE, F_SYNTH, F_SAMPSYN, F_ENV, F_PROBE /* k_sine_probe: behind the sine kinds' launches of its level */, F_SUM, F_SCALE, F_NORMFIX, F_ADSR, F_BAND, F_BAND_SPEC, F_BAND_FIX, F_BAND_FILL, F_BAND_SCAN, F_QUANT, F_AUDIT,
              F_STEMS /* k_stems: the chunk's stems, behind everything else */,
              F_SOURCES /* (no descriptors of its own: several of the families above as ONE grid, submit_chunk) */,
              F_LOUD /* k_loudness: td_graph_loudness / td_batch_loudness, launched outside the render (never compiled) */,
              F_MASTER_DETECT, F_MASTER_SCAN, F_MASTER_CARRY, F_MASTER_APPLY /* k_master_*: td_graph_master / td_batch_master (never compiled) */,
              F_COMP_DETECT, F_COMP_CARRY1, F_COMP_ENV, F_COMP_CARRY2, F_COMP_APPLY /* a level's compressor vertices: k_comp_detect, k_master_carry (y1), k_comp_env, k_master_carry (yL), k_comp_apply -- in this order */,
              F_EQ_LOCAL, F_EQ_CARRY, F_EQ_APPLY /* a level's EQ vertices: k_eq_local, k_eq_carry, k_eq_apply -- in this order */,
              F_DELAY_LOCAL, F_DELAY_CARRY, F_DELAY_APPLY /* a level's delay vertices: k_delay_local, k_delay_carry (both over the vertices whose chunk takes more than one tile only), k_delay_apply -- in this order */,
              F_SAT_SUM, F_SAT, F_SAT1 /* a level's saturator vertices: k_sat_sum (over the vertices whose chunk takes more than one tile only), k_sat (one launch per oversampling factor), k_sat1 (R = 1) */,
              F_CHORUS_SUM, F_CHORUS /* a level's chorus vertices: k_chorus_sum (when the chunk is longer than the one-launch form takes), k_chorus */,
              F_REVERB_SUM, F_REVERB /* a level's reverb vertices: k_reverb_sum, k_reverb -- in this order */,
              F_GATE_DETECT, F_GATE_CARRY_H, F_GATE_ENV, F_GATE_CARRY_ENV, F_GATE_APPLY /* a level's gate vertices: k_gate_detect, k_gate_carry (the (h, c) entering each tile), k_gate_env, k_gate_carry (the env entering each tile), k_gate_apply -- in this order */,
              F_PHASER_LOCAL, F_PHASER_CARRY, F_PHASER_APPLY /* a level's phaser vertices, per stage count: k_phaser_local, k_phaser_carry (both over multi-tile chunks only), k_phaser_apply -- in this order */,
              F_VOC_LOCAL, F_VOC_CARRY, F_VOC_ENV, F_VOC_CARRY_ENV, F_VOC_APPLY /* a level's vocoder vertices, per band count and keyed or not: k_voc_local, k_voc_carry (the biquads' states entering each tile), k_voc_env, k_voc_carry (the followers'), all four over multi-tile chunks only, k_voc_apply -- in this order */,
              F_FILT_DETECT, F_FILT_CARRY1, F_FILT_ENV, F_FILT_CARRY2, F_FILT_LOCAL, F_FILT_CARRY, F_FILT_APPLY /* a level's filter vertices: k_filt_detect, k_master_carry (y1), k_filt_env, k_master_carry (e) -- these four over the vertices whose follower runs -- k_filt_local, k_filt_carry, all six over multi-tile chunks only, k_filt_apply -- in this order */,
              F_LIM_DETECT, F_LIM_CARRY, F_LIM_APPLY /* a level's limiter vertices: k_lim_detect, k_master_carry (the u entering each tile), both over multi-tile chunks only, k_lim_apply -- in this order */,
              F_MB_LOCAL, F_MB_CARRY, F_MB_DETECT, F_MB_CARRY1, F_MB_ENV, F_MB_CARRY2, F_MB_APPLY /* a level's multiband vertices: k_mb_local, k_mb_carry (the crossover's states entering each tile), k_mb_detect, k_master_carry (y1 of the three bands), k_comp_env (over the bands), k_master_carry (yL), all six over multi-tile chunks only, k_mb_apply -- in this order */,
              F_CONV_IR, F_CONV_FWD, F_CONV_MAC, F_CONV_INV /* a level's convolution vertices: k_conv_ir (over the vertices whose spectra have to be built only), k_conv_fwd, k_conv_mac, k_conv_inv -- in this order */,
              F_COUNT };
extern const char* const kFamilyName[F_COUNT];

// ---- compile.cpp ----
void save_state(const Vertex& v, std::string& out);      // the carried host state of an event-driven vertex, as bytes
void load_state(Vertex& v, const std::string& in);
void build_plan(td_graph* g);                            // reachable vertices in topological order, levels (graph.rs:98-121: what the DFS reaches)
// Steps 1 and 2 for ONE graph, appended to `cb` (which several graphs of a batch may share): event tables, descriptors, launches
int compile_chunk(td_graph* g, const td_samplebank* sb, const td_flowwbank* fb, const std::vector<BlockCursor>& cur, uint64_t t0,
                  bool is_scan, void* pcm_dst, int qmode, float amplitude, ChunkBuild& cb);
size_t desc_size(int fam);
bool is_band_family(int fam);
bool is_delay_family(int fam);
double ms_between(std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b);
tdk::PanGain make_pg(float gain, float angle);           // a vertex' pan / gain as its kernel's epilogue applies it (sample.rs:98-109)

// ---- compile_fx.cpp: the effect kinds (compressor, EQ, delay, saturator, chorus, reverb, gate, phaser, vocoder, filter, limiter, multiband, convolution) ----
// What lowering the vertices of one effect kind at one level needs of compile_chunk, and the steps every kind's lowering
// shares.  The kinds' own functions (lower_comp ..) keep what is theirs: coefficients, tiling, scratch, launches.
struct FxLevel {
    td_graph* g;
    ChunkBuild& cb;
    size_t M, sr, bl;     // frames of the chunk, sample rate, reference block length
    uint64_t t0;          // the chunk's first frame on the timeline
    int lv;
    bool is_scan;
    int fam;              // the family the level's loop has reached (FxKind::family of the vertices handed over)
    std::map<size_t, size_t>& ins_off;        // vertex -> staging offset of its input terms
    std::map<size_t, uint32_t>& term_mode;    // vertex -> TERMS_* of those
    std::map<size_t, size_t>& key_off;        // keyed compressor / gate / vocoder / filter vertex that reads its key (Vertex::reads_key) -> staging offset of its key terms
    std::map<size_t, uint32_t>& key_mode;     // ... -> TERMS_* of those
    std::vector<float2*>& level_tmp;          // scratch edge buffers, given back behind the level
    const td_samplebank* sb;                  // the bank of the render (a convolution vertex' response)

    float2* tmp_buffer();   // an edge buffer for this level only; nullptr: failed (g_error set)
    // the fields every effect descriptor has, under the same names
    template <class D>
    void head(D& x, size_t vi) {
        const Vertex& v = g->vertices[vi];
        x.out = g->vbuf[vi];
        x.k = (uint32_t)g->edges[vi].size();
        x.term_mode = term_mode[vi];
        x.frames = (uint32_t)M;
        x.wet = v.wet;
        x.pg = make_pg(v.gain, v.angle);
    }
    // the descriptors of vertices `vs` into the arena, each pointed at its vertex' input terms; returns their offset
    template <class D>
    size_t put(const std::vector<D>& d, const std::vector<size_t>& vs) {
        const size_t off = cb.st->put(d);
        for (size_t i = 0; i < vs.size(); ++i) cb.ptr_field(off + i * sizeof(D), offsetof(D, ins), ins_off[vs[i]]);
        return off;
    }
    // the vertices of `vs` without a key first, the keyed ones behind them, each group in the order it came in; returns how many
    // have no key.  The keyed forms of the detect (and the gate's env) launch run over the second group only, so the unkeyed
    // launches keep the code, registers and occupancy they have without any key in the graph.
    size_t keyed_last(std::vector<size_t>& vs) const {
        std::vector<size_t> a, b;
        for (size_t vi : vs) (key_off.count(vi) ? b : a).push_back(vi);
        vs = a;
        vs.insert(vs.end(), b.begin(), b.end());
        return a.size();
    }
    // a keyed descriptor's key fields (CompDesc / GateDesc / VocDesc; key_ins is pointed at key_off[vi] once the descriptors are staged)
    template <class D>
    void key_fields(D& x, size_t vi) {
        x.key_k = (uint32_t)g->key_edges[vi].size();
        x.key_term_mode = key_mode[vi];
    }
    void add_launch(int family, size_t off, int n, uint32_t aux) {
        cb.launches.push_back({family, off, n, aux, lv, (uint32_t)M, (uint32_t)bl, is_scan ? 1 : 0});
    }
};

// One row per effect kind (the table: compile_fx.cpp), in the order of their families in `Family` -- the order a level launches them
// in.  Everything the compiler, the engine AND the project front end know of a kind: a new kind is a row, its parameter block
// (fx_params.h) and its functions, and td_graph_add_* / td_*_params in the public header.  The row's second half is the kind as the
// front ends see it: its script line `script`(name, gain, angle, wet, params ...), the parameters' schema in that order -- from
// which project.cpp binds, checks and dumps the line -- and what adding a vertex does beyond storing the block (engine.cpp add_fx).
constexpr double kNoStaticGain = -1.0;   // FxKind::through: no estimate is carried through this vertex
struct FxKind {
    Kind kind;
    const char* name;       // as in "<name>: chunk too long"
    const char* k;          // as in "this build has no k_<k> kernels"
    int first_family;       // the kind's families are [first_family, first_family + n_families)
    int n_families;
    size_t desc_bytes;      // of the descriptors its launches take (the compressor's, the filter's and the multiband's two carries and the limiter's one aside: MasterDesc; the multiband's F_MB_ENV: CompDesc)
    int state_slots;        // the consecutive StateSlots of td_graph::dstate a vertex carries from Vertex::state_slot on; 0: a Vertex::line, or nothing
    bool takes_key;         // td_graph_connect_key may end at a vertex of this kind
    bool (*fits)(const td_graph* g, const Vertex& v, size_t M);   // a chunk of M frames is within the kernels' index ranges
    int (*family)(const Vertex& v);                               // the family a vertex is lowered at; nullptr: first_family (all but the saturator)
    // the factor the guard's estimate goes through a vertex at, its own pan / gain aside (1 when dry); kNoStaticGain: none
    double (*through)(const Vertex& v, size_t sr);
    // descriptors + launches of the level's vertices of one family (FxLevel::fam), called where the level's loop reaches it; 0: failed
    int (*lower)(FxLevel& L, std::vector<size_t>& vs);
    // one of those launches onto the stream, `d` its descriptors on the device: decodes the Launch::aux that `lower` encoded
    void (*launch)(const Launch& L, const void* d, hipStream_t s);
    bool built;               // the weak launch_* entry points of the kind are linked
    bool keyed_built;         // ... and those of its keyed forms (true where there are none beyond `built`)
    const char* keyed_name;   // as in "this build has no keyed <keyed_name> kernels"
    void (*rest)(const td_graph* g, const Vertex& v, StateSlot* run);   // the state at time 0 into the vertex' slots; nullptr: all-zero bytes (put at add too: the gate's, closed, depends on the parameters)
    const char* script;       // the script line's function, "add_<kind>"
    const char* script_prefix;   // in front of a reason at the script line: "add_<kind>: " (two kinds name themselves twice)
    const FxParam* params;    // the line's arguments behind wet, in its order
    int n_params;
    // the parameters at rate sr: nullptr, or the reason without a prefix.  rate_free: only the ranges that do not depend on the rate
    const char* (*check)(size_t sr, const FxParams& p, bool rate_free);
    // what of `check` the script line is held to, where its number is known (the rest fails when the graph is built): the
    // compressor's nothing, the EQ's and the delay's the rate-free ranges, every later kind's all of it at the project's rate
    enum LineCheck { LINE_NONE, LINE_RATE_FREE, LINE_FULL } line_check;
    bool starts_pending;      // a vertex is added with Vertex::first_pending set: its line, once it exists, is read only where the vertex itself has written it
    void (*settle)(FxParams& p);   // the block as the vertex keeps it (the EQ's: no gain_db on a kind without gain); nullptr: as given
    int family_of(const Vertex& v) const { return family ? family(v) : first_family; }
    void put_rest(const td_graph* g, const Vertex& v, StateSlot* run) const {
        memset(run, 0, (size_t)state_slots * sizeof(StateSlot));
        if (rest) rest(g, v, run);
    }
};
const FxKind* fx_kind(Kind k);          // nullptr: not an effect kind
const FxKind* fx_of_family(int fam);    // nullptr: not an effect kind's family (one array read: submit_chunk asks per launch)

// ---- engine.cpp ----
// An effect vertex of kind `k` with the block `p` (sample_index: a convolution's response): what every td_graph_add_<kind> and the
// project's replay come down to.  0: `p` fails the kind's check, g_error names the kind and the parameter.
int add_fx(td_graph* g, Kind k, const char* name, float gain, float angle, float wet, const FxParams& p, size_t sample_index = 0);
// ... the device memory the compiler hands out addresses of
int upload_tables(td_graph* g, TableCache& tc, const Staging& tmp);   // a vertex' event tables -> its device buffer (queued on the graph's stream)
int ensure_buffers(td_graph* g, size_t frames);                      // the edge-buffer pool holds buffers of >= frames frames; all of them free
void* take_line(td_graph* g, tde::Vertex& v, size_t bytes);   // the block a delay, saturator, chorus, reverb, vocoder, limiter or multiband vertex carries (Vertex::line), allocated on first use (nullptr: out of device memory)
float2* take_buffer(td_graph* g);                                    // one edge buffer (nullptr: out of device memory)
// a convolution vertex' spectra block of `bytes`, for the sample at `src` of `src_len` frames; *build: the block is new or was
// built from another sample, k_conv_ir has to run (nullptr: out of device memory).  A line of another size than line_bytes goes.
void* take_spectra(td_graph* g, tde::Vertex& v, size_t bytes, const void* src, size_t src_len, size_t line_bytes, bool* build);
const double* take_twiddles(td_graph* g);                            // the transforms' twiddle table on the graph's device, uploaded once per process and device (nullptr: failed)

}  // namespace tde
