// compile.h -- what the host compiler (compile.cpp) and the device side of the engine (engine.cpp) share.
#pragma once
#include <chrono>
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

// ---- engine.cpp: the device memory the compiler hands out addresses of ----
int upload_tables(td_graph* g, TableCache& tc, const Staging& tmp);   // a vertex' event tables -> its device buffer (queued on the graph's stream)
int ensure_buffers(td_graph* g, size_t frames);                      // the edge-buffer pool holds buffers of >= frames frames; all of them free
void* take_line(td_graph* g, tde::Vertex& v, size_t bytes);   // the block a delay, saturator, chorus or reverb vertex carries (Vertex::line), allocated on first use (nullptr: out of device memory)
float2* take_buffer(td_graph* g);                                    // one edge buffer (nullptr: out of device memory)

}  // namespace tde
