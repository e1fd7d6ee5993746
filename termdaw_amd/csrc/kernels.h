// kernels.h -- descriptor structs and launch wrappers of the gfx950 vertex kernels.
//
// Layout contract (DESIGN.md "Data layout"): every edge buffer is `frames` interleaved stereo frames
// (float2 = {l, r}) in HBM; a kernel launch covers a contiguous run of whole reference blocks
// ("chunk") and is batched over same-kind vertices of one topological level through blockIdx.y, each
// vertex described by one descriptor in a device-resident table.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <algorithm>
#include "adsr_math.h"
#include "sum_partition.h"

namespace tdk {

constexpr int kThreads = 256;       // 4 wave64 per workgroup
constexpr int kTileFrames = 1024;
constexpr uint32_t kBandMaxSegs = 131072;   // k_band_fix keeps its mismatch bitmap in LDS
constexpr uint32_t kBandMaxS = 1024;        // ... so chunks beyond 33 M frames take longer segments (any multiple of 256 works: compile.cpp plan_band picks longer ones for batches)   // frames per workgroup tile: 2 x float4 (2 frames each) per thread

// Vertex epilogue: Sample::apply_angle then Sample::apply_gain (sample.rs:97-114, order fixed at
// extensions.rs:262-263).  Amplitudes are computed on the host with libm; flags carry the skip
// thresholds (|angle| < 0.001, |gain-1| < 0.001).
struct PanGain {
    float l_amp, r_amp, gain;
    uint32_t flags;  // bit0: apply pan, bit1: apply gain
};

// One input term of a summing vertex, in connect() order.
//   kind 0: an edge buffer in HBM.
//   kind 1: an inlined sample_loop source (extensions.rs:331-341 + its own pan/gain epilogue): the consumer
//           gathers sample[(t0 + m) % len] itself, so the source's edge buffer never exists (DESIGN.md
//           "source inlining").  32-bit form: t0 + m < 2^32, modulo by Barrett reduction with
//           magic = floor(2^32 / len).
//   kind 2: the same with 64-bit cursor / length (generic modulo).
//   kind 3: kind 1 over the sample's packed 16-bit form: one 32-bit word per frame (int16 l | int16 r << 16), the
//           loop followed by its own first 255 frames (sum_index.h), so that up to 256 consecutive loop frames are dword-aligned
//           16-byte loads behind ONE modulo; the f32 frame is rebuilt as (float)l * scale_l, (float)r * scale_r -- the
//           very expression the load pipeline used to produce the f32 bank entry (sample.rs:270-273 `as f32`,
//           sample.rs:121-129 `* (1.0 / max)`), so the values are bit-identical at half the gather bytes.
//   kind 4: an edge buffer read THROUGH a Sum vertex that has this one input only (a gain / pan stage): the
//           consumer computes `0.0 + x`, pan, gain itself (extensions.rs:310-319, sample.rs:97-114) and the
//           stage is never materialised.
//   kind 5: an edge buffer read through an Adsr vertex that has this one input and one consumer (adsr_gen,
//           extensions.rs:593-651, evaluated per frame by the consumer), optionally followed by a kind-4 stage
//           (magic != 0, `pg` is then the stage's): `len` = device address of the vertex' AdsrVDesc (its input term, its
//           own pan / gain, and `env`: the vertex' per-frame gain `lerp(1.0, adsr_vel, wet)` for this chunk, made once
//           per distinct envelope by k_adsr_env -- the gain depends on the frame and the event tables only, so the 84
//           envelope stages of a deep chain share one).  The consumer's only term (TERMS_ADSR1) or one of several
//           (TERMS_WITH_ADSR).
struct InTerm {
    const float2* p;   // edge buffer (kind 0) or sample frames (kind 1, 2)
    uint64_t len;      // sample length
    uint64_t t0;       // loop cursor at the chunk's first frame
    PanGain pg;        // the source vertex' epilogue
    uint32_t kind;
    uint32_t magic;
    float scale_l, scale_r;   // kind 3
};
enum TermMode : uint32_t { TERMS_MIXED = 0, TERMS_ALL_EDGE = 1, TERMS_ALL_LOOP32 = 2, TERMS_ALL_LOOP16 = 3,
                           TERMS_EDGE_FEW = 4,     // all edge buffers, fewer than 8: no deep prefetch pipeline (and its registers)
                           TERMS_ADSR1 = 5,        // exactly one term, of kind 5
                           TERMS_WITH_ADSR = 6 };  // several terms, at least one of kind 5: summed one term at a time

// Running-peak bookkeeping of normalize_gen (extensions.rs:321-329), carried across chunks / passes.
// `violated` / `ticket` belong to the speculative single-pass normalize (SumDesc mode 3): both are 0 between launches.
struct NormState { float max, scan_max; uint32_t violated, ticket; };

// Block responses of a band-pass vertex' two smoothers, made by the k_sum launch that materialises its input (mode 2)
// and used by k_band_spec as the starting point of its speculative warm-up: for every aligned 256-frame block b and
// chain c (low L, low R, high L, high R)   resp[4 b + c] = sum_i gamma (1 - gamma)^(255 - i) x_c[256 b + i],
// i.e. what the block alone adds to the smoother's state at its end -- in double, so that a few dozen of them chained by
// y <- (1 - gamma)^256 y + resp reproduce the exact-arithmetic state to far below an f32 ulp.
struct BandRespParam {
    double ql[8], qh[8];   // (1 - gamma)^(2^j), j = 0..7, low / high smoother
    double gl, gh;         // the two gammas; 0 = no responses for that smoother (it is constant, or so fast -- gamma >= 0.05,
                           // (1 - gamma)^400 < 2^-30 -- that any starting value has converged long before the window ends)
    double* resp;          // [ceil(frames / 256)][4]
};

// sum_inputs (extensions.rs:310-319), optionally + per-reference-block absolute peak
// (normalize_gen's scan_max, extensions.rs:322 / sample.rs:116-118).
struct SumDesc {
    const InTerm* ins;         // k input terms, in connect() order
    float2* out;
    float* peaks;              // [n_blocks] (mode 1)
    // mode 1: workgroup 0 snapshots the carried normalize state into scratch {max, scan_max} so that pass
    // B can update the state in place without racing its own readers
    const NormState* state;
    float* init_copy;
    float init_max;            // used instead of state->max when use_init (reset_normalization, extensions.rs:295-299)
    uint32_t use_init;
    uint32_t k;
    uint32_t mode;             // 0: Sum vertex (epilogue applied), 1: Normalize pass A (raw sum + peaks),
                               // 2: band-pass input (raw sum + peak of every 256-frame block -> peaks)
                               // 3: Normalize in ONE pass, speculating that no block peak exceeds the carried max (true
                               //    after a normalize scan, graph.rs:222-237, unless carried vertex state makes this
                               //    render louder than the scan was): sum, scale by 1 / max, epilogue, optional quantise
                               //    straight out of registers; block peaks still go to `peaks`, a peak above max sets
                               //    state->violated and k_norm_fix (same descriptors) redoes the vertex the two-pass way
                               // 4: Normalize in ONE pass with the running peak (fresh renders), see `sync` below
                               // 5: the same, for a grid the host expects to be resident at once (k_sum16w, k_norm1, the epilogue
                               //    of k_band_chain).  Same kernel code as mode 4: the wait for earlier tiles is BOUNDED, a tile
                               //    that gives up raises state->violated (and *host_flag) and k_norm_fix redoes the vertex
    uint32_t term_mode;        // TermMode: lets the kernel pick a loop specialised for the term kinds
    uint32_t debug;            // (tests) bit 0: every wait for an earlier tile's granule gives up at once -> violated -> k_norm_fix;
                               // bit 1 (k_sum16w, timing experiments only -- WRONG results): the earlier tiles' words are not read at all
                               // bit 2 (k_sum16w): a tile's one look at the earlier tiles' words sees nothing -- it stores with the running
                               //    peak of its own blocks, waits, and stores again every block whose running peak came out differently
                               // bit 3 (k_sum16w): a tile does NOT store before its wait (the engine sets it unless the early store is
                               //    asked for: kSpecEpilogueDefault, engine option debug.norm bit 3)
    PanGain pg;
    // mode 2: a second copy of the raw sum, planar within every aligned 4-frame block --
    // {l0 l1 l2 l3}{r0 r1 r2 r3} instead of {l0 r0 l1 r1}{l2 r2 l3 r3} -- the form k_band_spec's warm-up
    // walks (one register = one chain's next four inputs).  Same size and word addresses as `out`.
    float2* out_q4;
    // mode 3: fused quantise when the vertex is the output (as in ScaleDesc); `state` is written by k_norm_fix
    void* pcm;
    float amplitude;
    uint32_t qmode;
    const BandRespParam* rp;   // mode 2: block responses wanted (nullptr: not)
    // mode 4 (k_sum16w only): Normalize in ONE pass with the RUNNING peak -- every tile publishes its maximum as a granule
    // in `sync` ([tiles] words, zeroed before the launch) and reads the earlier tiles'; k_norm_fix behind it as in mode 3
    unsigned long long* sync;
    // modes 4 / 5: a word in page-locked HOST memory (device address), set to 1 by a tile whose bounded wait gave up.  Where
    // the vertex is the last thing its submission computes, the engine does not enqueue k_norm_fix behind the launch: it
    // looks at this word once the stream has drained and launches the fix only then (engine.cpp settle()).  nullptr: none.
    uint32_t* host_flag;
    // the ragged form (k_sum16r, mode 5): a reference block can lie in two workgroups, and each contributor has a slot of its
    // own -- `peaks[b]` from the workgroup that owns the block's first quad, `peaks2[b]` from the one that owns its last (0
    // where that is the same workgroup): complete in memory when the launch ends, whatever a wait did.  nullptr: every
    // other form (k_norm_fix folds the two where it is set).
    float* peaks2;
    // modes 4 / 5, k_sum16w: a device word that counts the blocks stored a second time (the early store's running peak did not
    // hold).  nullptr -- no atomic in the launch -- unless engine option debug.norm has bit 2 or bit 4 (td_graph_norm_respec).
    uint32_t* respec;
};
// k_sum16w's modes 4 / 5: does a tile scale and store with the lower tiles' peaks it can see BEFORE it waits for the rest (and
// again where that guess did not hold)?  Engine option debug.norm bit 3 selects the other order.  Measured on the headline
// (docs/EXPERIMENTS.md 000000) -- the gain has to clear ten times the parent's run-to-run spread to become the default.
constexpr bool kSpecEpilogueDefault = false;

// Normalize pass B: running max over the block peaks (`*max = buf_max.max(*max)`), buf.scale(len, 1.0 / max)
// (extensions.rs:323-328), epilogue, optional fused quantise.  Every workgroup derives the running max of
// its own blocks from the peak table (a few KB from L2); the workgroup of the last tile stores the carried
// state.  Scan passes scale by the STALE max and accumulate scan_max instead (quirk Q3).
struct ScaleDesc {
    float2* buf;            // in place
    const float* peaks;     // [n_blocks]
    const float* init_copy; // {max, scan_max} at chunk start
    NormState* state;       // updated by the last tile's workgroup
    void* pcm;              // optional int16/int32 interleaved output
    float amplitude;
    uint32_t qmode;         // 0 none, 1 int16, 2 int32
    PanGain pg;
    uint32_t pcm_only;      // the scaled f32 frames are not written back (engine option "output_f32" 0, set only where nothing in the
                            // render reads them: not when a stem is the output or sits downstream of it)
    uint32_t pad[3];
};

struct QuantDesc {
    const float2* in;
    void* pcm;
    float amplitude;
    uint32_t qmode;
};

// One stem of a chunk (k_stems, engine family F_STEMS): a vertex' frames quantised into a PCM stream of their own, beside the
// output's.  `src` is an input term of kind 0 -- the vertex' materialised edge buffer, pan / gain already applied -- or of kind
// 1 / 2 / 3: an inlined sample_loop source, which k_stems gathers itself through the same device code its consumers use
// (term_pair: the Barrett modulo, the packed 16-bit table, the epilogue), so its edge buffer still never exists.  Every stem
// reduces max |x| over the frames it quantises into `peak` (f32 bits; unsigned order, so a NaN frame wins).
struct StemDesc {
    InTerm src;
    void* pcm;          // this chunk's slice of the stem's PCM (same words as the output's), or nullptr
    float2* f32;        // a copy of the frames (resampled renders: the whole timeline is resampled afterwards), or nullptr
    uint32_t* peak;     // the stem's running peak over the render
    float amplitude;
    uint32_t qmode;     // 0 none, 1 int16, 2 int32
};

// One signal of a loudness measurement (k_loudness; ITU-R BS.1770-4 / EBU Tech 3341 / 3342): interleaved
// stereo words, scaled by `scale` as a WAV reader scales them.  The signal is cut into tiles of `tile` frames (a whole
// number of hops); the workgroup of a tile first runs the K-weighting cascade over the `kThreads * run - tile` frames in
// front of it from zero state (the warm-up: the host sizes it so that the largest pole radius r gives r^warm <= 1e-12),
// with each lane walking `run` frames and the lanes joined by a scan of the cascade's 4-dimensional state through `pw`.
// It stores the sum of squares of the K-weighted channels over every whole hop it owns (energy[hop * 2 + c], plain
// stores) and raises the signal's true / sample peak words (max |x| as f32 bits, atomicMax: order-independent).
struct LoudDesc {
    const void* pcm;
    double* energy;         // [frames / hop][2]
    uint32_t* peak;         // [0] true peak, [1] sample peak (the host zeroes them)
    uint32_t kind;          // 0 int16, 1 int32, 2 f32
    uint32_t frames;
    uint32_t hop;
    uint32_t tile;          // <= 128 hops
    uint32_t run;           // <= hop
    uint32_t n_tiles;
    uint32_t phases;        // true-peak oversampling: 1, 2 or 4
    uint32_t pad;
    double scale;
    double kw[10];          // shelf b0 b1 b2 a1 a2, then high-pass b0 b1 b2 a1 a2 (a0 = 1)
    double pw[8][16];       // A^(run * 2^k), k = 0..7, row-major: A maps the cascade state (s1, s2, t1, t2) one frame on, input 0
    float fir[4][12];       // phase p, tap i: the weight of x[m - 5 + i] in the point at m + p / phases (phase 0: the unit impulse)
};
constexpr uint32_t kLoudTaps = 12;

// One signal of a mastering pass (k_master_detect / k_master_scan / k_master_carry / k_master_apply): a
// lookahead brickwall limiter at gain g under the internal ceiling cp over interleaved stereo words scaled by `scale`.  The
// signal is cut into tiles of kMasterTile frames; a lane owns kMasterRun consecutive frames of a tile.  k_master_detect leaves
// q[n] = max of the detector p over [n, n + W - 1] (p: |x| and the meter's interpolated points next to frame n, as f32);
// the release u[n] = max(1 - h[n], a u[n - 1]) (h = min(1, cp / (g q))) is a (max, x) recurrence: k_master_scan leaves
// each tile's zero-start end value in agg[], k_master_carry the value entering each tile in carry[], and k_master_apply
// rebuilds e = 1 - u from there, forms G as the mean of e over the W frames ending at n (e[0] before frame 0) and writes
// saturate(trunc(w g G)) (f32: (float)(x g G)) to dst, and the smallest G as f32 bits to *gmin (atomicMin).
constexpr uint32_t kMasterRun = 8;                       // frames per lane
constexpr uint32_t kMasterTile = kMasterRun * kThreads;  // frames per workgroup
struct MasterDesc {
    const void* src;        // the words as rendered (never written)
    void* dst;              // the mastered words
    float* q;               // [frames]
    double* agg;            // [n_tiles]
    double* carry;          // [n_tiles]
    uint32_t* gmin;         // the host sets +inf bits
    uint32_t kind;          // 0 int16, 1 int32, 2 f32
    uint32_t frames;
    uint32_t n_tiles;
    uint32_t W;             // lookahead window, frames (1 .. 2^20)
    uint32_t chunk;         // tiles per lane in k_master_carry
    uint32_t phases;        // the meter's true-peak oversampling: 1, 2 or 4
    int32_t lo, hi;         // the bit depth's word range (saturation)
    double scale;
    double g, cp;           // this pass' gain and internal ceiling (linear)
    double pw[8];           // a^(kMasterRun * 2^k)
    double pwc[8];          // a^(kMasterTile * chunk * 2^k)
    double a_tile;          // a^kMasterTile
    double a;               // the release coefficient
    float fir[4][12];       // the meter's FIR (LoudDesc::fir)
    // k_master_carry as the carry of ANOTHER scan (a compressor vertex' two recurrences, CompDesc below -- the kernel reads agg,
    // carry, n_tiles, chunk, a_tile, pwc and these; the mastering passes leave them zero): the value entering tile 0 (device
    // address; nullptr: 0), and the operator -- 0: u <- max(agg, a_tile u), 1: u <- agg + a_tile u
    const double* init;
    uint32_t op, pad_op;
};

// A compressor vertex (k_comp_detect / k_comp_env / k_comp_apply with k_master_carry in between; the definition is
// in include/termdaw_amd.h at td_graph_add_compressor).  The chunk is cut into tiles of kCompTile frames, a lane owns kCompRun
// consecutive frames.  k_comp_detect evaluates the input terms, leaves the summed input in `x` and the wanted reduction d[n]
// (f64) in `dy`, and each tile's zero-start end value of the release  y1 = max(d, aR y1)  in agg1[]; k_master_carry (op 0)
// leaves the y1 entering each tile in carry1[]; k_comp_env rebuilds y1 from there, overwrites dy with it, and leaves each
// tile's zero-start end value of the attack  yL = aA yL + (1 - aA) y1  in agg2[]; k_master_carry (op 1) leaves the yL entering
// each tile in carry2[]; k_comp_apply rebuilds yL, G = 10^((makeup - yL) / 20) and writes lerp(x, (float)(x G), wet), pan,
// gain to `out`.  The lane that owns the chunk's last frame stores y1 (k_comp_env) / yL (k_comp_apply) into the carried state.
constexpr uint32_t kCompRun = 8;                     // frames per lane
constexpr uint32_t kCompTile = kCompRun * kThreads;  // frames per workgroup
struct CompState { double y1, yL; uint32_t pad[4]; };
struct CompDesc {
    const InTerm* ins;      // k input terms (kinds 0 .. 4), in connect() order
    float2* x;              // [frames] the summed input
    double* dy;             // [frames] d, then y1
    float2* out;
    CompState* state;       // carried across chunks / block pulls
    double* agg1;           // [n_tiles] each of the four
    double* carry1;
    double* agg2;
    double* carry2;
    uint32_t k, term_mode, frames, n_tiles;
    float wet;
    uint32_t pad;
    double thr, slope, knee, makeup;   // T, 1 - 1 / R, W, M (dB)
    double aR, aA, oA;      // release / attack coefficients, 1 - aA
    double pwR[8], pwA[8];  // aR^(kCompRun 2^k), aA^(kCompRun 2^k)
    PanGain pg;
    // a keyed vertex (td_graph_connect_key; null / 0 without key edges): key_k key terms (kinds 0 .. 4), in
    // connect_key() order.  k_comp_detect<true> sums them for the level of step 1 -- d[n] is taken from the key frame -- and
    // the input terms into `x` as ever; the later launches read dy and x only and are the unkeyed vertex' own.
    const InTerm* key_ins;
    uint32_t key_k, key_term_mode;
};
// Bit 31 of the aux word of a compressor / gate launch whose descriptors are keyed (the keyed instantiation: F_COMP_DETECT,
// F_GATE_DETECT, F_GATE_ENV); the low bits stay the largest tile count.  A level's unkeyed descriptors go out first, the keyed
// ones in a launch of their own behind them.
constexpr uint32_t kKeyedBit = 0x80000000u;

// A gate vertex (k_gate_detect / k_gate_carry / k_gate_env / k_gate_carry / k_gate_apply; the definition is in
// include/termdaw_amd.h at td_graph_add_gate).  The compressor's tiling: tiles of kGateTile frames, a lane owns kGateRun consecutive
// frames; ONE descriptor read by every launch.
//   The discrete recurrence (h, c) is scanned over a monoid of state maps.  A map is a word per entering h (kGateH: the leaving
//   h; kGateR: "c restarts"; the low 30 bits: k, the closed frames since the restart or on top of the entering c, capped at
//   cap = H + 1).  A state (h, c) is the constant map {h, restart, c}: one word of the same layout.
//   The fade env[n] = a[n] env[n-1] + (1 - a[n]) t[n] is scanned over pairs (A, B): env_out = A env_in + B.
// k_gate_detect evaluates the input terms, leaves the summed input in `x` and each tile's map in map[t]; k_gate_carry (discrete)
// leaves the state word entering each tile in carry_hc[t] (tile 0: *init, or closed when init is nullptr); k_gate_env rebuilds
// t[n] from there, leaves a byte of eight t per lane in tbits, each tile's pair in aggA / aggB and (h, c) behind the chunk's
// last frame in *state; k_gate_carry (affine) leaves the env entering each tile in carry_env[t]; k_gate_apply rebuilds env, G = F +
// (1 - F) env and writes lerp(x, (float)(x G), wet), pan, gain to `out`, and env behind the chunk's last frame to *state.
constexpr uint32_t kGateRun = 8;                     // frames per lane
constexpr uint32_t kGateTile = kGateRun * kThreads;  // frames per workgroup
constexpr uint32_t kGateH = 0x80000000u, kGateR = 0x40000000u, kGateK = 0x3FFFFFFFu;
struct GateState { double env; uint32_t h, c; uint32_t pad[4]; };
struct GateDesc {
    const InTerm* ins;      // k input terms (kinds 0 .. 4), in connect() order
    float2* x;              // [frames] the summed input
    float2* out;
    GateState* state;       // carried across chunks / block pulls
    const GateState* init;  // the state entering tile 0 (k_gate_carry reads it): `state`, or nullptr after a set_time (closed)
    uint32_t* map;          // [2 n_tiles] each tile's map, one packed word pair: word 0 for entering h = 0, word 1 for entering h = 1
    uint32_t* carry_hc;     // [n_tiles] the state word entering each tile
    uint8_t* tbits;         // [n_tiles kThreads] bit j: t of the lane's frame j
    double* aggA;           // [n_tiles] each tile's pair
    double* aggB;
    double* carry_env;      // [n_tiles] the env entering each tile
    uint32_t k, term_mode, frames, n_tiles;
    uint32_t chunk;         // tiles per lane in k_gate_carry
    uint32_t cap;           // H + 1
    float wet;
    uint32_t pad;
    double To, Tc;          // open at s >= To, close at s < Tc (linear)
    double aA, aR, oA, oR;  // attack / release coefficients, 1 - aA, 1 - aR
    double F, oF;           // the closed gain, 1 - F
    PanGain pg;
    // a keyed vertex (td_graph_connect_key; null / 0 without key edges): key_k key terms (kinds 0 .. 4), in
    // connect_key() order.  k_gate_detect<true> sums them for steps 1 and 2 and leaves the lane's eight 2-bit classes as one
    // 16-bit word in cls (frame j of the lane in bits 2 j, 2 j + 1; 0 from `frames` on); k_gate_env<true> reads the word
    // instead of deriving the classes from `x` -- 2 bytes per lane where the unkeyed form reads 64.
    const InTerm* key_ins;
    uint16_t* cls;          // [n_tiles kThreads]
    uint32_t key_k, key_term_mode;
};

// A phaser vertex (k_phaser_local<N> / k_phaser_carry<N> / k_phaser_apply<N>; the definition is in
// include/termdaw_amd.h at td_graph_add_phaser): per channel N first-order all-pass sections in transposed direct form II
// with one swept coefficient a[n] and a feedback fb z around the chain, f64.  One frame is the affine map S -> M[n] S + c[n] xs[n]
// on the state S = (s_1 .. s_N, z) of dimension D = N + 1; M[n] depends on a[n] and fb alone, a[n] on the graph's ABSOLUTE frame
// time (ChorusDesc::t0), so the scan's operator is a D x D matrix plus a D-vector per channel and frame: §3n's blocked scan with
// a per-frame matrix.  A map is stored augmented and row-major, D rows of D + 1 words: {P | q}, S_out = P S_in + q.
// Tiles of kPhaserTile frames; a lane owns kPhaserRun consecutive frames; a workgroup is ONE wave of kPhaserLanes lanes.
// k_phaser_local evaluates the input terms, leaves the summed input in `x` and each tile's total map, per channel, in
// agg[(2 t + c) D (D + 1) ..]; k_phaser_carry leaves the state entering each tile in carry[(2 t + c) D ..] (tile 0: *init, or 0
// when init is null); k_phaser_apply rebuilds the lanes' maps and their in-tile prefix, each lane's entry state from there, and
// runs the definition serially over the lane's run.  When one tile covers the chunk (every block pull) k_phaser_apply runs alone,
// in an instantiation of its own (kPhaserSingleBit): the term loop runs inside it and tile 0 enters with *init (x, agg, carry
// unused).
constexpr uint32_t kPhaserLanes = 64;                            // lanes per workgroup
constexpr uint32_t kPhaserRun = 32;                              // frames per lane
constexpr uint32_t kPhaserTile = kPhaserRun * kPhaserLanes;      // frames per workgroup
constexpr uint32_t kPhaserMaxD = 9;                              // D at 8 stages
struct PhaserState { double s[2][kPhaserMaxD]; double pad[2]; };   // channel c's (s_1 .. s_N, z) in s[c][0 .. N]; five 32-byte slots
struct PhaserDesc {
    const InTerm* ins;      // k input terms (kinds 0 .. 4), in connect() order
    float2* x;              // [frames] the summed input (three-launch form; null in the one-launch form)
    float2* out;
    PhaserState* state;     // carried across chunks / block pulls (k_phaser_apply stores it)
    const PhaserState* init;   // the state entering tile 0: `state`, or nullptr after a set_time
    double* agg;            // [2 n_tiles D (D + 1)] each tile's total map, per channel
    double* carry;          // [2 n_tiles D] the state entering each tile, per channel
    uint64_t t0;            // the graph's absolute frame time at the chunk's first frame (the LFO's n)
    uint32_t k, term_mode, frames, n_tiles;
    uint32_t stages;        // N: 2 | 4 | 6 | 8
    uint32_t shape;         // TD_CHORUS_*
    float wet;
    uint32_t pad;
    double am, ad;          // a[n] = am + ad lfo
    double f;               // LFO cycles per frame
    double fb;              // feedback
    double stereo;          // the right channel's phase offset in cycles
    PanGain pg;
};

// A vocoder vertex (k_voc_local<B, KEYED> / k_voc_carry / k_voc_env<B> / k_voc_carry / k_voc_apply<B>; the
// definition is in include/termdaw_amd.h at td_graph_add_vocoder): B RBJ band-pass biquads (the EQ's transposed direct form II,
// f64) over the carrier's two channels and the mono modulator m = 0.5 (kl + kr), a one-pole follower e_b of |BP_b(m)| per band,
// p = g sum_b e_b BP_b(x).  The compressor's five steps with the EQ's operator inside: per band three 2x2 affine scans that share
// A_b = [[-a1, 1], [-a2, 0]], then one scalar affine scan.  The compressor's tiling: tiles of kVocTile frames, a lane owns kVocRun
// consecutive frames; kVocJoin bands are joined per barrier round.
// k_voc_local evaluates the input terms into `x` (KEYED: and the key terms into `kx`; an unkeyed vertex has kx == x) and leaves
// each tile's zero-start end states (s1l, s2l, s1r, s2r, s1m, s2m) per band in agg[(t B + b) 6 ..]; k_voc_carry (mode 0) leaves the
// states entering each tile in carry[(t B + b) 6 ..] (tile 0: the line, or 0 when init is null); k_voc_env rebuilds BP_b(m) from
// there and leaves each tile's zero-start end value of e_b in agge[t B + b]; k_voc_carry (mode 1) leaves the e_b entering each tile in
// carrye[t B + b]; k_voc_apply rebuilds everything, writes lerp(x, p, wet), pan, gain to `out`, and the lane that owns the chunk's
// last frame writes the line back.  When one tile covers the chunk (every block pull) k_voc_apply runs alone (kVocSingleBit): the
// term loops run inside it and the tile enters with the line (x, kx, agg .. carrye unused).
// The line: 7 doubles per band, (s1l, s2l, s1r, s2r, s1m, s2m, e) at line[7 b ..].
constexpr uint32_t kVocRun = 8;                     // frames per lane
constexpr uint32_t kVocTile = kVocRun * kThreads;   // frames per workgroup
constexpr uint32_t kVocJoin = 4;                    // bands per barrier round (k_voc_local, k_voc_env)
constexpr uint32_t kVocApplyJoin = 2;               // ... in k_voc_apply, which holds every band's full state beside its sums
constexpr uint32_t kVocMaxBands = 16;
constexpr uint32_t kVocState = 7;                   // doubles of the line per band
struct VocBand {
    double b0, b1, b2, a1, a2;   // the normalised band-pass coefficients (td_vocoder_params)
    double c0, c1;          // b1 - a1 b0, b2 - a2 b0
    double pad;
    double pw[8][4];        // A_b^(kVocRun 2^k)
    double a_tile[4];       // A_b^kVocTile
    double pwc[8][4];       // A_b^(kVocTile chunk 2^k)
};
struct VocDesc {
    const InTerm* ins;      // k input terms (kinds 0 .. 4), in connect() order: the carrier
    float2* x;              // [frames] the summed input (five-launch form)
    const float2* kx;       // [frames] the summed key terms (five-launch form): a buffer of its own when keyed, else x
    float2* out;
    double* line;           // carried across chunks / block pulls (k_voc_apply stores it)
    const double* init;     // the state entering tile 0: `line`, or nullptr when the vertex starts afresh
    const VocBand* band;    // [bands]
    double* agg;            // [6 n_tiles bands]
    double* carry;          // [6 n_tiles bands]
    double* agge;           // [n_tiles bands]
    double* carrye;         // [n_tiles bands]
    uint32_t k, term_mode, frames, n_tiles;
    uint32_t chunk;         // tiles per lane in k_voc_carry
    uint32_t bands;         // B: 4 | 8 | 16
    float wet;
    uint32_t pad;
    double a, oa;           // the follower's coefficient, 1 - a
    double g;               // the output gain
    double pwa[8];          // a^(kVocRun 2^k)
    double a_tile;          // a^kVocTile
    double pwac[8];         // a^(kVocTile chunk 2^k)
    PanGain pg;
    // a keyed vertex (td_graph_connect_key; null / 0 without key edges): key_k key terms (kinds 0 .. 4), in connect_key() order
    const InTerm* key_ins;
    uint32_t key_k, key_term_mode;
};

// A filter vertex (k_filt_detect<KEYED> / k_filt_env / k_filt_local / k_filt_carry / k_filt_apply<SINGLE, KEYED> with
// k_master_carry behind the first two; the definition is in include/termdaw_amd.h at td_graph_add_filter): a
// trapezoidal state-variable filter per channel, f64, whose coefficient g[n] follows the chorus' LFO on the graph's ABSOLUTE frame
// time and a linear-domain level follower e[n] of the key (or the input).  Two stages:
//   the follower -- the compressor's pair of scalar scans, y1 = max(s, aR y1) and e = aA e + (1 - aA) y1, in the compressor's
//   tiling: k_filt_detect evaluates the input terms into `x` (KEYED: and the key terms), leaves s[n] (f64) in `lv` and each tile's
//   zero-start end value of y1 in agg1[]; k_master_carry (op 0) the y1 entering each tile in carry1[]; k_filt_env rebuilds y1,
//   overwrites lv with it and leaves each tile's zero-start end value of e in agg2[]; k_master_carry (op 1) the e entering each tile
//   in carry2[].  With `env` 0 (env_oct == 0) none of the four runs and y1, e stay as they are.
//   the filter -- one frame is the affine map z -> M[n] z + b[n] xs[n] on z = (i1, i2), M and b from g[n]: the phaser's blocked
//   scan at D = 2, with both channels' maps in a lane's registers.  A map is stored augmented and row-major, {p00, p01, q0, p10,
//   p11, q1}: z_out = P z_in + q.  k_filt_local rebuilds e (env: overwriting lv with it; otherwise it evaluates the input terms into
//   `x` itself) and leaves each tile's total map, per channel, in agg[(2 t + c) 6 ..]; k_filt_carry leaves the state entering each
//   tile in carry[4 t ..] = (i1l, i2l, i1r, i2r) (tile 0: *init, or 0 when init is null); k_filt_apply rebuilds the lanes' maps
//   from x and lv (g[n] is recomputed, not stored), their in-tile prefix, each lane's entry state, and runs the definition serially.
// Tiles of kFiltTile frames, a lane owns kFiltRun consecutive frames.  When one tile covers the chunk (every block pull)
// k_filt_apply runs alone (kFiltSingleBit): term loops, follower and filter inside, entered with the carried state (x, lv and all
// of agg1 .. carry unused).  The lane that owns the chunk's last frame stores y1 (k_filt_env), e (k_filt_local) and the four
// filter words (k_filt_apply) into the carried state.
constexpr uint32_t kFiltRun = 8;                     // frames per lane
constexpr uint32_t kFiltTile = kFiltRun * kThreads;  // frames per workgroup
struct FiltState { double y1, e, z[2][2]; double pad[2]; };   // z[c] = (i1, i2) of channel c; two 32-byte slots
struct FiltDesc {
    const InTerm* ins;      // k input terms (kinds 0 .. 4), in connect() order
    float2* x;              // [frames] the summed input (multi-tile form)
    double* lv;             // [frames] s, then y1, then e (multi-tile form with env)
    float2* out;
    FiltState* state;       // carried across chunks / block pulls
    const FiltState* init;  // the state entering tile 0: `state`, or nullptr after a set_time
    double* agg1;           // [n_tiles] each of the four (env)
    double* carry1;
    double* agg2;
    double* carry2;
    double* agg;            // [12 n_tiles] each tile's total map, per channel
    double* carry;          // [4 n_tiles] the filter state entering each tile
    uint64_t t0;            // the graph's absolute frame time at the chunk's first frame (the LFO's n)
    uint32_t k, term_mode, frames, n_tiles;
    uint32_t kind;          // TD_FILTER_*
    uint32_t shape;         // TD_CHORUS_*
    uint32_t env;           // 1: the follower runs (env_oct != 0)
    float wet;
    double g0, kq;          // tan(pi freq / sr), 1 / q
    double gmin, gmax;
    double cl, ce;          // ln2 lfo_oct, ln2 env_oct
    double f;               // LFO cycles per frame
    double stereo;          // the right channel's phase offset in cycles
    double S;               // the follower's sensitivity, linear
    double aR, aA, oA;      // release / attack coefficients, 1 - aA
    double pwR[8], pwA[8];  // aR^(kFiltRun 2^k), aA^(kFiltRun 2^k)
    PanGain pg;
    // a keyed vertex (td_graph_connect_key; null / 0 without key edges, and with env 0): key_k key terms (kinds 0 .. 4), in
    // connect_key() order -- the level s[n] is taken from their sum
    const InTerm* key_ins;
    uint32_t key_k, key_term_mode;
};

// A limiter vertex (k_lim_detect / k_master_carry / k_lim_apply; the definition is in include/termdaw_amd.h at
// td_graph_add_limiter): the mastering pass' lookahead limiter in causal form.  The compressor's tiling: tiles of kLimTile frames,
// a lane owns kLimRun consecutive frames; L <= kLimTile, so a tile's halo of L - 1 frames lies within the tile before it -- or,
// for the chunk's first tile, in the carried line.
//   k_lim_detect evaluates the tile's input terms into `x`, forms s over the tile and its halo in LDS (the halo's terms are
//   evaluated a second time for s alone; tile 0 reads the line's frames), the window maximum Q by doubling, stores Q as f32 in `q`
//   and leaves the tile's zero-start end value of the release u = max(1 - h, a u) in agg[t].  k_master_carry (op 0, init the
//   line's u) leaves the u entering each tile in carry[t].  k_lim_apply rebuilds u and e = 1 - u over the tile BEFORE its own from
//   carry[t - 1] (tile 0: reads the line's e) and over its own from carry[t], forms the prefix sums PS of e from frame t0 - L + 1
//   on in lane order, G[n] = (PS[n] - PS[n - L]) / L, reads xd[n] = x[n - L + 1] from `x` or the line and writes lerp(xd,
//   (float)((xd gin) G), wet), pan, gain to `out`.  The workgroup of the chunk's last tile stores the next state.
//   When one tile covers the chunk (every block pull) k_lim_apply runs alone (kLimSingleBit): all of the above in one workgroup,
//   x and s in LDS (x, q, agg, carry unused).
// The line: two halves of 2 L doubles, read at `parity`, written at `parity ^ 1` (no workgroup writes what another of the same
// launch reads).  A half holds what the next chunk needs of the frames before it: word 0 the u of the last frame, words
// 2 .. L the e of the last L - 1 frames, oldest first, words L + 1 .. 2 L - 1 their raw input frames as float2.  Frames before
// the restart are x = 0, e = 1, written out like any other, so a half is always whole; `fresh` (the first chunk since the
// restart): the read half is not read at all.
constexpr uint32_t kLimRun = 8;                    // frames per lane
constexpr uint32_t kLimTile = kLimRun * kThreads;  // frames per workgroup
struct LimDesc {
    const InTerm* ins;      // k input terms (kinds 0 .. 4), in connect() order
    float2* x;              // [frames] the summed input (multi-tile form)
    float* q;               // [frames] Q (multi-tile form)
    float2* out;
    double* line;           // the carried line, 4 L doubles
    double* agg;            // [n_tiles] each tile's zero-start end value of u
    double* carry;          // [n_tiles] the u entering each tile
    uint32_t k, term_mode, frames, n_tiles;
    uint32_t L;             // the lookahead window, frames (1 .. kLimTile)
    uint32_t parity;        // the half this launch reads
    uint32_t fresh;         // 1: the state is that of time 0 (u = 0; the frames before are x = 0, e = 1)
    float wet;
    double c, gin;          // ceiling and drive, linear
    double a;               // the release coefficient
    double pw[8];           // a^(kLimRun 2^k)
    PanGain pg;
};

// A multiband vertex (k_mb_local / k_mb_carry / k_mb_detect / k_master_carry / k_comp_env / k_master_carry / k_mb_apply, DESIGN.md
// §3y; the definition is in include/termdaw_amd.h at td_graph_add_multiband): a three-way Linkwitz-Riley crossover -- nine biquads
// per channel in the EQ's transposed direct form II, f64, a CASCADE -- into three of the compressor's detectors, one per band.
// With z the 18 state words of a channel (biquad i: words 2 i, 2 i + 1; order L1 L1 A2 | H1 H1 | L2 L2 | H2 H2) the crossover is
// z[n] = A z[n-1] + c x[n], A block lower triangular in 2x2 blocks with kMbBlocks of the 81 not zero (multiband_math.h kBlockRow /
// kBlockCol: biquad `col` reaches biquad `row`).  The compressor's tiling: tiles of kMbTile frames, a lane owns kMbRun consecutive frames;
// the lanes' run-end states are joined one channel at a time, 18 planes of LDS.
//   k_mb_local evaluates the input terms into `x` and leaves each tile's zero-start end state in agg[(2 t + ch) 18 ..];
//   k_mb_carry (one workgroup per channel and vertex) the state entering each tile in carry[(2 t + ch) 18 ..] (tile 0: the
//   line's, or 0 when init is null); k_mb_detect rebuilds the lanes' entry states, runs the cascade and writes the wanted
//   reduction d_b[n] (f64) of band b to dy[b], each tile's zero-start end value of the release to agg1[b][t]; k_master_carry
//   (op 0) and k_comp_env -- the compressor's own, over three MasterDesc / CompDesc per vertex -- overwrite dy[b] with y1_b and
//   leave the attack's tile totals, k_master_carry (op 1) the yL_b entering each tile in carry2[b][t]; k_mb_apply rebuilds the
//   band signals and yL_b, G_b = 10^((M_b - yL_b) / 20), p = (float)(((0 + low G_0) + mid G_1) + high G_2), writes lerp(x, p, wet),
//   pan, gain to `out`, and the lane that owns the chunk's last frame writes the 36 filter words and yL_b back (y1_b: k_comp_env).
//   When one tile covers the chunk (every block pull) k_mb_apply runs alone (kMbSingleBit): the term loop and both detector
//   recurrences run inside it and the tile enters with the line; a lane keeps its frames of x, d_b and y1_b in `x` and `dy` as the
//   seven-launch form does and reads back only what it wrote itself (agg .. carry2 unused).
// The line: 42 doubles -- z of the left channel, z of the right, then (y1_b, yL_b) for b = 0, 1, 2.
constexpr uint32_t kMbRun = 8;                    // frames per lane
constexpr uint32_t kMbTile = kMbRun * kThreads;   // frames per workgroup
constexpr uint32_t kMbBiquads = 9;
constexpr uint32_t kMbWords = 2 * kMbBiquads;     // state words of a channel
constexpr uint32_t kMbState = 2 * kMbWords + 6;   // doubles of the line
constexpr uint32_t kMbBlocks = 23;
struct MbPowers {
    double pw[8][kMbBlocks * 4];    // the blocks of A^(kMbRun 2^k): (p00, p01, p10, p11) each
    double a_tile[kMbBlocks * 4];   // ... of A^kMbTile
    double pwc[8][kMbBlocks * 4];   // ... of A^(kMbTile chunk 2^k)
};
struct MbDesc {
    const InTerm* ins;      // k input terms (kinds 0 .. 4), in connect() order
    float2* x;              // [frames] the summed input
    float2* out;
    double* line;           // carried across chunks / block pulls
    const double* init;     // the state entering tile 0: `line`, or nullptr when the vertex starts afresh
    const MbPowers* pow;
    double* agg;            // [36 n_tiles]
    double* carry;          // [36 n_tiles]
    double* dy[3];          // [frames] each: d_b, then y1_b (the bands' CompDesc::dy)
    double* agg1[3];        // [n_tiles] each (the bands' CompDesc::agg1)
    const double* carry2[3];   // [n_tiles] each (the bands' CompDesc::carry2)
    uint32_t k, term_mode, frames, n_tiles;
    uint32_t chunk;         // tiles per lane in k_mb_carry
    float wet;
    double co[5][5];        // (b0, b1, b2, a1, a2) of L1, H1, L2, H2, A2
    double thr[3], slope[3], makeup[3];   // T_b, 1 - 1 / R_b, M_b (dB)
    double knee;
    double aR, aA, oA;      // release / attack coefficients, 1 - aA
    double pwR[8], pwA[8];  // aR^(kMbRun 2^k), aA^(kMbRun 2^k)
    PanGain pg;
};

// A parametric EQ vertex (k_eq_local / k_eq_carry / k_eq_apply; the definition is in include/termdaw_amd.h at
// td_graph_add_eq): one RBJ biquad per channel in transposed direct form II, f64.  With z = (s1, s2) the recurrence is
// z[n] = A z[n-1] + c x[n],  A = [[-a1, 1], [-a2, 0]],  c = (b1 - a1 b0, b2 - a2 b0),  y[n] = b0 x[n] + s1[n-1]: an affine scan
// whose operator is a 2x2 matrix.  The compressor's tiling: tiles of kEqTile frames, a lane owns kEqRun consecutive frames.
// k_eq_local evaluates the input terms, leaves the summed input in `x` and each tile's zero-start end state (s1l, s2l, s1r,
// s2r) in agg[4 t ..]; k_eq_carry leaves the state entering each tile in carry[4 t ..] (tile 0: *init, or 0 when init is
// null); k_eq_apply rebuilds each lane's entry state from there and runs the definition serially.  A 2x2 matrix is stored
// row-major: {m00, m01, m10, m11}.  Every power is computed on the host in long double and rounded once.
constexpr uint32_t kEqRun = 8;                   // frames per lane
constexpr uint32_t kEqTile = kEqRun * kThreads;  // frames per workgroup
struct EqState { double s1l, s2l, s1r, s2r; };
struct EqDesc {
    const InTerm* ins;      // k input terms (kinds 0 .. 4), in connect() order
    float2* x;              // [frames] the summed input
    float2* out;
    EqState* state;         // carried across chunks / block pulls (k_eq_apply stores it)
    const EqState* init;    // the state entering tile 0 (k_eq_carry reads it): `state`, or nullptr after a set_time
    double* agg;            // [4 n_tiles]
    double* carry;          // [4 n_tiles]
    uint32_t k, term_mode, frames, n_tiles;
    uint32_t chunk;         // tiles per lane in k_eq_carry
    float wet;
    double b0, b1, b2, a1, a2;   // the normalised coefficients (td_eq_coefficients)
    double c0, c1;          // b1 - a1 b0, b2 - a2 b0
    double pw[8][4];        // A^(kEqRun 2^k)
    double a_tile[4];       // A^kEqTile
    double pwc[8][4];       // A^(kEqTile chunk 2^k)
    PanGain pg;
};

// A feedback delay vertex (k_delay_local / k_delay_carry / k_delay_apply; the definition is in
// include/termdaw_amd.h at td_graph_add_delay): u[n] = x[n] + G u[n - D], G = [[gs, gc], [gc, gs]] over (l, r) -- D independent
// first-order recurrences, one per residue of n mod D, each a constant 2x2 affine map: §3n's blocked scan with stride D.
// Lane j = chunk frame mod D, step k = chunk frame div D; a tile is T steps of every lane.  A chunk shorter than D has lanes
// = min(D, frames) of them, one step each.  One thread owns one lane of one tile: thread index = tile * lanes + j, so a step's loads and stores are contiguous across a wave.
// The line holds the last D values of (ul, ur), 16 D bytes; the vertex has run `pos` frames (mod D) since the line restarted, so
// lane j's word is line[2 ((pos + j) mod D)] and no other lane's -- a word below `filled` holds a value, the others read as 0
// (after a set_time filled = 0: nothing is read and nothing needs clearing).
// k_delay_local evaluates the input terms, leaves the summed input in `x` and each (tile, lane)'s zero-start end state in
// agg[2 (tile lanes + j) ..]; k_delay_carry leaves the state entering each tile in carry[..] (per lane: `seg` threads fold
// `chunk` consecutive tiles each, Hillis-Steele over them); k_delay_apply runs each thread's T steps from its entry state in
// the definition's order.  When one tile covers the chunk (n_tiles == 1) k_delay_apply runs alone, in an instantiation of its
// own (launch_delay_apply's `single`): the entry state is the line and the term loop runs inside it (x, agg, carry unused).  A 2x2 matrix is stored row-major; every power is computed on the
// host in long double and rounded once.
struct DelayDesc {
    const InTerm* ins;      // k input terms (kinds 0 .. 4), in connect() order
    float2* x;              // [frames] the summed input (three-launch form)
    float2* out;
    double* line;           // [2 D] carried across chunks / block pulls (k_delay_apply stores the words of the last D frames)
    double* agg;            // [2 n_tiles lanes]
    double* carry;          // [2 n_tiles lanes]
    uint32_t k, term_mode, frames, D;
    uint32_t lanes;         // min(D, frames)
    uint32_t T;             // steps per tile (even)
    uint32_t n_tiles;       // ceil(ceil(frames / D) / T)
    uint32_t pos, filled;   // the line's rotation and how many of its words hold a value
    uint32_t seg, chunk;    // k_delay_carry: threads per lane (a power of two <= kThreads), tiles per thread
    float wet;
    double gs, gc;          // feedback (1 - cross), feedback cross
    double g_tile[4];       // G^T
    double pwc[8][4];       // G^(T chunk 2^k)
    PanGain pg;
};

// A saturator vertex (k_sat_sum / k_sat<R> / k_sat1; the definition is in include/termdaw_amd.h at
// td_graph_add_saturator): polyphase up-sampling by R, a memoryless shaper at R x sr, a linear-phase decimator -- all in f64 on
// the f32 summed input, every output frame a pure function of the last 128 input frames.  One workgroup owns a tile of F output
// frames: the tile's raw x with 128 frames of halo in LDS, w for (F + 64) R oversampled samples in LDS as f64, phase-major
// (w[channel][phase][frame]), one barrier, then the decimation, the lerp against x delayed by 64 frames, pan / gain.
// The line holds the last 128 raw input frames in two halves of 128 float2, used alternately: a launch reads half `parity`
// (its first tile's halo; only the `filled` most recent frames hold values, the others read as 0) and its last tile writes half
// parity ^ 1, so no tile reads what another writes.  line[h][i] is the frame 128 - i back from the chunk's start.
// A chunk of at most kSatInlineFrames frames -- every block pull -- is ONE launch: k_sat in an instantiation of its own
// (launch_sat's `terms`) that runs the term loop itself over each tile and its halo; otherwise k_sat_sum leaves the summed input
// in `x` first and k_sat streams it.  R = 1 (k_sat1) has no
// filters, no line and no LDS: one launch with the term loop inside.
struct SatDesc {
    const InTerm* ins;      // k input terms (kinds 0 .. 4), in connect() order
    float2* x;              // [frames] the summed input (two-launch form; null in the one-launch form)
    float2* out;
    float2* line;           // [2][128] carried across chunks / block pulls (R > 1)
    const double* taps;     // [2 Z R + 1] the prototype h (R > 1); the up-sampler's R h is formed in the kernel (exact)
    uint32_t k, term_mode, frames;
    uint32_t F;             // output frames per tile (even, >= 128)
    uint32_t n_tiles;       // ceil(frames / F)
    uint32_t filled;        // min(frames the vertex has run since its line restarted, 128)
    uint32_t parity;        // the half of the line this launch reads
    uint32_t kind;          // TD_SAT_*
    float wet;
    double g_in, bias, fb, g_out;
    PanGain pg;
};

// A chorus vertex (k_chorus_sum / k_chorus; the definition is in include/termdaw_amd.h at td_graph_add_chorus):
// `voices` fractional delay lines per channel, each read by four-point Lagrange interpolation at the distance D0 + A lfo behind
// the output frame, the LFO a function of the graph's ABSOLUTE frame time -- all in f64 on the f32 summed input, every output
// frame a pure function of the last H input frames.  One lane per output frame, a workgroup owns a tile of F of them; every
// voice and both channels of a frame stay in the lane's registers.
// The line holds the last H raw input frames in two halves of H float2, used alternately: a launch reads half `parity` (only the
// `filled` most recent frames hold values, the others read as 0) and its last tile writes the last H frames of (old line ++
// chunk) to half parity ^ 1, so no tile reads a word another tile of the launch writes -- H may exceed the chunk.
// line[h][i] is the frame H - i back from the chunk's start.
// A chunk of at most kSatInlineFrames frames -- every block pull -- is ONE launch: k_chorus<true> runs the term loop itself over
// the part of the chunk its tile can reach, [max(t0 - H, 0), t0 + F), into LDS (at most 32 KB); otherwise k_chorus_sum leaves
// the summed input in `x` first and k_chorus<false> gathers from it with plain global loads.
struct ChorusDesc {
    const InTerm* ins;      // k input terms (kinds 0 .. 4), in connect() order
    float2* x;              // [frames] the summed input (two-launch form; null in the one-launch form)
    float2* out;
    float2* line;           // [2][H] carried across chunks / block pulls
    uint64_t t0;            // the graph's absolute frame time at the chunk's first frame (the LFO's n)
    uint32_t k, term_mode, frames;
    uint32_t F;             // output frames per tile (a multiple of kThreads)
    uint32_t n_tiles;       // ceil(frames / F)
    uint32_t H;             // frames per half of the line (a multiple of 64, >= floor(D0 + A) + 3)
    uint32_t filled;        // min(frames the vertex has run since its line restarted, H)
    uint32_t parity;        // the half of the line this launch reads
    uint32_t voices;        // 1 .. 4
    uint32_t shape;         // TD_CHORUS_*
    float wet;
    double D0, A, f;        // centre delay and depth in frames, LFO cycles per frame
    double stereo;          // the right channel's phase offset in cycles
    double inv_v;           // 1 / voices
    PanGain pg;
};

// A reverb vertex (k_reverb_sum / k_reverb; the definition is in include/termdaw_amd.h at td_graph_add_reverb):
// per channel 8 parallel damped feedback combs, then 4 series all-pass sections, all in f64 on the f32 summed input.
// ONE workgroup of kReverbThreads per vertex walks the chunk in windows of B frames, B <= the vertex' shortest line: inside a
// window every delayed read line[n - D] is history, so a comb is a first-order recurrence with the constant coefficient d1 over
// known data and the all-pass chain is elementwise.  Wave w owns comb w & 7 of channel w >> 3; a lane takes B / 64 consecutive
// frames.  The windows are serial, everything inside one is parallel.
// `state` is one block of doubles: f[16] (the combs' one-pole states, index = wave), then the 24 lines at off[i]; frame m of a line
// (m counted from the vertex' restart) lives in slot m mod D, read and then rewritten by the same lane in the same window.  The
// block is never cleared: a line's first `skip` frames of this chunk read as 0 (m - D < 0), and f reads as 0 when `fresh`.
// Lines are indexed 0 .. 7 left combs, 8 .. 15 right combs, 16 .. 19 left all-passes, 20 .. 23 right all-passes.
struct ReverbDesc {
    const InTerm* ins;      // k input terms (kinds 0 .. 4), in connect() order
    float2* x;              // [frames] the summed input (k_reverb_sum leaves it)
    float2* out;
    double* state;          // f[16], then the lines
    uint32_t k, term_mode, frames;
    uint32_t B;             // frames per window: 64 | 128 | 256, <= every len[]
    uint32_t fresh;         // 1: the vertex has not run since its restart -- f reads as 0
    float wet;
    uint32_t len[24];       // D: frames of each line
    uint32_t off[24];       // where each line starts in state[] (doubles)
    uint32_t pos[24];       // (frames run since the restart) mod D: the slot of the chunk's first frame
    uint32_t skip[24];      // the chunk's frames before this one read the line as 0: max(D - frames run since the restart, 0)
    double g, d1, d2, w1, w2;
    double pw[6];           // d1^((B / 64) 2^k): the wave scan's lane strides
    PanGain pg;
};
constexpr int kReverbThreads = 1024;   // 16 wave64: one per (comb, channel)

// sample_loop_gen (extensions.rs:331-341): out[m] = sample[(t0 + m) % len]
struct LoopDesc {
    const float2* sample;
    float2* out;
    uint64_t len;
    uint64_t t0;
    uint32_t magic;   // floor(2^32 / len) when the 32-bit form applies (len, t0 + frames < 2^32), else 0
    uint32_t pad[3];
    PanGain pg;
};

// sample_multi_gen (extensions.rs:344-381): hits in onset order; a voice with origin o sounds on frames
// [o, o + len) reading sample[m - o].  Origins are chunk-relative and may be negative (carried voices).
struct MultiHit { int64_t origin; float vel; float pad; };
struct MultiDesc {
    const float2* sample;
    float2* out;
    const MultiHit* hits;
    uint64_t len;
    uint32_t n_hits;
    uint32_t pad;
    PanGain pg;
    const uint32_t* tile_first;   // [tiles]: first hit that can still sound at the tile's first frame (origin > frame - len)
};

// sample_lerp_gen (extensions.rs:384-421).  key = frame from which the entry is `primary` (INT64_MIN for
// the two carried entries), origin = frame of sample position 0, fade = frame at which countdown was set
// to lerp_len.
struct LerpHit { int64_t key, origin, fade; float vel; float pad; };
struct LerpDesc {
    const float2* sample;
    float2* out;
    const LerpHit* hits;   // >= 2 entries; [0] = initial ghost, [1] = initial primary
    uint64_t len;
    uint32_t n_hits;
    uint32_t lerp_len;
    PanGain pg;
    const uint32_t* tile_first;   // [tiles]: number of entries with key <= the tile's first frame
};

// Interval tables for the voice-list vertices: the chunk is cut at block starts and event frames into
// intervals inside which the voice list is constant.  istart[i] = first frame (chunk-relative),
// ivoff[i]..ivoff[i+1] = voice records.
struct IntervalTab {
    const uint32_t* istart;
    const uint32_t* ivoff;
    const float4* voices;
    const uint32_t* tile_first;   // [tiles] index of the interval holding each 1024-frame tile's first frame
    uint32_t n_int;
    uint32_t pad;
    // [tiles] a permutation of the tiles, the costliest first (compile.cpp put_intervals: a tile costs a pass of the voice loop per
    // interval it holds frames of, each as long as the interval has voices): the expensive ones start at the head of the launch,
    // the grid's last workgroups are the cheap ones.  (Round 3: the tiles with an interval start inside them first, k_synth
    // 0.198 -> 0.14 ms on BASELINE config 3; round 6: by cost.)  nullptr: identity.
    const uint32_t* tile_order;
};

struct OscConfD { float volume, param; AdsrConfD adsr; };

// debug_sine_gen (extensions.rs:423-457): voice = (hz, vel, -, -)
struct SineDesc {
    IntervalTab tab;
    float2* out;
    uint64_t t0;   // graph time of the chunk's first frame
    uint32_t sr;
    uint32_t exact_sin;   // 1: glibc's sinf, operation for operation (SynthDesc::exact_sin)
    PanGain pg;
};

// synth_gen (extensions.rs:460-529): voice = (hz, vel, env_t at block start, rel_t)
struct SynthDesc {
    IntervalTab tab;
    float2* out;
    uint64_t t0;
    uint32_t sr, bl;
    OscConfD square, topflat, triangle;
    float osc_amp_multiplier;
    // envelope sharing: 1 / 2 = this oscillator's AdsrConf is bit-identical to the square's / topflat's (and that
    // one is enabled), so its envelope value -- a pure function of the conf and the voice's clocks -- is reused
    uint32_t tf_env_src, tr_env_src;
    PanGain pg;
    // 1: the interval table is cut at every envelope breakpoint and a voice is FOUR float4 -- (hz, env_t, 0, 0) and, per
    // oscillator (square, top-flat, triangle), (s1, s2, A, B): envelope x velocity x volume x osc_amp_multiplier x shape scale
    // = A + B ((t - s1) - s2), t = env_t + in-block offset (engine.cpp synth_refine_affine); 0: one float4 (hz, vel, env_t,
    // rel_t) per voice, envelopes evaluated per frame (confs that can reach the `res <= -1.0` escape, zero-length pieces)
    uint32_t affine;
    uint32_t exact_sin;   // 1: the oscillators' sine is glibc's sinf, operation for operation (kernels.hip sin_glibc; engine option "sine_mode"); affine is 0 then    // 1 (host: compile.cpp synth_desc_of): every sine argument of the chunk, (t0 + m) / sr * hz * 2 pi over the tables' largest hz,
    // stays below 2e6 rad -- the affine form's sine then rounds to half turns by adding 1.5 * 2^23 and takes a degree-9 polynomial
    // fitted to the reduced range that bound leaves (sin_small2); beyond: sin_any2
    uint32_t small_args, pad_sa;
};

// sampsyn_gen (extensions.rs:532-578) with this engine's own wavetable oscillator (the sampsyn crate is
// un-vendored; DESIGN.md "Wavetable voice"): voice = (hz, vel, env_t at block start, rel_t)
struct WaveTableD {
    const float4* quads;    // [n_frames][frame_len] of {w[f][i], w[f][i+1 wrapped], w[f+1 clamped][i], w[f+1 clamped][i+1 wrapped]}
    uint32_t n_frames, frame_len;
    float table_seconds;
    uint32_t pad;
};
struct SampsynDesc {
    IntervalTab tab;
    float2* out;
    WaveTableD wt;
    uint32_t sr, bl;
    AdsrConfD adsr;
    float amp_multiplier;
    PanGain pg;
};

// adsr_gen (extensions.rs:593-651): two voice records per interval: primary, ghost = (t_off, vel,
// release_val, skip) -- skip != 0 on the primary record marks a frame the reference leaves untouched
// (the `continue` at extensions.rs:632-635).
struct AdsrVDesc {
    IntervalTab tab;
    const InTerm* ins;
    float2* out;
    uint32_t k;
    uint32_t sr, bl;
    uint32_t use_off, use_max, term_mode;
    float wet;
    AdsrConfD conf;
    PanGain pg;
    // for the run form of the envelope (adsr_run, kernels.hip): 1.0 / (double)x of attack_sec, decay_sec, sustain_sec,
    // release_sec and of (float)sr -- (float)((double)n * rcp) is the IEEE f32 quotient n / x -- and whether every level an
    // attack / decay / sustain piece can return stays above the `res <= -1.0` escape of adsr.rs:62-69,75-86
    double rcp[5];
    uint32_t tame, pad2;
    // the vertex' gain per frame of the chunk (>= frames + 1 floats): written by k_adsr_env, read by consumers of a kind-5 term
    float* env;
    // ... and its mean square over every 512 frames ([ceil(frames / 512)], behind the gains in the same buffer): what the
    // guarded chain launch multiplies its estimate by where the vertex is a link (two scalar loads per stage)
    float* env_tile;
};
void adsr_fill_run_consts(AdsrVDesc* d);   // host: rcp[], tame from conf / sr
void launch_adsr_env(const AdsrVDesc* d, int n_desc, uint32_t frames, hipStream_t s);

// band_pass_gen (extensions.rs:654-689), exact sequential form.
struct BandState { float lprevl, lprevr, hprevl, hprevr; uint32_t first; uint32_t pad[3]; };
struct BandDesc {
    const InTerm* ins;
    float2* out;
    BandState* state;   // carried across chunks
    uint32_t k;
    uint32_t term_mode;
    uint32_t pass;
    float lgamma, hgamma;
    PanGain pg;
    // set_time since the vertex last ran (extensions.rs:196-204 sets BandPass.first): the kernel treats the state's `first`
    // word as set whatever the device copy says -- a descriptor bit instead of a fill kernel per set_time
    uint32_t first_override, pad_fo;
};

// band_pass_gen, exact AND parallel: speculative segments.
//   The recurrence y += gamma * (x - y) is a contraction: two trajectories fed the same input collapse onto
//   each other and, once bit-identical, stay identical.  The chunk is cut into segments of S frames; a
//   quad of lanes (low L, low R, high L, high R) runs each segment after a warm-up of W frames started from
//   a guess, records the state it entered the segment with and the state it left with, and writes the
//   segment's output.  k_band_fix then checks, bit for bit, that every segment entered with exactly the
//   state its predecessor left with -- by induction from the exactly-known first segment this proves the
//   whole output exact -- and recomputes (only) segments where the check fails, keeping seg_start honest
//   (= the entry state the stored output was computed from) so that the check can simply be repeated.  The usual failures are
//   constant or silent input stretches, where f32 trajectories park on different sticky points: there the
//   true state is a fixed point, so k_band_fix skips the whole stretch in one step and leaves its output
//   (state fixed, input known) to the parallel fill at the end of the launch (band_fill_tiles).
struct BandJob { uint32_t begin, end; float y[4]; uint32_t pad[2]; };   // frames [begin, end) with parked state y
struct BandSpecDesc {
    const float2* x;        // summed input of the vertex, materialised (sum_inputs, no epilogue)
    const float2* xq4;      // the same frames, planar within 4-frame blocks (SumDesc::out_q4)
    float2* out;
    BandState* state;       // carried across chunks
    float* seg_start;       // [nseg][4] state on entry (after warm-up)
    float* seg_final;       // [nseg][4] state on exit
    const float* blk_peaks; // [ceil(frames / 256)] per 256-frame block: input peak, or -1 if bit-constant (k_sum mode 2)
    uint32_t* seg_flags;    // [nseg] bit0: input bit-identical over the whole segment, bit1: input all (+-)0
    float2* seg_x0;         // [nseg] first input frame of the segment
    BandJob* jobs;          // [nseg] parked stretches found by k_band_fix's cascades, executed by its fill phase
    uint32_t* seg_job;      // [nseg] index of the job whose stretch covers (part of) the segment, or ~0
    uint32_t* stats;        // [8]: cascades repaired, segments recomputed, segments parked, jobs, ticket (zeroed by k_band_spec)
    uint32_t nseg, S, W;
    uint32_t Ws;            // short warm-up (k_band_spec picks W or Ws per segment from blk_peaks)
    float live_thr;         // (energy left from before the short window) / (energy fed in inside it) below which Ws is enough
    float gmin;             // the smaller non-zero gamma of the two smoothers
    float decay1, decay4;   // e^(-gamma_min * 256), and its 4th power: decay of a state over one / four 256-frame blocks
    uint32_t post_blocks;   // blocks right before the segment that must not be held constants (~20 / gamma frames)
    uint32_t pass;
    uint32_t first_override;   // see BandDesc
    float lgamma, hgamma;
    PanGain pg;
    // warm-up guess from the block responses (BandRespParam): state at a block boundary = Horner over the last K blocks
    const double* resp;     // nullptr: no guess (the warm-up starts from the input frame itself and takes Ws)
    double Al, Ah;          // (1 - gamma)^256 of the low / high smoother
    uint32_t Kl, Kh;        // blocks after which A^K is negligible
    uint32_t Wq;            // quick warm-up, taken when the energy from before it is below quick_thr x the energy inside it
    uint32_t Wq2;           // medium warm-up, taken when the window is merely alive (no parked stretch); then Ws, then W
    float quick_thr;
    uint32_t pad2[3];
};

// band_pass_gen, TOLERANCE class (engine option "band_mode" 1; <= 1e-6 RMS against the exact forms above): the four
// one-pole recurrences  y <- y + gamma (x - y)  =  (1 - gamma) y + gamma x  as a blocked affine scan, ONE launch per
// vertex -- or per CHAIN of band-pass vertices -- that also evaluates the first vertex' input terms (no materialised
// input sum).
//   A workgroup owns a tile of NF * 256 consecutive frames, a lane NF consecutive frames.  Per lane the zero-state
//   response b of its run (double), a wave / workgroup scan of the (a^NF, b) pairs gives the tile's response B, which
//   is published as eight 8-byte {tag, value} granules (agent-scope atomic stores).  The state entering the tile is
//   the Horner chain  C = sum_j a_tile^(j-1) B_(tile-j)  over the K preceding tiles (a_tile^K <= e^-depth: what is
//   dropped is below the f32 denormal floor), read back with agent-scope atomic loads; then every lane starts from its
//   exact-arithmetic entry state rounded to f32 and runs the REFERENCE's expression over its NF frames, so what
//   differs from the exact kernels is only the entry state's last bits (the f32 trajectory's own accumulated rounding).
//   Tiles are numbered by a ticket drawn at start: a workgroup only ever waits for LOWER tickets, whose holders are
//   running -- nothing depends on the order workgroups are dispatched in or on how many are resident at once.
//   One vertex (n_stages 1): the look-back's wait is bounded all the same -- a predecessor that has not published in
//   time is recomputed by the waiting workgroup itself, same arithmetic, same values.
//   A chain (n_stages > 1: `pass` band-pass vertices linked by single-input, single-consumer gain / pan stages and Adsr
//   vertices -- the shape of BASELINE config 4's 252 effect stages; k_band_chain): the frames stay in registers from
//   stage to stage, the links (`0.0 + x`, envelope gain, pan / gain: BandPost) are applied in between, and every stage
//   has its own granules.  Nobody can recompute a predecessor's stage s > 0, so tiles are numbered by a ticket drawn at
//   start (one only ever waits for lower tickets, whose holders are running), and waits are unbounded.
constexpr uint32_t kScanMaxK = 128;   // look-back depth limit (tiles); slower smoothers take the exact kernels
constexpr uint32_t kScanMaxStages = 128;   // band-pass vertices per launch (the engine cuts longer chains)
struct BandPost {               // one link between two band-pass vertices of a chain
    const float* env;           // an Adsr vertex (its gain buffer, AdsrVDesc::env), or nullptr: a single-input Sum (gain / pan stage)
    PanGain pg;                 // the link vertex' own pan / gain
    uint32_t pad[2];
};
struct BandStageDesc {          // one band-pass vertex
    BandState* state;           // carried across chunks (same slot the exact kernels use)
    unsigned long long* sync;   // [n_tiles][8] granules, zeroed before the launch: chain c's B as (lo, hi) halves of the double
    const double* pw;           // [2][64]: (1 - gamma)^(NF * lane), low / high smoother
    double ap[2][6];            // (1 - gamma)^(NF * 2^s), s = 0..5: the wave scan's step factors
    double aw[2];               // (1 - gamma)^(NF * 64): one wave
    double at[2];               // (1 - gamma)^(NF * 256): one tile
    float lgamma, hgamma;
    uint32_t pass;
    uint32_t K;                 // look-back depth in tiles (1 .. kScanMaxK)
    PanGain pg;                 // the vertex' own epilogue
    // what lies between this vertex' output and the next stage's input, in graph order (unused by the last stage);
    // each link first does its own sum_inputs `0.0 + x`, and so does the next band-pass vertex
    uint32_t n_post, first_override;   // first_override: see BandDesc
    BandPost post[3];
    // k_band_chain (a chain's launch; `pass` vertices only)
    float pn[16][2];            // (1 - gamma)^(n + 1), n = 0 .. NF - 1, {low, high} smoother: what an entry state still weighs after n + 1 frames
    const double* pk;           // [2][kScanMaxK]: (1 - gamma)^(NF * 256 * j): the weight of the tile j + 1 tiles back
    uint32_t Kw, pad3;          // (= K)
    // k_band_chain, guarded form (engine option "band_mode" 2, BandScanDesc::noise): what this vertex adds to the launch's
    // estimate of its own deviation from the reference's f32 trajectory (DESIGN.md 3e "The guard"), {low, high} smoother, every
    // coefficient already multiplied by the STATIC gain G between this vertex' recurrence and the launch's last stage (own pan /
    // gain, the links', every later vertex' -- largest channel amplitude; envelope links multiply in per lane in the kernel) --
    // nzv: G^2 0.25 K0 / (gamma (2 - gamma)), the variance a unit-level state picks up from independent roundings of the
    // recurrence's sum, seen through the 0.5 of `cut`; nzs: G 0.5 2^-24 / gamma, the offset at which an f32 state of unit
    // level parks short of a (nearly) constant input; nzk: 4 * 2^-23 / gamma -- the state counts as parked while
    // |x - y| < nzk |y| (|gamma (x - y)| below 4 ulp(y)); nzk[1] = 0: the faster smoother's test is skipped (both see the same
    // input: when the slower one is parked so is the faster, at a level equal and an offset smaller by gamma_low / gamma_high)
    float nzv[2], nzs[2];
    float nzk[2];
    const float* envt;          // the envelope link behind this vertex, if any: AdsrVDesc::env_tile (at most one Adsr vertex per hop)
};
struct BandScanDesc {
    const InTerm* ins;          // the (first) vertex' input terms, in connect() order
    float2* out;                // the (last) vertex' output
    const BandStageDesc* stages;
    uint32_t* ticket;           // {tile counter, "tile 0 has read the carried states"}, zeroed before the launch
    uint32_t n_stages;
    uint32_t k, term_mode, n_tiles;
    uint32_t flags;             // bit 0: (tests) every poll times out at once -> all predecessors recomputed (n_stages 1)
    uint32_t pad;
    // k_band_chain: a Normalize vertex whose one input is the chain's last vertex (through that stage's `post` links) is
    // evaluated by the launch itself, fresh-render form (SumDesc mode 5 fields: state, init, peaks, init_copy, sync with one
    // granule per tile, pg, out / pcm / qmode / amplitude); the host has checked block length == 1 024 frames = one wave-tile
    const SumDesc* norm;
    // k_band_chain: the first vertex' one input is a Sum vertex evaluated right here -- `ins` / `k` / `term_mode` are THAT
    // vertex' terms, `pre` its pan / gain, `pre2` those of a gain / pan stage between it and the band-pass vertex (flags 0:
    // nothing to apply -- no such vertex, or one without pan and gain)
    PanGain pre, pre2;
    // [n_tiles] granules, zeroed before the launch -- the first stage at which a tile's state went non-finite
    // (n_stages: never).  The reference's state stays NaN for good once it is; the look-back forgets a tile after K tiles,
    // so every tile learns at the end of the chain whether ANY earlier tile was poisoned and turns NaN itself if so
    unsigned long long* poison;
    // k_band_chain: [n_tiles] granules, zeroed before the launch -- the first frame of the chunk (or 0xFFFFFFFF: none) at which
    // the chain's RIGHT input is not finite (tile 0: frame 0 when a carried right smoother state is not).  A `pass` vertex'
    // right output is cutr * 0 + (r - cutl) * 1 (extensions.rs:682-687): its right smoothers, which this kernel does not
    // run, reach the output in exactly one way -- once non-finite (an infinite or NaN right input frame makes them so, for
    // good) they turn it NaN.  Every tile publishes this at its start and reads all earlier tiles' at its end.
    unsigned long long* rpoison;
    // Guarded form (band_mode 2) -- k_band_chain: [ceil(frames / 1024)], per wave-tile; k_band_scan (a single vertex, `cut`
    // vertices included): [n_tiles], per workgroup tile -- the estimated ENERGY (sum over its frames of variance + offset^2) of
    // the launch's deviation from the reference at the launch's output (behind the fused Normalize vertex where there is
    // one); nullptr: not guarded (band_mode 1).  Read by k_band_audit at the end of the submission.
    float* noise;
    float nz_end;               // the static gain behind the last stage that the kernel applies itself (fused Normalize vertex' pan / gain)
    // ... or, where this launch is the graph's ONLY guarded one and carries the Normalize vertex itself, the verdict right
    // here, without k_band_audit: every tile leaves its energy as one granule, the tile with the last ticket gathers them,
    // compares  sum x nz_scale (= (static gain to the output)^2 / frames)  with nz_thr2 and writes the host words
    float nz_scale;
    unsigned long long* nz_sync;   // [n_tiles] granules, zeroed before the launch; nullptr: leave the wave-tiles' energies in `noise`
    uint32_t* nz_host;          // AuditHead::host_word
    float nz_thr2, pad5;
    // ... and with it what the graph's probed sine vertices measured (ProbeDesc::noise; engine option "sine_mode" 2), where every
    // one of them reaches the output through this launch's Normalize vertex: per sample frame the energy of the vertex' deviation
    // at its own output, nz_xcnt (<= 64) samples per wave-tile; nz_xg2 = (its static gain to the Normalize vertex' INPUT)^2.
    // The tile adds its own samples through its own 1 / max, like its own estimate.  nullptr: none.
    const float* nz_extra[2];
    float nz_xg2[2];
    uint32_t nz_xcnt, pad6;
    // ... measured BY THIS LAUNCH (round 6): with one probed vertex and a sample every 256 frames a tile's 4 096 frames hold sixteen
    // sample frames -- one workgroup of k_sine_probe's -- and the tile evaluates them itself, right behind its ticket (the probed
    // vertex' output is complete: it was written by an earlier launch), keeps the sixteen energies in LDS and adds them to its
    // verdict: no k_sine_probe launch (10 us of BASELINE config 3's 114).  nz_extra[0] is nullptr then; nz_xg2[0] as above.
    const struct ProbeDesc* nz_probe;
};
// The guard's verdict (engine option "band_mode" 2): one workgroup per graph adds up what its scan launches estimated, carried to
// the graph's output -- a static gain per launch (the host walks the graph: pan / gain of everything downstream) and, where the
// path runs through ONE Normalize vertex that the launch has not evaluated itself, that vertex' running maximum per block
// (its peak table and carried max, as k_scale / k_norm_fix read them) -- and raises a word in page-locked host memory when
// the estimated RMS deviation exceeds the bound: the engine then renders the graph again with the exact kernels.
struct AuditDesc {
    const float* noise;         // a launch's per-wave-tile energies
    const float* peaks;         // the Normalize vertex on the way to the output: [nb] block peaks (nullptr: none, or evaluated by the launch)
    const float* init_copy;     // ... its carried max at the chunk start
    uint32_t n_wt, nb, bl;      // entries of `noise`; the Normalize vertex' blocks and block length
    uint32_t tile_frames;       // frames per entry of `noise`: 1 024 (k_band_chain: a wave-tile) or NF x 256 (k_band_scan: a workgroup tile)
    float gain;                 // static gain from the launch's output to the graph's
    uint32_t sampled;           // 1: the entries are k_sine_probe's samples (ProbeDesc::noise) -- entry w was measured AT frame probe_frame(w, log2 tile_frames), whose block's running max it goes through
    uint32_t pad2[2];
};
struct AuditHead {              // one graph of the submission
    const AuditDesc* descs;
    uint32_t n, frames;
    float thr2;                 // (bound on the RMS)^2
    uint32_t pad;
    uint32_t* host_word;        // page-locked host memory (device address): [0] raised when over the bound, [1] the estimate (f32 bits)
};
void launch_band_audit(const AuditHead* heads, int n_heads, hipStream_t s);

// The sine kinds' guard (engine option "sine_mode" 2 -- the front-end's default).  The fast forms of debug_sine /
// synth (sin_any, affine envelopes, folded products) differ from the reference's own arithmetic by a white, signal-sized
// rounding noise that a graph can amplify without bound (43 dB of cancellation in a `cut` band-pass, then a Normalize vertex).
// Nothing models that noise: k_sine_probe MEASURES it.  Behind the vertex' launch, on a sample of the chunk's frames -- one in
// every 1 << stride_log2, at an offset that walks all residues -- it evaluates the frame the reference's way (synth_frame /
// sine_frame with exact_sin: glibc's sinf, adsr.rs's divisions, the reference's order of products -- what "sine_mode" 1 renders)
// and takes the squared distance to what the fast launch left in the vertex' buffer (pan / gain applied on both sides; the
// larger channel).  noise[i] = that x the frames the sample stands for: an energy in the audit's own units (AuditDesc::noise
// with tile_frames = the stride), carried to the output by k_band_audit -- or by the chain launch's own verdict -- like a scan
// launch's estimate: static gain, the Normalize vertex' running 1 / max AT THE SAMPLE'S OWN BLOCK.  A NaN on one side only
// counts as an infinite energy.
// sample i of a chunk probed with stride 1 << lg: one frame inside [i << lg, (i + 1) << lg), at an offset that walks all residues
// (block starts, in-block envelope clocks and event frames are not favoured)
#if defined(__HIPCC__)
__host__ __device__
#endif
inline uint32_t probe_frame(uint32_t i, uint32_t lg) { return (i << lg) + (((i & 63u) * 37u + (i >> 6) * 11u) & ((1u << lg) - 1u)); }
struct ProbeDesc {
    SynthDesc syn;              // kind 1: the vertex' descriptor with exact_sin = 1, affine = 0 and the RAW interval tables
    SineDesc sine;              // kind 0: ... with exact_sin = 1
    uint32_t kind;
    uint32_t stride_log2;       // one sample per 1 << stride_log2 frames (4 .. 8: short chunks are sampled densely)
    uint32_t n_groups, pad;     // workgroups: 16 samples each
    float* noise;               // [ceil(frames >> stride_log2)], one entry per sample
    const uint32_t* ranges;     // [2 x samples] host-made: the voice records {first, one past the last} of the sample frame's interval
};
void launch_sine_probe(const ProbeDesc* d, int n_desc, uint32_t frames, uint32_t n_groups, hipStream_t s);
void launch_band_scan(const BandScanDesc* d, int n_desc, uint32_t frames, uint32_t term_mode, int nf, hipStream_t s);
int band_scan_resident_capacity(int nf);   // workgroups of k_band_scan resident at once (0: unknown)
void launch_band_chain(const BandScanDesc* d, int n_desc, uint32_t frames, uint32_t term_mode, bool guarded, hipStream_t s);   // NF 16; guarded: every descriptor has `noise`
inline uint32_t band_scan_tile_frames(int nf) { return (uint32_t)nf * (uint32_t)kThreads; }

// ---- build-defined sinc resampler (stands in for the un-vendored rubato crate; DESIGN.md "Resampler") ----
// Shaped like the streaming SincFixedIn the reference drives block by block (state.rs:545-560): output j sits at input
// position j * from / to - sinc_len / 2 (the resampler's documented output delay: the filter only ever looks at frames it
// has already been handed, history before the first frame is zeros), it is complete -- and in a block-by-block run
// emitted -- as soon as input frame floor(j * from / to) has arrived, and nothing is flushed at the end, like the
// reference: ceil(len * to / from) outputs.  One launch over the whole timeline computes exactly what the block-by-block
// run with carried history would (an FIR has no other state).
constexpr int kSincLen = 256, kSincOver = 256;
struct ResampleDesc {
    const float2* in;
    float2* out;
    const float* table;   // [(kSincOver + 1) * kSincLen], built on the host in f64 and rounded once
    uint64_t len, nout, from, to;
};
void launch_resample(const ResampleDesc& d, hipStream_t s);

// ---- sample load pipeline (SampleBank::add, sample.rs:262-303) on the device ----
// raw PCM words -> f32 exactly like hound + `as f32` (sample.rs:264-273): ints are NOT scaled.
enum PcmFormat : uint32_t { PCM_F32 = 0, PCM_U8 = 1, PCM_S16 = 2, PCM_S24 = 3, PCM_S32 = 4 };
void launch_pcm_decode(const uint8_t* raw, float* linear, uint32_t n_values, uint32_t format, hipStream_t s);
// de-interleave by load mode into planar l / r (lengths nl, nr): src_l / src_r pick the source channel of
// the interleaved stream (channel index, stride = channels), per Sample::from (sample.rs:38-77)
void launch_sample_split(const float* linear, uint32_t channels, uint32_t src_l, uint32_t src_r, float* l, float* r,
                         uint32_t nl, uint32_t nr, hipStream_t s);
void launch_absmax(const float* v, uint32_t n, float* out, hipStream_t s);             // absmax (sample.rs:8-14)
void launch_abs_sum_serial(const float* v, uint32_t n, float* out, hipStream_t s);     // mean_energy's f32 sum, in order
void launch_add_planar(const float* a, const float* b, float* out, uint32_t n, hipStream_t s);   // mix_down sum
// frames[i] = {l[i] * scale_l, r[i] * scale_r} with scale = 1.0f / *max (normalize / normalize_seperate / mix_down)
void launch_sample_pack(const float* l, const float* r, const float* max_l, const float* max_r, float2* frames,
                        uint32_t n, hipStream_t s);
// packed 16-bit form of the same sample (un-scaled integer PCM values); *not_int16 is set when a value is
// not an integer in [-32768, 32767] (then the packed form is not usable)
void launch_sample_pack16(const float* l, const float* r, uint32_t* packed, uint32_t n, uint32_t* not_int16, hipStream_t s);

// per-project peak table of a batch: table[first + i * stride] = *src[i] for i < n_own, every other entry 0
void launch_peak_table(const float* const* src, float* table, uint32_t n_total, uint32_t n_own, uint32_t first, uint32_t stride,
                       hipStream_t s);

void launch_band_spec(const BandSpecDesc* d, int n_desc, uint32_t frames, uint32_t max_nseg, hipStream_t s);
void launch_band_fix(const BandSpecDesc* d, int n_desc, uint32_t frames, uint32_t max_nseg, hipStream_t s);
// every descriptor of one launch_sum call has the same term_mode (the engine groups them)
// k_norm1 (SumDesc mode 5 outside the wide all-loop sums): tiles per workgroup (1 | 2 | 4) with which the whole grid of a
// `frames`-long chunk is resident at once, 0 if none; and its launch
int norm1_tiles_per_workgroup(uint32_t term_mode, uint32_t frames);
void launch_norm1(const SumDesc* d, int n_desc, uint32_t frames, uint32_t term_mode, int tpw, uint32_t tag, hipStream_t s);   // tag: see launch_sum
// (nq 0: the ragged form k_sum16r; nq -1: the device's CU count)
int sum16w_resident_capacity(int nq, bool packed);
// The ragged form of the wide packed sum (k_sum16r; sum_partition.h): the workgroups of its grid for a timeline of `frames`, 0 where
// the form does not apply -- tdsp::pick_groups with this device's figures.  Automatic: kSumGroupsPerCU workgroups per CU where
// launch_sum would pick 16 frames per lane (from 2 600 tiles on).  compile.cpp decides with it, launch_sum gets the answer.
// kSumGroupsPerCU is 0 -- the automatic choice never takes the form: on config 2 it measured 75 / 79 us at 3 / 4 workgroups per CU
// against k_sum16w<4>'s 58 (docs/EXPERIMENTS.md 0000); the form is reached through debug.sum_groups, or through the tuning aid
// TD_SUM_WPC (workgroups per CU; read once per process like TD_FORCE_NQ, which turns the form off).
constexpr uint32_t kSumGroupsPerCU = 0;
inline uint32_t sum16r_groups(uint32_t frames, uint32_t forced, bool need_resident) {
    static const int env_wpc = getenv("TD_SUM_WPC") ? atoi(getenv("TD_SUM_WPC")) : -1;
    static const bool env_nq = getenv("TD_FORCE_NQ") && atoi(getenv("TD_FORCE_NQ")) != 0;
    const uint32_t wpc = env_nq ? 0u : (env_wpc >= 0 ? (uint32_t)env_wpc : kSumGroupsPerCU);
    return tdsp::pick_groups(frames, forced, need_resident, (uint32_t)std::max(0, sum16w_resident_capacity(0, true)),
                             (uint32_t)std::max(0, sum16w_resident_capacity(-1, true)), wpc, 2600u * 1024u);
}   // workgroups of k_sum16w<nq, packed> the device holds at once (0: unknown)
// must_wide: the descriptors hold a mode-4 / mode-5 Normalize, which only the k_sum16w forms implement (the engine sets it where they would run anyway)
// tag: what a tile word of a single-pass Normalize (SumDesc::sync, modes 4 / 5) carries beside its value -- 1 when the engine has
// zeroed the words before the launch, otherwise the submission's epoch (engine.cpp, submit_chunk)
// term_mode: the TermMode in bits 0 .. 7; bits 16 .. 31, if not 0: the ragged form k_sum16r with that many workgroups (the descriptors
// are plain Sums or mode-5 Normalizes with `peaks2`: compile.cpp)
void launch_sum(const SumDesc* d, int n_desc, uint32_t frames, uint32_t bl, uint32_t term_mode, bool wide_ok, bool must_wide, uint32_t tag, hipStream_t s);
void launch_scale(const ScaleDesc* d, int n_desc, uint32_t frames, uint32_t bl, int is_scan, hipStream_t s);
// second half of the speculative single-pass normalize: a no-op unless a block peak exceeded the carried max
void launch_norm_fix(const SumDesc* d, int n_desc, uint32_t frames, uint32_t bl, hipStream_t s);
void launch_quantise(const QuantDesc* d, int n_desc, uint32_t frames, hipStream_t s);
// Weak: the host engine calls it only when stems are set, and a host-only build of the engine (tests/mock_hip.cpp) has no
// definition -- the engine then refuses stems with an error instead of failing to link.
__attribute__((weak)) void launch_stems(const StemDesc* d, int n_desc, uint32_t frames, hipStream_t s);
// Weak for the same reason: every signal of a loudness measurement in ONE launch (grid.x: the largest tile count).
__attribute__((weak)) void launch_loudness(const LoudDesc* d, int n_desc, uint32_t max_tiles, hipStream_t s);
// Weak for the same reason: the mastering launches, every signal of a pass in ONE grid each (grid.x: the largest tile count;
// launch_master_carry: one workgroup per signal).
__attribute__((weak)) void launch_master_detect(const MasterDesc* d, int n_desc, uint32_t max_tiles, hipStream_t s);
__attribute__((weak)) void launch_master_scan(const MasterDesc* d, int n_desc, uint32_t max_tiles, hipStream_t s);
__attribute__((weak)) void launch_master_carry(const MasterDesc* d, int n_desc, hipStream_t s);
__attribute__((weak)) void launch_master_apply(const MasterDesc* d, int n_desc, uint32_t max_tiles, hipStream_t s);
// Weak for the same reason: a level's compressor vertices, ONE grid per step (grid.x: the largest tile count); the two carries
// between the steps are launch_master_carry's.
__attribute__((weak)) void launch_comp_detect(const CompDesc* d, int n_desc, uint32_t max_tiles, hipStream_t s);
__attribute__((weak)) void launch_comp_env(const CompDesc* d, int n_desc, uint32_t max_tiles, hipStream_t s);
__attribute__((weak)) void launch_comp_apply(const CompDesc* d, int n_desc, uint32_t max_tiles, hipStream_t s);
// ... and the keyed form of the first (CompDesc::key_ins; a launch whose aux carries kKeyedBit)
__attribute__((weak)) void launch_comp_detect_keyed(const CompDesc* d, int n_desc, uint32_t max_tiles, hipStream_t s);
// Weak for the same reason: a level's EQ vertices, ONE grid per step (grid.x: the largest tile count; the carry: one workgroup
// per vertex).
__attribute__((weak)) void launch_eq_local(const EqDesc* d, int n_desc, uint32_t max_tiles, hipStream_t s);
__attribute__((weak)) void launch_eq_carry(const EqDesc* d, int n_desc, hipStream_t s);
__attribute__((weak)) void launch_eq_apply(const EqDesc* d, int n_desc, uint32_t max_tiles, hipStream_t s);
// Weak for the same reason: a level's delay vertices (grid.x: the largest thread count in workgroups; the carry's: the largest
// lane count in workgroups of kThreads / seg lanes).  launch_delay_apply takes either the multi-tile vertices of a level or the
// single-tile ones (`single`), never both: kDelaySingleBit of a launch's aux says which.
constexpr uint32_t kDelaySingleBit = 0x80000000u;
__attribute__((weak)) void launch_delay_local(const DelayDesc* d, int n_desc, uint32_t max_groups, hipStream_t s);
__attribute__((weak)) void launch_delay_carry(const DelayDesc* d, int n_desc, uint32_t max_groups, hipStream_t s);
__attribute__((weak)) void launch_delay_apply(const DelayDesc* d, int n_desc, uint32_t max_groups, bool single, hipStream_t s);
// Weak for the same reason: a level's saturator vertices.  launch_sat_sum: grid.x from `frames`; launch_sat: the vertices of ONE
// oversampling factor R (2 | 4 | 8), grid.x = n_tiles, F output frames per tile (every descriptor's), `terms`: the instantiation
// with the term loop inside.  A launch's aux packs these: sat_aux().
constexpr uint32_t kSatTermsBit = 0x80000000u;
constexpr uint32_t kSatInlineFrames = 4096;   // chunks up to here take the one-launch form (the halo's terms are evaluated twice)
inline uint32_t sat_aux(uint32_t n_tiles, uint32_t F, uint32_t R, bool terms) {
    return n_tiles | ((F / 128u) << 20) | (R << 24) | (terms ? kSatTermsBit : 0u);
}
__attribute__((weak)) void launch_sat_sum(const SatDesc* d, int n_desc, uint32_t frames, hipStream_t s);
__attribute__((weak)) void launch_sat(const SatDesc* d, int n_desc, uint32_t R, uint32_t n_tiles, uint32_t F, bool terms, hipStream_t s);
__attribute__((weak)) void launch_sat1(const SatDesc* d, int n_desc, uint32_t frames, hipStream_t s);
// Weak for the same reason: a level's chorus vertices.  launch_chorus_sum: grid.x from `frames`; launch_chorus: grid.x = n_tiles
// (every descriptor's), `terms`: the instantiation with the term loop inside, whose LDS holds the chunk's `frames` frames.
constexpr uint32_t kChorusTermsBit = 0x80000000u;
inline uint32_t chorus_aux(uint32_t n_tiles, bool terms) { return n_tiles | (terms ? kChorusTermsBit : 0u); }
__attribute__((weak)) void launch_chorus_sum(const ChorusDesc* d, int n_desc, uint32_t frames, hipStream_t s);
__attribute__((weak)) void launch_chorus(const ChorusDesc* d, int n_desc, uint32_t n_tiles, uint32_t frames, bool terms, hipStream_t s);
// Weak for the same reason: a level's gate vertices, ONE grid per step (grid.x: the largest tile count); launch_gate_carry: one
// workgroup per vertex, the discrete carry or (affine) the fade's.
__attribute__((weak)) void launch_gate_detect(const GateDesc* d, int n_desc, uint32_t max_tiles, hipStream_t s);
__attribute__((weak)) void launch_gate_carry(const GateDesc* d, int n_desc, bool affine, hipStream_t s);
__attribute__((weak)) void launch_gate_env(const GateDesc* d, int n_desc, uint32_t max_tiles, hipStream_t s);
__attribute__((weak)) void launch_gate_apply(const GateDesc* d, int n_desc, uint32_t max_tiles, hipStream_t s);
// ... and the keyed forms of detect and env (GateDesc::key_ins / cls; launches whose aux carries kKeyedBit)
__attribute__((weak)) void launch_gate_detect_keyed(const GateDesc* d, int n_desc, uint32_t max_tiles, hipStream_t s);
__attribute__((weak)) void launch_gate_env_keyed(const GateDesc* d, int n_desc, uint32_t max_tiles, hipStream_t s);
// Weak for the same reason: a level's phaser vertices of ONE stage count (the kernels are templates on it), grid.x = n_tiles
// (every descriptor's; the carry: one workgroup per vertex).  A launch's aux packs tile count, stage count and, for
// launch_phaser_apply, `single`: the instantiation with the term loop inside, entered with the carried state.
constexpr uint32_t kPhaserSingleBit = 0x80000000u;
inline uint32_t phaser_aux(uint32_t n_tiles, uint32_t stages, bool single) { return n_tiles | (stages << 24) | (single ? kPhaserSingleBit : 0u); }
__attribute__((weak)) void launch_phaser_local(const PhaserDesc* d, int n_desc, uint32_t stages, uint32_t n_tiles, hipStream_t s);
__attribute__((weak)) void launch_phaser_carry(const PhaserDesc* d, int n_desc, uint32_t stages, hipStream_t s);
__attribute__((weak)) void launch_phaser_apply(const PhaserDesc* d, int n_desc, uint32_t stages, uint32_t n_tiles, bool single, hipStream_t s);
// Weak for the same reason: a level's vocoder vertices of ONE band count (the kernels are templates on it), grid.x = n_tiles
// (every descriptor's; the carries: one workgroup per band and vertex).  A launch's aux packs tile count, band count, for
// F_VOC_APPLY `single` (the instantiation with the term loops inside, entered with the line), and kKeyedBit where the descriptors
// are keyed: those go through the *_keyed entry points only.
constexpr uint32_t kVocSingleBit = 0x40000000u;
inline uint32_t voc_aux(uint32_t n_tiles, uint32_t bands, bool single, bool keyed) {
    return n_tiles | (bands << 24) | (single ? kVocSingleBit : 0u) | (keyed ? kKeyedBit : 0u);
}
inline uint32_t voc_aux_tiles(uint32_t aux) { return aux & 0xFFFFFFu; }
inline uint32_t voc_aux_bands(uint32_t aux) { return (aux >> 24) & 31u; }
__attribute__((weak)) void launch_voc_local(const VocDesc* d, int n_desc, uint32_t bands, uint32_t n_tiles, hipStream_t s);
__attribute__((weak)) void launch_voc_local_keyed(const VocDesc* d, int n_desc, uint32_t bands, uint32_t n_tiles, hipStream_t s);
__attribute__((weak)) void launch_voc_carry(const VocDesc* d, int n_desc, uint32_t bands, bool env, hipStream_t s);
__attribute__((weak)) void launch_voc_env(const VocDesc* d, int n_desc, uint32_t bands, uint32_t n_tiles, hipStream_t s);
__attribute__((weak)) void launch_voc_apply(const VocDesc* d, int n_desc, uint32_t bands, uint32_t n_tiles, bool single, hipStream_t s);
// (single and keyed: the one-launch form of a keyed vertex, with both term loops inside)
__attribute__((weak)) void launch_voc_apply_keyed(const VocDesc* d, int n_desc, uint32_t bands, uint32_t n_tiles, hipStream_t s);
// Weak for the same reason: a level's filter vertices, grid.x = n_tiles (every descriptor's; the carry: one workgroup per vertex).
// A launch's aux packs the tile count, for F_FILT_APPLY `single` (the one-launch form, entered with the carried state), and
// kKeyedBit where the descriptors are keyed (F_FILT_DETECT, and F_FILT_APPLY when single).  The follower's two carries are
// launch_master_carry's, over MasterDesc.
constexpr uint32_t kFiltSingleBit = 0x40000000u;
inline uint32_t filt_aux(uint32_t n_tiles, bool single, bool keyed) { return n_tiles | (single ? kFiltSingleBit : 0u) | (keyed ? kKeyedBit : 0u); }
inline uint32_t filt_aux_tiles(uint32_t aux) { return aux & 0xFFFFFFu; }
__attribute__((weak)) void launch_filt_detect(const FiltDesc* d, int n_desc, uint32_t n_tiles, bool keyed, hipStream_t s);
__attribute__((weak)) void launch_filt_env(const FiltDesc* d, int n_desc, uint32_t n_tiles, hipStream_t s);
__attribute__((weak)) void launch_filt_local(const FiltDesc* d, int n_desc, uint32_t n_tiles, hipStream_t s);
__attribute__((weak)) void launch_filt_carry(const FiltDesc* d, int n_desc, hipStream_t s);
__attribute__((weak)) void launch_filt_apply(const FiltDesc* d, int n_desc, uint32_t n_tiles, bool single, bool keyed, hipStream_t s);
// Weak for the same reason: a level's limiter vertices, grid.x = n_tiles (every descriptor's).  F_LIM_APPLY's aux packs the tile
// count and `single` (the one-launch form of a one-tile chunk: term loop, detector, release and window mean inside).  The carry in
// between is launch_master_carry's, over MasterDesc.
constexpr uint32_t kLimSingleBit = 0x40000000u;
inline uint32_t lim_aux(uint32_t n_tiles, bool single) { return n_tiles | (single ? kLimSingleBit : 0u); }
inline uint32_t lim_aux_tiles(uint32_t aux) { return aux & 0xFFFFFFu; }
__attribute__((weak)) void launch_lim_detect(const LimDesc* d, int n_desc, uint32_t n_tiles, hipStream_t s);
__attribute__((weak)) void launch_lim_apply(const LimDesc* d, int n_desc, uint32_t n_tiles, bool single, hipStream_t s);
// Weak for the same reason: a level's multiband vertices, grid.x = n_tiles (every descriptor's; launch_mb_carry: one workgroup per
// channel and vertex).  F_MB_APPLY's aux packs the tile count and `single` (the one-launch form of a one-tile chunk).  The two
// scalar carries are launch_master_carry's over MasterDesc, the launch between them launch_comp_env's over CompDesc.
constexpr uint32_t kMbSingleBit = 0x40000000u;
inline uint32_t mb_aux(uint32_t n_tiles, bool single) { return n_tiles | (single ? kMbSingleBit : 0u); }
inline uint32_t mb_aux_tiles(uint32_t aux) { return aux & 0xFFFFFFu; }
__attribute__((weak)) void launch_mb_local(const MbDesc* d, int n_desc, uint32_t n_tiles, hipStream_t s);
__attribute__((weak)) void launch_mb_carry(const MbDesc* d, int n_desc, hipStream_t s);
__attribute__((weak)) void launch_mb_detect(const MbDesc* d, int n_desc, uint32_t n_tiles, hipStream_t s);
__attribute__((weak)) void launch_mb_apply(const MbDesc* d, int n_desc, uint32_t n_tiles, bool single, hipStream_t s);
// A convolution vertex (k_conv_ir / k_conv_fwd / k_conv_mac / k_conv_inv; the definition is in
// include/termdaw_amd.h at td_graph_add_convolution): an impulse response from the sample bank by uniform-partitioned
// overlap-save in f64.  The partition is kConvB frames, a transform kConvN = 2 kConvB complex points (32 KB of LDS); both
// channels ride one transform as z = l + i r, so with Z = FFT(z) and the real responses' spectra H_l, H_r a product is
//   Y[k] = Z[k] A[k] + conj(Z[N - k]) C[k],   A = (H_l + H_r) / 2,  C = (H_l - H_r) / 2,
// and since A[N - k] = conj A[k], C[N - k] = conj C[k] only the bins 0 .. N / 2 of A and C are kept (kConvBins per partition).
//   k_conv_ir (one workgroup per partition p; only when the spectra have to be built) transforms frames [p B, (p + 1) B) of
//   the effective response -- D zeros, then g h, g divided by sqrt(max_c sum h_c^2) when `norm` (every workgroup forms that sum
//   itself, in one fixed order) -- and stores A_p, C_p in `spec` behind a header of kConvHead doubles (word 0, 1: the two sums,
//   -1 without `norm`; word 2: the g used).
//   k_conv_fwd (one workgroup per window w = 0 .. n_tiles + P - 2) evaluates the input terms of chunk frames
//   [(j - 1) B, (j + 1) B), j = w - (P - 1), takes the frames in front of the chunk from the line's half `parity` (0 beyond
//   `hist` back, and all of them when `fresh`; a non-finite sample enters as 0), stores the raw sum of [j B, (j + 1) B) in
//   `x`, and leaves the window's spectrum in xs[w] (natural bin order).
//   k_conv_mac: ys[t][k] = sum over p = 0 .. P - 1, ascending, of the product above with Z = xs[t - p + P - 1]; a lane holds
//   one bin pair (k, N - k) of kConvTT consecutive tiles, so an (A_p, C_p) and a window's pair are read once for
//   2 kConvTT products.  No atomics.
//   k_conv_inv (one workgroup per tile, `hist_groups` more for the line) transforms ys[t] back, keeps the last B frames,
//   rounds once to f32, p = (float)(re / N), (float)(im / N), lerps against x with `wet`, pan, gain -> `out`; the extra
//   workgroups write the last `hist` frames of (old half ++ chunk) into the half parity ^ 1, whole.
// The transforms are radix 2 over a table of N / 2 twiddles (cos, -sin)(2 pi j / N) the host computes in long double: forward
// decimation in frequency, natural order in, bit-reversed out; inverse decimation in time, bit-reversed in, natural out.
constexpr uint32_t kConvB = 1024;                  // frames per partition
constexpr uint32_t kConvN = 2 * kConvB;            // complex points per transform
constexpr uint32_t kConvBins = kConvN / 2 + 1;     // bins of A and C kept per partition
constexpr uint32_t kConvTT = 4;                    // tiles per lane of k_conv_mac
constexpr uint32_t kConvMacGroups = (kConvBins + kThreads - 1) / kThreads;   // workgroups per kConvTT tiles
constexpr uint32_t kConvHead = 32;                 // doubles in front of the spectra
constexpr uint32_t kConvHistFrames = 8192;         // line frames per extra workgroup of k_conv_inv
constexpr uint32_t kConvHistGroups = 64;           // ... at most this many
struct ConvDesc {
    const InTerm* ins;      // k input terms (kinds 0 .. 4), in connect() order
    float2* x;              // [frames] the summed input
    float2* out;
    float2* line;           // the carried line: two halves of `hist` frames
    const float2* ir;       // the bank's sample: the response's frames
    double* spec;           // kConvHead doubles, then P x kConvBins x (A.re, A.im, C.re, C.im)
    const double* tw;       // kConvN / 2 twiddles (re, im)
    double* xs;             // [n_tiles + P - 1][kConvN] window spectra (re, im)
    double* ys;             // [n_tiles][kConvN] products
    uint32_t k, term_mode, frames, n_tiles;
    uint32_t P, Lh, D, hist;   // partitions; response frames; pre-delay frames; D + Lh - 1
    uint32_t parity;        // the half this chunk reads
    uint32_t fresh;         // 1: the frames in front of the chunk are all 0, the half is not read
    uint32_t norm, hist_groups;
    float wet;
    uint32_t pad;
    double g;               // 10^(out_db / 20)
    PanGain pg;
};
// Weak for the same reason: a level's convolution vertices.  The second argument behind the count is grid.x, the largest of the
// launch's descriptors (a workgroup beyond its own descriptor's range returns): partitions, windows, kConvMacGroups x tile
// groups, tiles + hist_groups.
__attribute__((weak)) void launch_conv_ir(const ConvDesc* d, int n_desc, uint32_t grid_x, hipStream_t s);
__attribute__((weak)) void launch_conv_fwd(const ConvDesc* d, int n_desc, uint32_t grid_x, hipStream_t s);
__attribute__((weak)) void launch_conv_mac(const ConvDesc* d, int n_desc, uint32_t grid_x, hipStream_t s);
__attribute__((weak)) void launch_conv_inv(const ConvDesc* d, int n_desc, uint32_t grid_x, hipStream_t s);
// Weak for the same reason: a level's reverb vertices.  launch_reverb_sum: grid.x from `frames`; launch_reverb: one workgroup per
// descriptor, `form` 0 the serial walk of each comb's one-pole, 1 the wave scan.
__attribute__((weak)) void launch_reverb_sum(const ReverbDesc* d, int n_desc, uint32_t frames, hipStream_t s);
__attribute__((weak)) void launch_reverb(const ReverbDesc* d, int n_desc, uint32_t form, hipStream_t s);
void launch_sinf(const float* in, float* out, uint32_t n, int exact, hipStream_t s);   // out[i] = sin_glibc(in[i]) (exact) or sin_any(in[i])
void launch_debug_verify(const uint32_t* p, uint32_t n_words, const uint32_t* seg_sums, uint32_t* report, hipStream_t s);   // (TD_DEBUG_SYNC & 16)
void launch_sample_loop(const LoopDesc* d, int n_desc, uint32_t frames, hipStream_t s);
void launch_sample_multi(const MultiDesc* d, int n_desc, uint32_t frames, hipStream_t s);
void launch_sample_lerp(const LerpDesc* d, int n_desc, uint32_t frames, hipStream_t s);
void launch_debug_sine(const SineDesc* d, int n_desc, uint32_t frames, uint32_t bl, hipStream_t s);
void launch_synth(const SynthDesc* d, int n_desc, uint32_t frames, bool affine, hipStream_t s);   // every descriptor: SynthDesc::affine == affine
void launch_sampsyn(const SampsynDesc* d, int n_desc, uint32_t frames, hipStream_t s);
// k_sources: the source launches of a level and the envelope launch as the parts of ONE grid (kernels.hip); the engine lists
// the parts longest-running family first, launch_sources fills in the grid geometry
enum SourceKind : uint32_t { SRC_SYNTH_AFFINE = 0, SRC_SAMPSYN = 1, SRC_LERP = 2, SRC_ENV = 3 };
struct SourceParts {   // the launches that become parts (n_* 0: none of that kind)
    const SynthDesc* synth = nullptr; int n_synth = 0;       // every descriptor: SynthDesc::affine set
    const SampsynDesc* sampsyn = nullptr; int n_sampsyn = 0;
    const LerpDesc* lerp = nullptr; int n_lerp = 0;
    const AdsrVDesc* env = nullptr; int n_env = 0;
};
struct SourceGrid {
    uint32_t gx[4], end[4];   // per SourceKind: workgroups per descriptor; the first workgroup BEHIND the part
    // The submission's zeroed hand-off words (ChunkBuild::sync_bytes: tickets and granules of the scan launches BEHIND this one
    // on the stream), cleared by this grid's threads instead of by a fill kernel of their own (16-byte words; 0: nothing)
    uint4* zero;
    uint32_t zero_n16, pad;
};
int launch_sources(const SourceParts& P, uint32_t frames, void* zero, size_t zero_bytes, hipStream_t s);   // zero_bytes: a multiple of 16
void launch_adsr(const AdsrVDesc* d, int n_desc, uint32_t frames, uint32_t term_mode, hipStream_t s);
void launch_band_pass(const BandDesc* d, int n_desc, uint32_t frames, hipStream_t s);

}  // namespace tdk
