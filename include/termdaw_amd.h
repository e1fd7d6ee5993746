/* termdaw_amd.h -- C ABI of the MI355X-native offline render engine for termdaw audio graphs.
 *
 * This is the drop-in boundary for termdaw's per-block vertex/graph render path.  The reference
 * (Rust, /root/reference/src) has no FFI of its own: its "operator API" is the in-process surface
 * State (state.rs) uses to talk to Graph (graph.rs), SampleBank (sample.rs) and FlowwBank
 * (floww.rs).  Every entry point below cites the reference item it replaces; INTEGRATION.md shows
 * the Rust `extern "C"` block a termdaw maintainer would add to bind them.
 *
 * Conventions
 *   - plain C types only; opaque handles are created/destroyed by the library
 *   - functions returning int: 1 = ok/true, 0 = failed/false (mirrors the reference's bool / Result /
 *     Option); td_last_error() returns the message of the last failure on the calling thread
 *   - audio is f32; "frames" are stereo frames; PCM out is interleaved L,R little-endian
 *   - one host thread per graph handle; handles bound to different GPUs are independent.  Handles may be
 *     freed in any order, also with asynchronous renders not yet synced; a SampleBank that gives device
 *     memory back (td_samplebank_free, an entry replaced) first completes what is queued on its GPU, so do
 *     that from the thread that renders the graphs using the bank
 *   - the library never falls back to a CPU implementation: without a usable gfx950 device every
 *     render call fails with an error
 */
#ifndef TERMDAW_AMD_H
#define TERMDAW_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct td_samplebank td_samplebank;
typedef struct td_flowwbank td_flowwbank;
typedef struct td_graph td_graph;
typedef struct td_state td_state;
typedef struct td_batch td_batch;
typedef struct td_comm td_comm;       /* the ranks of a multi-GPU job, for the one collective of the path (td_batch_exchange_peaks) */

/* One event of a floww: the (_, t, note, vel) tuple of the floww crate as used at floww.rs:74-75,
 * 105-116, 131-135 (field 0 is never read on the render path). vel <= 0.001 means note-off. */
typedef struct td_event {
    float t_sec;
    float note;
    float vel;
} td_event;

const char* td_last_error(void);
/* HIP device selection for handles created afterwards on this thread (one process per GPU). */
int td_device_count(void);
int td_set_device(int device);

/* ---- SampleBank (sample.rs:187-348) -------------------------------------------------------- */
td_samplebank* td_samplebank_new(size_t sample_rate);                    /* SampleBank::new   sample.rs:213 */
void td_samplebank_free(td_samplebank* sb);
/* SampleBank::add sample.rs:224-314 (WAV decode -> load mode -> peak normalise -> upload to HBM).
 * method: "" (stereo) | "left" | "right" | "loudest" | "normalize-seperate" | "mix-down".
 * A file whose rate differs from the bank's is resampled (Sample::resample sample.rs:150-175) with this
 * engine's own sinc resampler (rubato is un-vendored: parity unpinned, DESIGN.md "Resampler"). */
int td_samplebank_add_file(td_samplebank* sb, const char* name, const char* path, const char* method);
/* Same pipeline from an already decoded stream (what hound hands to sample.rs:262-274): `linear`
 * holds n interleaved values, integer PCM cast to f32 without scaling, or float PCM as is. */
int td_samplebank_add_decoded(td_samplebank* sb, const char* name, const float* linear, size_t n,
                              int channels, size_t sample_rate, size_t bits, const char* method);
long td_samplebank_get_index(const td_samplebank* sb, const char* name);  /* get_index sample.rs:338; -1 = None */
size_t td_samplebank_sample_len(const td_samplebank* sb, size_t index);   /* Sample::len sample.rs:79 */
/* get_sample sample.rs:342: copies the bank entry back from HBM as planar l / r. */
int td_samplebank_read(const td_samplebank* sb, size_t index, float* l, float* r);
void td_samplebank_get_max_sr_bd(const td_samplebank* sb, size_t* max_sr, size_t* max_bd); /* sample.rs:346 */

/* ---- FlowwBank (floww.rs:6-141) ------------------------------------------------------------- */
td_flowwbank* td_flowwbank_new(size_t sr, size_t bl);                     /* FlowwBank::new floww.rs:19 */
void td_flowwbank_free(td_flowwbank* fb);
void td_flowwbank_reset(td_flowwbank* fb);                                /* floww.rs:23-30 */
/* declare_floww floww.rs:32-38 with the events given directly (add_floww floww.rs:40-48 reads them
 * from MIDI through the un-vendored floww crate). Returns the floww index, or -1. */
long td_flowwbank_add_events(td_flowwbank* fb, const char* name, const td_event* events, size_t n);
/* add_floww floww.rs:40-48: a Standard MIDI File through this library's own reader (the floww crate's
 * read_floww_from_midi is un-vendored; mapping fixed in csrc/midi.h).  Returns the floww index, or -1 with
 * the reference's "Could not read midi file" message in td_last_error(). */
long td_flowwbank_add_midi(td_flowwbank* fb, const char* name, const char* path);
long td_flowwbank_declare_stream(td_flowwbank* fb, const char* name);     /* floww.rs:50-53 */
/* append_streams floww.rs:55-57 with the packets already decoded (`unpacket` is the floww crate's): appends
 * events to the named floww.  Returns its new length, or -1 if the name is unknown. */
long td_flowwbank_append_stream(td_flowwbank* fb, const char* name, const td_event* events, size_t n);
void td_flowwbank_trim_streams(td_flowwbank* fb);                         /* floww.rs:59-64 */
/* copy of floww `index` (at most cap events are written); returns its length */
size_t td_flowwbank_get_events(const td_flowwbank* fb, size_t index, td_event* out, size_t cap);
long td_flowwbank_get_index(const td_flowwbank* fb, const char* name);    /* floww.rs:66-68 */
void td_flowwbank_set_time(td_flowwbank* fb, size_t t);                   /* floww.rs:83-86 */
void td_flowwbank_set_time_to_next_block(td_flowwbank* fb);               /* floww.rs:88-91 */

/* ---- Graph (graph.rs:12-238) + vertex constructors (extensions.rs:83-194, state.rs:341-457) -- */
td_graph* td_graph_new(size_t max_buffer_len, size_t sr);                 /* Graph::new graph.rs:25 */
void td_graph_free(td_graph* g);
void td_graph_reset(td_graph* g);                                         /* graph.rs:39-47 */
/* Graph::add(Vertex::new(bl, gain, angle, wet, VertexExt::<kind>(..)), name).  Argument fix-ups are
 * those of state.rs:341-457: note < 0 -> any note; lerp_len < 0 -> 0; square z clamped to >= 1e-4;
 * adsr arrays of 0, 6 or 9 floats (anything else fails, where the reference panics). */
int td_graph_add_sum(td_graph* g, const char* name, float gain, float angle);
int td_graph_add_normalize(td_graph* g, const char* name, float gain, float angle);
int td_graph_add_sampleloop(td_graph* g, const char* name, float gain, float angle, size_t sample_index);
int td_graph_add_sample_multi(td_graph* g, const char* name, float gain, float angle, size_t sample_index,
                              size_t floww_index, int note);
int td_graph_add_sample_lerp(td_graph* g, const char* name, float gain, float angle, size_t sample_index,
                             size_t floww_index, int note, int lerp_len);
int td_graph_add_debug_sine(td_graph* g, const char* name, float gain, float angle, size_t floww_index);
int td_graph_add_synth(td_graph* g, const char* name, float gain, float angle, size_t floww_index,
                       float square_vel, float square_z, const float* square_adsr, int square_adsr_len,
                       float topflat_vel, float topflat_z, const float* topflat_adsr, int topflat_adsr_len,
                       float triangle_vel, const float* triangle_adsr, int triangle_adsr_len);
/* add_sampsyn (state.rs:406-426, extensions.rs:143-150,532-578).  The wavetable oscillator and its file
 * format live in the un-vendored sampsyn crate; this engine defines its own (DESIGN.md "Wavetable voice":
 * "TDWT" u32 version=1, u32 n_frames, u32 frame_len, f32 table_seconds, n_frames*frame_len f32 LE) --
 * parity with the reference is unpinned.  Unparseable / NULL bytes select the default table. */
int td_graph_add_sampsyn(td_graph* g, const char* name, float gain, float angle, size_t floww_index, const float* adsr,
                         int adsr_len, const void* table_bytes, size_t table_len);
int td_graph_add_adsr(td_graph* g, const char* name, float gain, float angle, float wet, size_t floww_index,
                      int use_off, int use_max, int note, const float* adsr, int adsr_len);
int td_graph_add_bandpass(td_graph* g, const char* name, float gain, float angle, float wet,
                          float cut_off_hz_low, float cut_off_hz_high, int pass);
/* A compressor vertex -- THIS ENGINE'S OWN: no reference counterpart (the reference reaches dynamics through LV2 plugins,
 * add_lv2fx, which this engine parses and drops).  A feed-forward, stereo-linked, log-domain compressor with the
 * decoupled peak detector of Giannoulis, Massberg, Reiss (JAES 2012).  The vertex sums its inputs like every input vertex
 * (sum_inputs, extensions.rs:310-319), processes, mixes with `wet`, then pan and gain like every vertex (extensions.rs:262-263).
 *   sr: the graph's rate.  aR = exp(-1 / (release_ms sr / 1000));  aA = exp(-1 / (attack_ms sr / 1000)), aA = 0 for attack_ms = 0;
 *   T, R, W, M = threshold_db, ratio, knee_db, makeup_db (each f32 parameter widened to f64).  Steps 1-5 in f64 on the f32
 *   summed input (l[n], r[n]):
 *   1. level s[n] = max(|l[n]|, |r[n]|).  s[n] zero or not finite: d[n] = 0.
 *   2. otherwise x = 20 log10(s[n]), o = x - T, and the wanted reduction in dB
 *        d[n] = 0                                  for 2 o < -W
 *               (1 - 1/R) (o + W/2)^2 / (2 W)      for 2 |o| <= W  (only when W > 0)
 *               (1 - 1/R) o                        for 2 o > W
 *   3. release:  y1[n] = max(d[n], aR y1[n-1])
 *   4. attack:   yL[n] = aA yL[n-1] + (1 - aA) y1[n]
 *   5. G[n] = 10^((M - yL[n]) / 20);  p = (float)(l[n] G[n]), the same for r (a NaN / infinite input frame stays what IEEE
 *      makes of it, at that frame only: step 1 keeps it out of the state)
 *   6. in f32, the reference's lerp (adsr.rs:42): out = l + wet * (p - l); then pan and gain.  wet < 0.0001: the summed input
 *      passes through untouched and the state stays as it is.
 * State: (y1, yL), two doubles, (0, 0) at time 0; carried between consecutive block pulls and between the chunks of a render,
 * reset to (0, 0) by td_graph_set_time / td_graph_change_time / td_graph_reset (so every whole render starts from (0, 0)).
 * Ranges, rejected with a td_last_error that names the parameter (NaN included): threshold_db [-80, 0], ratio [1, 1000],
 * attack_ms [0, 1000], release_ms [1, 10000], knee_db [0, 40], makeup_db [-40, 40].  `wet` is clamped to [0, 1].
 * Under "band_mode" 2 / "sine_mode" 2 everything upstream of a compressor vertex takes the exact forms (no estimate is carried
 * through a gain that depends on the signal). */
int td_graph_add_compressor(td_graph* g, const char* name, float gain, float angle, float wet, float threshold_db,
                            float ratio, float attack_ms, float release_ms, float knee_db, float makeup_db);
/* A parametric EQ vertex -- THIS ENGINE'S OWN: no reference counterpart (the reference reaches an equaliser only through LV2
 * plugins, add_lv2fx, which this engine parses and drops).  One biquad of Robert Bristow-Johnson's "Audio EQ
 * Cookbook" per channel.  The vertex sums its inputs like every input vertex (sum_inputs, extensions.rs:310-319), filters l and
 * r independently, mixes with `wet`, then pan and gain like every vertex (extensions.rs:262-263).
 *   Coefficients, once on the host in f64 from the f32 parameters widened; sr: the graph's rate.
 *     w0 = 2 pi freq_hz / sr,  alpha = sin w0 / (2 q),  A = 10^(gain_db / 40)   (1 - cos w0 is evaluated as 2 sin^2(w0 / 2))
 *     TD_EQ_LOWPASS    b = ((1 - cos w0) / 2, 1 - cos w0, (1 - cos w0) / 2),    a = (1 + alpha, -2 cos w0, 1 - alpha)
 *     TD_EQ_HIGHPASS   b = ((1 + cos w0) / 2, -(1 + cos w0), (1 + cos w0) / 2), the same a
 *     TD_EQ_BANDPASS   b = (alpha, 0, -alpha)  (constant 0 dB peak gain),       the same a
 *     TD_EQ_NOTCH      b = (1, -2 cos w0, 1),                                   the same a
 *     TD_EQ_PEAK       b = (1 + alpha A, -2 cos w0, 1 - alpha A),               a = (1 + alpha / A, -2 cos w0, 1 - alpha / A)
 *     TD_EQ_LOWSHELF   with S = 2 sqrt(A) alpha (the cookbook's shelves in their Q form):
 *                      b = (A ((A+1) - (A-1) cos w0 + S), 2 A ((A-1) - (A+1) cos w0), A ((A+1) - (A-1) cos w0 - S)),
 *                      a = ((A+1) + (A-1) cos w0 + S, -2 ((A-1) + (A+1) cos w0), (A+1) + (A-1) cos w0 - S)
 *     TD_EQ_HIGHSHELF  b = (A ((A+1) + (A-1) cos w0 + S), -2 A ((A-1) + (A+1) cos w0), A ((A+1) + (A-1) cos w0 - S)),
 *                      a = ((A+1) - (A-1) cos w0 + S, 2 ((A-1) - (A+1) cos w0), (A+1) - (A-1) cos w0 - S)
 *     each divided by a0: (b0, b1, b2, a1, a2).  td_eq_coefficients returns exactly the values the engine uses.
 *   Recurrence, per channel, in f64, transposed direct form II, on the f32 summed input x[n]:
 *     y[n] = b0 x[n] + s1;   s1 = (b1 x[n] - a1 y[n]) + s2;   s2 = b2 x[n] - a2 y[n];   p[n] = (float)y[n]
 *     A non-finite x[n] enters the recurrence as 0 and its frame's p[n] is x[n] itself: the state never holds a NaN.
 *   Then in f32, the reference's lerp (adsr.rs:42): out = x + wet * (p - x); then pan and gain.  wet < 0.0001: the summed input
 *   passes through untouched and the state stays as it is.
 * State: (s1l, s2l, s1r, s2r), four doubles, zero at time 0; carried between consecutive block pulls and between the chunks of
 * a render, reset to zero by td_graph_set_time / td_graph_change_time / td_graph_reset (so every whole render starts from zero).
 * Ranges, rejected with a td_last_error that names the parameter (NaN included): kind 0 .. 6, freq_hz [10, 0.45 sr], q [0.1, 20],
 * gain_db [-24, 24] (ignored by the four kinds without gain).  `wet` is clamped to [0, 1].
 * Under "band_mode" 2 / "sine_mode" 2 the estimate is carried through an EQ vertex at the gain (1 - wet) + wet Hmax, Hmax the
 * largest |H(e^jw)| of the biquad: vertices upstream keep their scan / fast forms. */
enum { TD_EQ_LOWPASS = 0, TD_EQ_HIGHPASS = 1, TD_EQ_BANDPASS = 2, TD_EQ_NOTCH = 3, TD_EQ_PEAK = 4, TD_EQ_LOWSHELF = 5, TD_EQ_HIGHSHELF = 6 };
int td_graph_add_eq(td_graph* g, const char* name, float gain, float angle, float wet, int kind, float freq_hz, float q,
                    float gain_db);
/* Host only, no GPU: the EQ vertex' coefficients at rate sr -- out[0 .. 4] = b0 b1 b2 a1 a2 (a0 = 1) as the engine uses them,
 * out[5] = Hmax, the maximum over w of |H(e^jw)|, in closed form (|H|^2 is a ratio of two quadratics in sin^2(w / 2): the
 * maximum lies at w = 0, w = pi or a root of a quadratic).  The same range checks as td_graph_add_eq. */
int td_eq_coefficients(int kind, size_t sr, float freq_hz, float q, float gain_db, double out[6]);
/* A feedback delay (echo) vertex -- THIS ENGINE'S OWN: no reference counterpart (the reference reaches a delay only through LV2
 * plugins, add_lv2fx, which this engine parses and drops).  The vertex sums its inputs like every input vertex
 * (sum_inputs, extensions.rs:310-319), processes, mixes with `wet` by the reference's f32 lerp, then pan and gain like every
 * vertex (extensions.rs:262-263).
 *   Constants, once on the host in f64 from the f32 parameters widened; sr: the graph's rate.
 *     D = max(1, llround(time_ms sr / 1000)),   gs = feedback (1 - cross),   gc = feedback cross
 *   Recurrence, in f64, on the f32 summed input x[n]; w = u[n - D] comes from the line, which is all zeros before time 0:
 *     ul[n] = xl[n] + (gs wl + gc wr);   ur[n] = xr[n] + (gs wr + gc wl);   pl[n] = (float)(xl[n] + wl), likewise pr
 *     in exactly this operation order, with no FMA contraction.  The first echo is therefore at full level and `feedback` sets
 *     every later one: feedback = 0 is a single slapback; cross = 1 alternates the echoes between the channels.
 *     A non-finite x[n] enters the line as 0 and its frame's p[n] is x[n] itself: the line never holds a NaN.
 *   Then in f32, the reference's lerp (adsr.rs:42): out = x + wet * (p - x), which is x + wet * echoes; then pan and gain.
 *   wet < 0.0001: the summed input passes through untouched (a plain k_sum launch) and the line stays as it is.
 * State: the line, the last D values of (ul, ur) as doubles, 16 D bytes of device memory (counted by td_graph_device_bytes,
 * allocated when the vertex is first rendered); zero at time 0, carried between consecutive block pulls and between the chunks of
 * a render, restarted from zero by td_graph_set_time / td_graph_change_time / td_graph_reset (so every whole render starts from
 * zero).  A render ends where the project ends: no tail is appended.
 * Ranges, rejected with a td_last_error that names the parameter (NaN included): time_ms [1, 2000], feedback [0, 0.98],
 * cross [0, 1].  `wet` is clamped to [0, 1].
 * Under "band_mode" 2 / "sine_mode" 2 the estimate is carried through a delay vertex at the gain 1 + wet Hecho,
 * Hecho = 1 / (1 - feedback) the L2 gain of the echo path (G = [[gs, gc], [gc, gs]] is symmetric with eigenvalues feedback and
 * feedback (1 - 2 cross)): vertices upstream keep their scan / fast forms.
 * Not part of the vertex: a low-pass in the feedback path ("damping": its u[n-1] term couples the D recurrences; the reverb vertex
 * has one, by another kernel shape), modulated or fractional delay times, tempo sync, a tail past the project's end. */
int td_graph_add_delay(td_graph* g, const char* name, float gain, float angle, float wet, float time_ms, float feedback,
                       float cross);
/* Host only, no GPU: the delay vertex' constants at rate sr -- out[0 .. 3] = D, gs, gc, Hecho as the engine uses them.  The same
 * range checks as td_graph_add_delay. */
int td_delay_params(size_t sr, float time_ms, float feedback, float cross, double out[4]);
/* A saturator vertex: an oversampled waveshaper -- THIS ENGINE'S OWN: no reference counterpart (the reference reaches drive and
 * clipping only through LV2 plugins, add_lv2fx, which this engine parses and drops).  The vertex sums its inputs
 * like every input vertex (sum_inputs, extensions.rs:310-319), processes, mixes with `wet` by the reference's f32 lerp, then pan
 * and gain like every vertex (extensions.rs:262-263).
 *   Constants, once on the host in f64:  Z = 32,  R = oversample,  L = 2 Z R + 1.
 *   Prototype low-pass, a 4-term Blackman-Harris windowed sinc; t = k - Z R, fc = (0.5 - 2 / Z) / R cycles per oversampled sample:
 *     s[k] = 2 fc at t = 0, else sin(2 pi fc t) / (pi t)
 *     w[k] = 0.35875 - 0.48829 cos(2 pi k / (L - 1)) + 0.14128 cos(4 pi k / (L - 1)) - 0.01168 cos(6 pi k / (L - 1))
 *     h = s w / sum(s w)
 *     The taps do not depend on the sample rate: in units of sr the pass band reaches 0.375, the response is -1 dB at 0.417 and
 *     the stop band (<= -105 dB) starts at 0.5.
 *   g_in = 10^(drive_db / 20),  g_out = 10^(out_db / 20),  fb = f(bias)   (f32 parameters widened)
 *   Shapers f (IEEE operations only):  hard  min(max(u, -1), 1);   cubic  1.5 u - ((0.5 u) u) u for |u| < 1, else sign(u);
 *     soft  u / (1 + |u|).  Lipschitz constants Lf = 1, 1.5, 1.
 *   Pipeline per channel, in f64 on the f32 summed input x, with no FMA contraction and every sum accumulated from acc = 0.0 in
 *   ascending index:
 *     xs[n] = x[n] if finite, else 0; frames before time 0 are 0
 *     up-sampling, polyphase (no zero-stuffed terms):  v[n R + r] = sum_{j = 0 .. J_r} (R h[r + j R]) xs[n - j],
 *         J_0 = 2 Z, J_r = 2 Z - 1 for r > 0
 *     shaper:      w[m] = f(g_in v[m] + bias) - fb
 *     decimation:  y[n] = sum_{k = 0 .. L - 1} h[k] w[n R - k]
 *     output:      p[n] = (float)(g_out y[n])
 *   LATENCY: the two linear-phase filters delay by exactly 2 Z = 64 frames, so the dry leg of the lerp is delayed to match:
 *     xd[n] = x[n - 64] (raw f32, zeros before time 0);  out = xd + wet * (p - xd) in f32 (adsr.rs:42); then pan and gain.
 *     The vertex therefore delays its signal by 64 frames (td_saturator_params returns it); nothing compensates for that
 *     elsewhere in the graph.  A non-finite x[n] reaches the output through xd only, at frame n + 64.
 *   oversample = 1 has no filters, no latency and no state:  p = (float)(g_out (f(g_in x + bias) - fb)), a non-finite x gives
 *     p = x;  out = x + wet * (p - x).
 *   wet < 0.0001: the summed input passes through untouched (a plain k_sum launch) and the line stays as it is.
 * State (oversample > 1): the line, the last 4 Z = 128 raw input frames (64 for the decimator's reach, 64 more for the up-sampler
 * under it), kept as two halves used alternately: 2 KB of device memory (counted by td_graph_device_bytes, allocated when the
 * vertex is first rendered); silent at time 0, carried between consecutive block pulls and between the chunks of a render,
 * restarted from silence by td_graph_set_time / td_graph_change_time / td_graph_reset.  A render ends where the project ends: no
 * tail is appended.
 * Ranges, rejected with a td_last_error that names the parameter (NaN included): kind 0 .. 2, oversample 1 | 2 | 4 | 8, drive_db
 * [-24, 48], bias [-1, 1], out_db [-48, 24].  `wet` is clamped to [0, 1].
 * Under "band_mode" 2 / "sine_mode" 2 the estimate is carried through a saturator vertex at the gain (1 - wet) + wet Hsat,
 * Hsat = g_out Hdown Lf g_in Hup with Hup = sqrt(sum_r max_w |U_r|^2) over the up-sampler's branches U_r = R h[r::R] and Hdown
 * the same over the decimator's G_r = h[r::R] (Hup Hdown = 1.000005; oversample = 1: Hsat = g_out Lf g_in): vertices upstream
 * keep their scan / fast forms.
 * Not part of the vertex: tanh / exp shapers (not IEEE-exact on the device), a tail past the project's end, latency
 * compensation across the graph, per-band drive. */
enum { TD_SAT_HARD = 0, TD_SAT_CUBIC = 1, TD_SAT_SOFT = 2 };
int td_graph_add_saturator(td_graph* g, const char* name, float gain, float angle, float wet, int kind, float drive_db, float bias,
                           float out_db, int oversample);
/* Host only, no GPU: the engine's own prototype taps h[0 .. L - 1], L = 64 oversample + 1.  Writes min(L, cap) of them (taps may
 * be null) and returns L; 0 for an oversample that is not 1, 2, 4 or 8. */
int td_saturator_taps(int oversample, double* taps, size_t cap);
/* Host only, no GPU: the saturator vertex' constants -- out[0 .. 5] = g_in, g_out, f(bias), the latency in frames, Lf, Hsat as
 * the engine uses them.  The same range checks as td_graph_add_saturator. */
int td_saturator_params(int kind, int oversample, float drive_db, float bias, float out_db, double out[6]);
/* A chorus vertex: LFO-modulated fractional delay lines -- THIS ENGINE'S OWN: no reference counterpart (the reference reaches
 * modulation effects only through LV2 plugins, add_lv2fx, which this engine parses and drops).  The vertex sums its
 * inputs like every input vertex (sum_inputs, extensions.rs:310-319), processes, mixes with `wet` by the reference's f32 lerp,
 * then pan and gain like every vertex (extensions.rs:262-263).  wet 0.5 with 2 .. 4 voices is a chorus, wet 1 with one voice a
 * vibrato, a short delay_ms a feed-forward flanger, depth_ms 0 a static fractional delay.
 *   Everything is f64 on the f32 summed input x, with no FMA contraction and IEEE add, multiply, floor and fabs only (no libm on
 *   either side), in exactly the order written here.
 *   Constants, once on the host from the f32 parameters widened:  D0 = delay_ms sr / 1000,  A = depth_ms sr / 1000 (frames),
 *     f = rate_hz / sr (cycles per frame),  H = floor(D0 + A) + 3 rounded up to a multiple of 64 (frames of the line),
 *     s = (2 pi A) f for a sine, (4 A) f for a triangle: the largest change of the delay per frame,  iv = 1 / V.
 *   LFO, for voice v = 0 .. V - 1 and channel c at frame n -- n is the graph's ABSOLUTE frame time, so a render that
 *   td_graph_set_time starts in the middle of a project sees the modulation a whole render sees there, whatever the chunking:
 *     phi = v iv  (left),  v iv + stereo  (right);   th = n f + phi;  th = th - floor(th)
 *     triangle:  lfo = 1 - 4 |th - 0.5|
 *     sine:      u = 4 th for th < 0.25,  2 - 4 th for th < 0.75,  else 4 th - 4   (sin(2 pi th) = sin(pi u / 2), u in [-1, 1]);
 *                u2 = u u;  p = c9;  p = p u2 + c7;  p = p u2 + c5;  p = p u2 + c3;  p = p u2 + c1;  lfo = u p
 *                with (pi/2)^k / k!, signed:  c1 = 1.5707963267948966, c3 = -0.6459640975062463, c5 = 0.07969262624616705,
 *                c7 = -0.004681754135318688, c9 = 0.00016044118478735983  -- within 3.6e-6 of sin, |lfo| <= 1 + 3.6e-6
 *   Read:  d = D0 + A lfo;  i = floor(d);  mu = d - i;  m = n - i
 *     xs[j] = x[j] if finite, else 0; frames before the line's start are 0
 *     a = mu - 1, b = mu - 2, e = mu + 1;   four-point Lagrange weights
 *       w0 = ((mu a) b) (-1/6),  w1 = ((e a) b) (1/2),  w2 = ((e mu) b) (-1/2),  w3 = ((e mu) a) (1/6)      (1/6 = 0.16666666666666666)
 *     y = 0.0;  y = y + w0 xs[m + 1];  y = y + w1 xs[m];  y = y + w2 xs[m - 1];  y = y + w3 xs[m - 2]
 *     (D0 - A >= 2 keeps i >= 1 even at the polynomial's overshoot: no future frame is read; at the far end the overshoot can
 *      carry i to floor(D0 + A) + 1, so i + 2 <= H: the oldest frame read is at most H back, the line's first word)
 *   Output:  S = 0.0;  S = S + y_v for v ascending;  p[n] = (float)(iv S);
 *     out = x + wet * (p - x) in f32 with the undelayed input (adsr.rs:42); then pan and gain.  The vertex has no latency.  A
 *     non-finite x[n] makes frame n of the output non-finite and no other.
 *   wet < 0.0001: the summed input passes through untouched (a plain k_sum launch) and the line stays as it is.
 * State: the line, the last H raw input frames (at most 2 432 at 48 kHz), kept as two halves used alternately: 16 H bytes of
 * device memory (counted by td_graph_device_bytes, allocated when the vertex is first rendered); silent at the start, carried
 * between consecutive block pulls and between the chunks of a render, restarted from silence by td_graph_set_time /
 * td_graph_change_time / td_graph_reset -- the LFO is not restarted, it is a function of the time alone.  A render ends where the
 * project ends: no tail is appended.
 * Ranges, rejected with a td_last_error that names the parameter (NaN included): voices 1 .. 4, delay_ms [0.5, 50], depth_ms >= 0
 * with D0 - A >= 2 frames and delay_ms + depth_ms <= 50, rate_hz [0.01, 20] with s <= 0.5 (the error names rate_hz), stereo
 * [0, 0.5], shape 0 .. 1.  `wet` is clamped to [0, 1].
 * Under "band_mode" 2 / "sine_mode" 2 the estimate is carried through a chorus vertex at the gain (1 - wet) + wet Hch, Hch =
 * 2.307 an L2 bound of x -> p for every parameter in range (DESIGN.md 3q has the proof): vertices upstream keep their scan / fast
 * forms.
 * Not part of the vertex: feedback around the modulated line (a time-varying recurrence), tempo sync, other interpolators, a
 * tail past the project's end. */
enum { TD_CHORUS_SINE = 0, TD_CHORUS_TRIANGLE = 1 };
int td_graph_add_chorus(td_graph* g, const char* name, float gain, float angle, float wet, int voices, float delay_ms, float depth_ms,
                        float rate_hz, float stereo, int shape);
/* Host only, no GPU: the chorus vertex' constants at rate sr -- out[0 .. 5] = D0, A, f, H (frames of the line), s (the largest
 * delay slope) and Hch as the engine uses them.  The same range checks as td_graph_add_chorus. */
int td_chorus_params(size_t sr, int voices, float delay_ms, float depth_ms, float rate_hz, float stereo, int shape, double out[6]);
/* A reverb vertex: a damped comb bank and an all-pass chain -- THIS ENGINE'S OWN: no reference counterpart (the reference reaches
 * reverb only through LV2 plugins, add_lv2fx, which this engine parses and drops).  The topology is the
 * public-domain Freeverb's: per channel 8 parallel feedback combs with a one-pole low-pass in the feedback path ("damping": the
 * u[n-1] term the delay vertex leaves out), then 4 all-pass sections in series.  The vertex sums its inputs like every input vertex
 * (sum_inputs, extensions.rs:310-319), processes, mixes with `wet` by the reference's f32 lerp, then pan and gain like every vertex
 * (extensions.rs:262-263).
 *   Everything is f64 on the f32 summed input x, with no FMA contraction, in exactly the order written here.
 *   Constants, once on the host from the f32 parameters widened:  g = 0.7 + 0.28 room,  d1 = 0.4 damp,  d2 = 1 - d1,
 *     w1 = (1 + width) / 2,  w2 = (1 - width) / 2.
 *   Tunings in frames at 44.1 kHz:  combs 1116, 1188, 1277, 1356, 1422, 1491, 1557, 1617;  all-passes 556, 441, 341, 225.
 *   Line lengths:  D = llround(tuning size sr / 44100) on the left,  llround((tuning + 23) size sr / 44100) on the right
 *     (D_c the combs', E_a the all-passes').
 *   Per frame n, xs = x where finite, else 0:   in = (xsl + xsr) 0.015
 *   Per channel, combs c = 0 .. 7 ascending, S = 0.0 first:
 *     w = cline_c[n - D_c];   f_c = w d2 + f_c d1;   cline_c[n] = in + f_c g;   S = S + w
 *   Per channel, all-passes a = 0 .. 3 in series, s = S first:
 *     v = aline_a[n - E_a];   y = v - s;   aline_a[n] = s + v 0.5;   s = y          then A_ch = s
 *   Output:  pl = (float)(Al w1 + Ar w2),  pr = (float)(Ar w1 + Al w2);
 *     out = x + wet * (p - x) in f32 with the raw input (adsr.rs:42); then pan and gain.  A non-finite x[n] makes frame n of the
 *     output non-finite and enters the lines as 0: the lines never hold a NaN.
 *   wet < 0.0001: the summed input passes through untouched (a plain k_sum launch) and the state stays as it is.
 * State: the 24 lines and the 16 f_c, all doubles, one block of device memory (counted by td_graph_device_bytes, allocated when
 * the vertex is first rendered, 8 (16 + the sum of the line lengths) bytes: 204 KB at 44.1 kHz and size 1); frame m of a line,
 * counted from the restart, lives in slot m mod D, a read of m - D < 0 is 0; silent at the start, carried between consecutive
 * block pulls and between the chunks of a render, restarted from silence by td_graph_set_time / td_graph_change_time /
 * td_graph_reset.  A render ends where the project ends: no tail is appended.
 * Ranges, rejected with a td_last_error that names the parameter (NaN included): room, damp, width [0, 1]; size [0.5, 2], and the
 * shortest of the 24 lines must be at least 64 frames (at a low sample rate the error names size).  `wet` is clamped to [0, 1].
 * Under "band_mode" 2 / "sine_mode" 2 the estimate is carried through a reverb vertex at the gain (1 - wet) + wet Hrev, Hrev =
 * 0.03 x 8 / (1 - g) x (5/3)^4 an L2 bound of x -> p (DESIGN.md 3r has the proof): vertices upstream keep their scan / fast forms.
 * Not part of the vertex: pre-delay, a tail past the project's end, modulated lines; convolution with a measured response is a
 * vertex of its own (td_graph_add_convolution below). */
int td_graph_add_reverb(td_graph* g, const char* name, float gain, float angle, float wet, float room, float damp, float width, float size);
/* Host only, no GPU: the reverb vertex' constants at rate sr -- out[0 .. 4] = g, d1, d2, w1, w2; out[5] = Hrev; out[6] = B, the
 * frames per window of k_reverb at the default "debug.reverb_block"; out[7 .. 30] = the line lengths: left combs, right combs,
 * left all-passes, right all-passes.  The same range checks as td_graph_add_reverb. */
int td_reverb_params(size_t sr, float room, float damp, float width, float size, double out[31]);
/* A noise gate vertex -- THIS ENGINE'S OWN: no reference counterpart (the reference reaches dynamics through LV2 plugins,
 * add_lv2fx, which this engine parses and drops).  Stereo-linked level detection with hysteresis, a hold counter and
 * an attack / release fade of the gain between `range_db` and 0 dB.  The vertex sums its inputs like every input vertex
 * (sum_inputs, extensions.rs:310-319), processes, mixes with `wet` by the reference's f32 lerp, then pan and gain like every
 * vertex (extensions.rs:262-263).
 *   Constants, f64, once on the host, each from the f32 parameter widened to f64 (td_gate_params returns them):
 *     To = 10^(threshold_db / 20);  Tc = 10^((threshold_db - hysteresis_db) / 20);  H = llround(hold_ms sr / 1000) frames;
 *     aA = exp(-1 / (attack_ms sr / 1000)), aA = 0 for attack_ms = 0;  aR the same from release_ms;  F = 10^(range_db / 20).
 *   Steps 1-5 in f64 on the f32 summed input (l[n], r[n]), with no FMA contraction, in the order written:
 *   1. level s[n] = max(|l[n]|, |r[n]|).  A frame with a NaN or infinite sample forces nothing in step 2 (it comes out as what
 *      IEEE makes of it, at that frame only).
 *   2. hysteresis, in the linear domain:  h[n] = 1 if s[n] >= To;  h[n] = 0 if s[n] < Tc;  h[n] = h[n-1] otherwise.
 *   3. hold:  c[n] = 0 if h[n] == 1, else min(c[n-1] + 1, H + 1).  The target t[n] = 1 if c[n] <= H, else 0.
 *   4. fade:  a[n] = aA if t[n] == 1, else aR;   env[n] = a[n] env[n-1] + (1 - a[n]) t[n].
 *   5. G[n] = F + (1 - F) env[n];  p = (float)(l[n] G[n]), the same for r.
 *   6. in f32, the reference's lerp (adsr.rs:42): out = l + wet * (p - l); then pan and gain.  wet < 0.0001: the summed input
 *      passes through untouched (a plain k_sum launch) and the state stays as it is.
 * State: (env, h, c), closed -- (0, 0, H + 1) -- at time 0; carried between consecutive block pulls and between the chunks of a
 * render, restarted from closed by td_graph_set_time / td_graph_change_time / td_graph_reset.
 * Ranges, rejected with a td_last_error that names the parameter (NaN included): threshold_db [-80, 0], hysteresis_db [0, 24],
 * hold_ms [0, 2000], attack_ms [0, 1000], release_ms [1, 10000], range_db [-120, 0].  `wet` is clamped to [0, 1].
 * Under "band_mode" 2 / "sine_mode" 2 everything upstream of a gate vertex takes the exact forms (no estimate is carried
 * through a gain that depends on the signal); vertices downstream are unaffected.
 * An external key input (ducking): td_graph_connect_key below.  Not part of the vertex: lookahead. */
int td_graph_add_gate(td_graph* g, const char* name, float gain, float angle, float wet, float threshold_db, float hysteresis_db,
                      float hold_ms, float attack_ms, float release_ms, float range_db);
/* Host only, no GPU: the gate vertex' constants at rate sr, exactly the doubles the engine uses -- out[0 .. 5] = To, Tc, H, aA,
 * aR, F.  The same range checks as td_graph_add_gate. */
int td_gate_params(size_t sr, float threshold_db, float hysteresis_db, float hold_ms, float attack_ms, float release_ms,
                   float range_db, double out[6]);
/* A phaser vertex: a swept all-pass chain with feedback -- THIS ENGINE'S OWN: no reference counterpart (the reference reaches
 * modulation effects only through LV2 plugins, add_lv2fx, which this engine parses and drops).  Per channel N
 * first-order all-pass sections in series (transposed direct form II) share one coefficient a[n], swept by the chorus' LFO
 * between the coefficients of lo_hz and hi_hz; the chain's output is fed back to its input.  The vertex sums its inputs like
 * every input vertex (sum_inputs, extensions.rs:310-319), processes, mixes with `wet` by the reference's f32 lerp, then pan and
 * gain like every vertex (extensions.rs:262-263).
 *   Constants, f64, once on the host, each from the f32 parameter widened to f64 (td_phaser_params returns them):
 *     N = stages;  g(fc) = (tan(pi fc / sr) - 1) / (tan(pi fc / sr) + 1);  a_lo = g(lo_hz);  a_hi = g(hi_hz);
 *     am = 0.5 (a_lo + a_hi);  ad = 0.5 (a_hi - a_lo);  f = rate_hz / sr;  fb = feedback.
 *   The sweep is linear in the all-pass COEFFICIENT, not in Hz: the device stays on IEEE add, multiply, floor and fabs (the
 *   chorus' rule), so a[n] is the same bits wherever it is computed.
 *   Per channel c, at the ABSOLUTE frame n (the graph's time, as for the chorus), phi = 0 on the left, phi = stereo on the
 *   right, in f64 with no FMA contraction, in the order written:
 *     th = n f + phi;  th = th - floor(th);  a = am + ad lfo(shape, th)       (lfo: td_graph_add_chorus' -- sine or triangle)
 *     xs = x[n] if finite, else 0;   v = xs + fb z
 *     for k = 1 .. N:   w = a v + s_k;   s_k = v - a w;   v = w
 *     z = v;   p[n] = (float)v
 *   Output: out = x + wet * (p - x) in f32 (adsr.rs:42); then pan and gain.  wet 0.5: the classic phaser, N / 2 moving notches;
 *   wet 1: a swept phase shift.  wet < 0.0001: the summed input passes through untouched (a plain k_sum launch) and the state
 *   stays as it is.
 * State: (s_1 .. s_N, z) per channel, f64, zero at time 0; carried between consecutive block pulls and between the chunks of a
 * render, restarted from zero by td_graph_set_time / td_graph_change_time / td_graph_reset.  The LFO never restarts: it is a
 * function of the graph's time.  No latency, no tail.
 * Ranges, rejected with a td_last_error that names the parameter (NaN included): stages 2 | 4 | 6 | 8; lo_hz >= 20; hi_hz <=
 * 0.45 sr; lo_hz <= hi_hz (equal: a static chain); rate_hz [0.01, 20]; feedback [-0.95, 0.95]; stereo [0, 0.5]; shape 0 .. 1
 * (TD_CHORUS_*).  `wet` is clamped to [0, 1].
 * Under "band_mode" 2 / "sine_mode" 2 everything upstream of a phaser vertex takes the exact forms: the vertex is linear but
 * time-varying with feedback, and no L2 bound of it is proven; vertices downstream are unaffected.
 * Not part of the vertex: an exponential (linear-in-Hz or in octaves) sweep law, tempo sync, more than 8 stages, barber-pole
 * forms. */
int td_graph_add_phaser(td_graph* g, const char* name, float gain, float angle, float wet, int stages, float lo_hz, float hi_hz,
                        float rate_hz, float feedback, float stereo, int shape);
/* Host only, no GPU: the phaser vertex' constants at rate sr, exactly the doubles the engine uses -- out[0 .. 6] = N, a_lo, a_hi,
 * am, ad, f, fb.  The same range checks as td_graph_add_phaser. */
int td_phaser_params(size_t sr, int stages, float lo_hz, float hi_hz, float rate_hz, float feedback, float stereo, int shape, double out[7]);
/* A vocoder vertex: a keyed band-pass bank (the channel vocoder) -- THIS ENGINE'S OWN: no reference counterpart (the reference
 * reaches it only through LV2 plugins, add_lv2fx, which this engine parses and drops).  The vertex sums its inputs
 * like every input vertex (sum_inputs, extensions.rs:310-319): that sum (l, r) is the CARRIER.  Its MODULATOR comes through key
 * edges (td_graph_connect_key below): the key frames (kl, kr) are the f32 sum of its key sources.  Without a key edge the vertex
 * uses its own summed input as modulator, (kl, kr) = (l, r), as an unkeyed compressor listens to itself -- so a vocoder keyed by
 * its own source is bit for bit the unkeyed one.
 *   Constants, f64, once on the host, each from the f32 parameter widened to f64 (td_vocoder_params returns them), B = bands:
 *     f_b = lo_hz (hi_hz / lo_hz)^(b / (B - 1)),  b = 0 .. B - 1;
 *     (b0, b1, b2, a1, a2)_b: the RBJ band-pass with constant 0 dB peak gain (td_graph_add_eq's TD_EQ_BANDPASS formulas) at
 *     frequency f_b (f64, not rounded to f32) and `q`;
 *     a = exp(-1 / (response_ms sr / 1000));  g = 10^(out_db / 20).
 *   Per frame n, in f64 on the f32 sums with no FMA contraction, in the order written.  A non-finite carrier sample enters as
 *   0 (the EQ's rule); a modulator frame with a NaN or infinite sample enters as m = 0 (the key frame's rule of
 *   td_graph_connect_key):
 *     1. m = 0.5 ((double)kl + (double)kr)
 *     2. for every band b, three biquads BP_b with the same coefficients and a state (s1, s2) each, in td_graph_add_eq's order
 *        y = b0 x + s1;  s1 = (b1 x - a1 y) + s2;  s2 = b2 x - a2 y:     cl_b = BP_b(l);  cr_b = BP_b(r);  km_b = BP_b(m)
 *     3. e_b = a e_b + (1 - a) |km_b|            (1 - a is rounded once; a rectifier and a one-pole low-pass: linear on purpose)
 *     4. sl = 0;  for b = 0 .. B - 1: sl = sl + e_b cl_b;   pl = (float)(g sl);   pr likewise from cr_b
 *   Output: out = x + wet * (p - x) in f32 (adsr.rs:42) -- a non-finite x comes out as what IEEE makes of it -- then pan and gain.
 *   wet < 0.0001: the summed input passes through untouched (a plain k_sum launch); the vertex ignores its key edges bit for
 *   bit and its state stays as it is.
 * State: seven doubles per band -- (s1, s2) of the three biquads, and e_b -- zero at time 0; carried between consecutive block
 * pulls and between the chunks of a render, restarted from zero by td_graph_set_time / td_graph_change_time / td_graph_reset.
 * No latency, no tail.
 * Ranges, rejected with a td_last_error that names the parameter (NaN included): bands 4 | 8 | 16; lo_hz >= 40; hi_hz <= 0.45 sr;
 * lo_hz < hi_hz; q [0.5, 20]; response_ms [0.1, 1000]; out_db [-24, 48].  `wet` is clamped to [0, 1].
 * Under "band_mode" 2 / "sine_mode" 2 everything upstream of a vocoder vertex that is not dry -- of its inputs and of its key --
 * takes the exact forms: the gain on the carrier is the modulator's envelope, no static bound of it exists.
 * Not part of the vertex: an unvoiced / sibilance path, a separate attack and release, formant shift, more than 16 bands. */
int td_graph_add_vocoder(td_graph* g, const char* name, float gain, float angle, float wet, int bands, float lo_hz, float hi_hz,
                         float q, float response_ms, float out_db);
/* Host only, no GPU: the vocoder vertex' constants at rate sr, exactly the doubles the engine uses -- out[6 b .. 6 b + 5] = f_b,
 * b0, b1, b2, a1, a2 for b = 0 .. bands - 1, then out[6 bands] = a, out[6 bands + 1] = g.  `cap`: the doubles `out` holds, at least
 * 6 bands + 2.  The same range checks as td_graph_add_vocoder. */
int td_vocoder_params(size_t sr, int bands, float lo_hz, float hi_hz, float q, float response_ms, float out_db, double* out, size_t cap);
/* A filter vertex: a resonant state-variable filter whose cutoff is swept by an LFO and by an envelope follower -- THIS ENGINE'S
 * OWN: no reference counterpart (add_bandpass and td_graph_add_eq have fixed coefficients).  The vertex sums its
 * inputs like every input vertex (sum_inputs, extensions.rs:310-319), processes the sum (l, r), mixes with `wet` by the
 * reference's f32 lerp, then pan and gain like every vertex (extensions.rs:262-263).  Everything below is f64 on the f32 sums,
 * with no FMA contraction, in the order written.
 *   Constants, once on the host, each from the f32 parameter widened to f64 (td_filter_params returns exactly these):
 *     g0 = tan(pi freq_hz / sr);  k = 1 / q;  gmin = tan(pi 20 / sr);  gmax = tan(0.45 pi);
 *     cl = ln2 lfo_oct;  ce = ln2 env_oct;  f = rate_hz / sr;  S = 10^(sens_db / 20);
 *     aA = exp(-1 / (attack_ms sr / 1000)), 0 for attack_ms = 0;  aR likewise from release_ms.
 *   Per frame, at the ABSOLUTE frame n (the graph's time, as for the chorus and the phaser):
 *     1. Level, stereo-linked, in the linear domain (the compressor's steps 1, 3 and 4).  The key frame (kl, kr) is the f32 sum of
 *        the vertex' key sources (td_graph_connect_key below); without a key edge (kl, kr) = (l, r), as an unkeyed compressor
 *        listens to itself.
 *          s[n] = max(|kl|, |kr|), and 0 for a key frame with a NaN or an infinity
 *          y1[n] = max(s[n], aR y1[n-1])
 *          e[n] = aA e[n-1] + (1 - aA) y1[n]                              (1 - aA is rounded once)
 *     2. Control, per channel c: phi = 0 on the left, phi = stereo on the right
 *          th = n f + phi;  th = th - floor(th)
 *          t = cl lfo(shape, th) + ce min(S e[n], 1)       (lfo: td_graph_add_chorus' -- sine or triangle; there is no second LFO)
 *     3. Cutoff.  The sweep is exponential: octaves of the prewarped coefficient g, which are octaves of Hz below about sr / 8.
 *          g = min(max(g0 E(t), gmin), gmax)
 *        E(t) is this FIXED sequence of IEEE multiplies and adds -- no libm call runs on the device; every implementation computes
 *        the same E(t) from the same t:
 *          x = t 0.0625;  p = 1;  for j = 10 down to 1: p = 1 + p (x c_j);  then four times: p = p p;  E = p
 *          c_j is the double nearest 1 / j: c_10 = 0.1, c_9 = 0.1111111111111111, c_8 = 0.125, c_7 = 0.14285714285714285,
 *          c_6 = 0.16666666666666666, c_5 = 0.2, c_4 = 0.25, c_3 = 0.3333333333333333, c_2 = 0.5, c_1 = 1.
 *        Over |t| <= 10.5 it is within 7.2e-9 relative of exp(t); the ranges below keep |t| <= 12 ln2 = 8.32.
 *     4. The filter: the trapezoidal (zero-delay-feedback) state-variable filter, per channel, state (i1, i2).  xs = x[n] if
 *        finite, else 0.
 *          a1 = 1 / (1 + g (g + k));  a2 = g a1;  a3 = g a2                   (one correctly rounded f64 division)
 *          v3 = xs - i2;  v1 = a1 i1 + a2 v3;  v2 = (i2 + a2 i1) + a3 v3
 *          i1 = 2 v1 - i1;  i2 = 2 v2 - i2
 *          low-pass p = v2;  band-pass p = k v1 (0 dB peak);  high-pass p = (xs - k v1) - v2;  notch p = xs - k v1
 *          p[n] = (float)p
 *     5. Output: out = x + wet * (p - x) in f32 (adsr.rs:42) -- a non-finite x[n] comes out as what IEEE makes of it, at that
 *        frame only -- then pan and gain.  wet < 0.0001: the summed input passes through untouched (a plain k_sum launch), the
 *        state stays as it is and key edges are ignored bit for bit.
 * State: (y1, e, i1l, i2l, i1r, i2r), six doubles, zero at time 0; carried between consecutive block pulls and between the chunks
 * of a render, restarted from zero by td_graph_set_time / td_graph_change_time / td_graph_reset.  The LFO never restarts: it is a
 * function of the graph's time.  No latency, no tail.
 * env_oct == 0: the detector is not run -- y1 and e stay as they are, key edges are ignored, and the output is bit for bit that
 * of the same vertex without them.
 * Ranges, rejected with a td_last_error that names the parameter (NaN and the infinities included): kind 0 .. 3 (TD_FILTER_*);
 * freq_hz [20, 0.45 sr]; q [0.5, 30]; lfo_oct [0, 4]; rate_hz [0.01, 20]; stereo [0, 0.5]; shape 0 .. 1 (TD_CHORUS_*); env_oct
 * [-8, 8]; sens_db [0, 60]; attack_ms [0, 1000]; release_ms [1, 10000].  `wet` is clamped to [0, 1].
 * Under "band_mode" 2 / "sine_mode" 2 everything upstream of a filter vertex that is not dry takes the exact forms, and so does
 * everything upstream of a key edge into one whose follower runs: the resonance gain follows the signal and the time, and no
 * static bound of it is proven; vertices downstream are unaffected.
 * Not part of the vertex: a ladder or other topology, slopes beyond 12 dB / octave (two vertices in series give 24), tempo sync,
 * a per-note envelope, audio-rate modulation of the cutoff. */
enum { TD_FILTER_LOWPASS = 0, TD_FILTER_HIGHPASS = 1, TD_FILTER_BANDPASS = 2, TD_FILTER_NOTCH = 3 };
int td_graph_add_filter(td_graph* g, const char* name, float gain, float angle, float wet, int kind, float freq_hz, float q,
                        float lfo_oct, float rate_hz, float stereo, int shape,
                        float env_oct, float sens_db, float attack_ms, float release_ms);
/* Host only, no GPU: the filter vertex' constants at rate sr, exactly the doubles the engine uses -- out[0 .. 10] = g0, k, gmin,
 * gmax, cl, ce, f, S, aA, 1 - aA, aR.  `cap`: the doubles `out` holds, at least 11.  The same range checks as
 * td_graph_add_filter. */
int td_filter_params(size_t sr, int kind, float freq_hz, float q, float lfo_oct, float rate_hz, float stereo, int shape,
                     float env_oct, float sens_db, float attack_ms, float release_ms, double* out, size_t cap);
/* A limiter vertex: a lookahead brickwall limiter -- THIS ENGINE'S OWN: no reference counterpart.  It is the
 * limiter of td_graph_master (below) in causal form, inside the graph: on a bus, on a stem, in a block pull.  The vertex sums its
 * inputs like every input vertex (sum_inputs, extensions.rs:310-319), processes the sum (l, r), mixes with `wet` by the
 * reference's f32 lerp, then pan and gain like every vertex (extensions.rs:262-263).
 *   Constants, f64, once on the host, each from the f32 parameter widened to f64 (td_limiter_params returns exactly these):
 *     c = 10^(ceiling_db / 20);  gin = 10^(drive_db / 20);  L = max(1, llround(lookahead_ms sr / 1000)) frames;
 *     a = exp(-1 / (release_ms sr / 1000)).
 *   Per frame n, on the f32 summed input with no FMA contraction, in the order written.  Frames before the restart time (time 0,
 *   or the last td_graph_set_time) count as 0:
 *     1. s[n] = max(|l[n]|, |r[n]|) as f32 (exact); a frame with a NaN or an infinite sample has s = 0: it stays out of the state
 *     2. Q[n] = max of s over [n - L + 1, n]                                  (f32, exact in any order)
 *     3. d = gin (double)Q[n];  h[n] = c / d if d > c, else 1
 *     4. u[n] = max(1 - h[n], a u[n-1]), u = 0 at the restart;  e[n] = 1 - u[n];  frames before the restart have e = 1
 *     5. G[n] = (sum of e over [n - L + 1, n]) / (double)L
 *     6. xd[n] = x[n - L + 1], the raw f32 input;  p = (float)(((double)xd gin) G[n]) per channel;
 *        out = xd + wet * (p - xd) in f32 (adsr.rs:42); then pan and gain.
 *   The engine forms the sum of step 5 as a difference of f64 prefix sums of e taken in a fixed order, so a render is bitwise
 *   reproducible; it differs from the serial sum by rounding alone (DESIGN.md 3x gives the bound).
 *   wet < 0.0001: the summed input passes through untouched and UNDELAYED (a plain k_sum launch) and the state stays as it is.
 * Latency: the vertex delays its signal by L - 1 frames (td_limiter_params returns the figure).  Nothing compensates for it
 * elsewhere in the graph -- the saturator's rule.  L = 1 is an instantaneous limiter with no latency.
 * What the definition guarantees:
 *   every e[j] in the window of frame n was formed from a Q[j] that contains frame n - L + 1, so gin |xd[n]| G[n] <= c: no
 *   output sample of the wet path exceeds the ceiling, up to its one f32 rounding;
 *   when nothing exceeds the ceiling G is exactly 1: the wet path is then the input times gin, delayed.
 * State: zero at time 0.  u at the last frame, the last L - 1 raw input frames and the last L - 1 values of e (the engine keeps
 * e itself, not the further input it could be rebuilt from); carried between consecutive block pulls and between the chunks of
 * a render, restarted by td_graph_set_time / td_graph_change_time / td_graph_reset.
 * Ranges, rejected with a td_last_error that names the parameter (NaN and the infinities included): ceiling_db [-24, 0];
 * drive_db [-24, 24]; lookahead_ms [0, 50] and L <= 2048 frames (the error names lookahead_ms too); release_ms [1, 10000].
 * `wet` is clamped to [0, 1].
 * Under "band_mode" 2 / "sine_mode" 2 everything upstream of a limiter vertex that is not dry takes the exact forms: the gain
 * depends on the signal, the compressor's case; vertices downstream are unaffected.  td_graph_connect_key refuses a limiter.
 * Not part of the vertex: true-peak (oversampled) detection, which td_graph_master has; a key input; a gain-reduction read-out;
 * latency compensation across the graph; a tail past the project's end (the last L - 1 input frames are not played out). */
int td_graph_add_limiter(td_graph* g, const char* name, float gain, float angle, float wet, float ceiling_db, float lookahead_ms,
                         float release_ms, float drive_db);
/* Host only, no GPU: the limiter vertex' constants at rate sr, exactly the doubles the engine uses -- out[0 .. 4] = c, gin, L, a,
 * latency (L - 1 frames).  The same range checks as td_graph_add_limiter. */
int td_limiter_params(size_t sr, float ceiling_db, float lookahead_ms, float release_ms, float drive_db, double out[5]);
/* A multiband vertex: a three-way Linkwitz-Riley crossover into three band compressors -- THIS ENGINE'S OWN: no reference
 * counterpart (the reference reaches it only through LV2 plugins, add_lv2fx, which this engine parses and drops).
 * With one band working it is a de-esser.  The vertex sums its inputs like every input vertex (sum_inputs,
 * extensions.rs:310-319); everything below is f64 on the f32 summed input (l, r), per channel, with no FMA contraction, in the
 * order written.  Bands are in the order low, mid, high (b = 0, 1, 2) wherever three values stand together.
 *   1. Coefficients, f64, once on the host, from the f32 parameters widened to f64 (td_multiband_params returns them); Q =
 *      sqrt(0.5) throughout.  L1 and H1: the RBJ low-pass and high-pass (td_graph_add_eq's TD_EQ_LOWPASS / TD_EQ_HIGHPASS formulas)
 *      at lo_hz; L2 and H2: those at hi_hz; A2: the RBJ all-pass at hi_hz, b = (1 - alpha, -2 cos w0, 1 + alpha) / (1 + alpha)
 *      with the same a1 and a2 as L2.  aR = exp(-1 / (release_ms sr / 1000)), aA likewise from attack_ms (0 for attack_ms = 0).
 *   2. Crossover: Linkwitz-Riley, 24 dB per octave.  Every section is td_graph_add_eq's transposed direct form II in its
 *      operation order, y = b0 u + s1;  s1 = (b1 u - a1 y) + s2;  s2 = b2 u - a2 y, with a state (s1, s2) of its own:
 *        low = A2(L1(L1(x)));  rest = H1(H1(x));  mid = L2(L2(rest));  high = H2(H2(rest))
 *      -- nine biquads per channel, in that order.  A non-finite input sample enters as 0 (the EQ's rule) and reaches the output
 *      through the dry leg of the lerp only.  A2 on the low band makes low + mid + high an all-pass of x.
 *   3. Per band b, td_graph_add_compressor's steps 1 - 4 with the band's own T_b = threshold_db[b], R_b = ratio[b], M_b =
 *      makeup_db[b] and the shared knee W, aA and aR, on the level s_b[n] = max(|l_b[n]|, |r_b[n]|) of the f64 band signals
 *      (zero or not finite: d_b = 0):  d_b from 20 log10 s_b - T_b;  y1_b = max(d_b, aR y1_b);  yL_b = aA yL_b + (1 - aA) y1_b;
 *      G_b = 10^((M_b - yL_b) / 20).
 *   4. p = (float)(((0.0 + low G_0) + mid G_1) + high G_2) per channel, rounded once; out = x + wet * (p - x) in f32
 *      (adsr.rs:42); then pan and gain.
 *   wet < 0.0001: the summed input passes through untouched (a plain k_sum launch) and the state stays as it is.
 * State: 42 doubles -- (s1, s2) of the 18 biquads and (y1, yL) of the three bands -- zero at time 0; carried between consecutive
 * block pulls and between the chunks of a render, restarted from zero by td_graph_set_time / td_graph_change_time /
 * td_graph_reset.  No latency, no tail.  No key input: td_graph_connect_key refuses a multiband ("takes no key input").
 * Ranges, rejected with a td_last_error that names the parameter and starts "multiband:" (NaN fails every comparison):
 * lo_hz >= 40; hi_hz <= 0.45 sr; hi_hz >= 2 lo_hz; per band threshold_db [-60, 0]; and the compressor's own for ratio [1, 1000],
 * attack_ms [0, 1000], release_ms [1, 10000], knee_db [0, 40], makeup_db [-40, 40].  `wet` is clamped to [0, 1].
 * Under "band_mode" 2 / "sine_mode" 2 everything upstream of a multiband vertex that is not dry takes the exact forms: the gains
 * depend on the signal, the compressor's case; vertices downstream are unaffected.
 * Not part of the vertex: a key input; more than three bands, or two; per-band attack / release / knee; linear-phase
 * crossovers; lookahead. */
int td_graph_add_multiband(td_graph* g, const char* name, float gain, float angle, float wet, float lo_hz, float hi_hz,
                           const float threshold_db[3], const float ratio[3], float attack_ms, float release_ms, float knee_db,
                           const float makeup_db[3]);
/* Host only, no GPU: the multiband vertex' constants at rate sr, exactly the doubles the engine uses -- out[5 s .. 5 s + 4] = (b0,
 * b1, b2, a1, a2) of set s = L1, H1, L2, H2, A2, then out[25] = aA, out[26] = aR.  `n`: the doubles `out` holds, at least 27.  The
 * same range checks as td_graph_add_multiband. */
int td_multiband_params(size_t sr, float lo_hz, float hi_hz, const float threshold_db[3], const float ratio[3], float attack_ms,
                        float release_ms, float knee_db, const float makeup_db[3], double* out, size_t n);
/* A convolution vertex: an impulse response from the sample bank, applied by FFT -- THIS ENGINE'S OWN: no reference counterpart
 * (the reference reaches it only through LV2, add_lv2fx).  A room or plate response, a speaker cabinet, a measured
 * linear-phase filter: any WAV that td_samplebank_add / load_sample brought into the bank at the project's rate.  The vertex sums its
 * inputs like every input vertex (sum_inputs, extensions.rs:310-319), processes the sum x = (l, r), mixes with `wet` by the
 * reference's f32 lerp, then pan and gain like every vertex (extensions.rs:262-263).  It takes no key.
 *   The response: h_c[k], c = left or right, is the bank's sample at `sample_index`, exactly the f32 frames td_samplebank_read returns.
 *     Lh = sample_len if length_ms == 0, else min(sample_len, llround(length_ms sr / 1000)) frames of it are used; 1 <= Lh <= 262144:
 *     a longer response is an error that names length_ms, raised where the bank is first seen -- by the render, by
 *     td_convolution_params, and by a project script's refresh.
 *   Pre-delay and trim, f64, from the f32 parameters widened (td_convolution_params returns exactly these):
 *     D = llround(predelay_ms sr / 1000) frames;  g = 10^(out_db / 20).
 *   norm = 1 divides g by sqrt(max_c sum_k h_c[k]^2), the sums in f64 over the Lh frames used, so that white noise leaves at the
 *     RMS it came in at.  An all-zero response with norm = 1 is an error that names norm, raised by the render that first sees it.
 *   The wet path, in f64 on the f32 summed input:  p_c[n] = (float)(g sum_{k < Lh} h_c[k] x_c[n - D - k]); x is 0 before the
 *     restart time (time 0, or the last td_graph_set_time).  The left response acts on the left channel, the right on the right.  A
 *     NaN or infinite input sample enters the sum as 0 (and passes to the output through the mix alone).
 *   The mix, f32:  out = x + wet (p - x) (adsr.rs:42), then pan and gain.  The dry path is NOT delayed.
 *   The engine forms the sum by uniform-partitioned overlap-save with f64 transforms in a fixed order, so a render is bitwise
 *   reproducible; it differs from the direct sum by rounding alone (DESIGN.md 3z gives the bound), and a render cut into chunks or
 *   block pulls from the same render in one piece by that rounding too.
 *   wet < 0.0001: the summed input passes through untouched (a plain k_sum launch) and the state stays as it is.
 * State: the last D + Lh - 1 summed input frames, zero at time 0; carried between consecutive block pulls and between the chunks
 * of a render, restarted by td_graph_set_time / td_graph_change_time / td_graph_reset.  When the bank's sample behind the index is
 * replaced by one of another length the vertex restarts from silence.
 * Ranges, rejected with a td_last_error that names the parameter (NaN and the infinities included): length_ms [0, 60000];
 * predelay_ms [0, 500]; out_db [-60, 24]; norm 0 or 1.  `wet` is clamped to [0, 1].
 * Under "band_mode" 2 / "sine_mode" 2 everything upstream of a convolution vertex that is not dry takes the exact forms: its gain is
 * the peak of the response's spectrum, which the host does not hold; vertices downstream are unaffected.  td_graph_connect_key
 * refuses a convolution vertex.
 * Not part of the vertex: a tail past the project's end; a true-stereo (four-channel) response; resampling of the response at
 * render time (the bank holds it at the project's rate); a spectra ring that would spare block pulls the transforms of the
 * carried frames (every pull transforms them again). */
int td_graph_add_convolution(td_graph* g, const char* name, float gain, float angle, float wet, size_t sample_index, float length_ms,
                             float predelay_ms, float out_db, int norm);
/* Host only, no GPU: the convolution vertex' constants at rate sr for a sample of sample_len frames -- out[0 .. 5] = Lh, D, g
 * (before norm), P = ceil((D + Lh) / B) partitions, the carried frames D + Lh - 1, B (the partition, 1024 frames).  The same range
 * checks as td_graph_add_convolution, and the response's length. */
int td_convolution_params(size_t sr, size_t sample_len, float length_ms, float predelay_ms, float out_db, int norm, double out[6]);
/* Host only: the twiddle table of the engine's transforms, (cos, -sin)(2 pi j / 2048) for j = 0 .. 1023 as 2048 doubles, computed
 * in long double -- the table the kernels read.  Returns 2048; writes only when cap >= 2048. */
size_t td_convolution_twiddles(double* out, size_t cap);
int td_graph_connect(td_graph* g, const char* a, const char* b);          /* graph.rs:80-96 (+58-78) */
/* A key edge (sidechain) from any vertex `a` to a compressor, gate, vocoder or filter vertex `b` -- THIS ENGINE'S OWN, like the
 * vertices.  A vocoder vertex takes its MODULATOR from the key frames defined here (td_graph_add_vocoder above), a filter vertex
 * the LEVEL its envelope follows (td_graph_add_filter above; ignored when its env_oct is 0); for the other two: a
 * vertex with at least one key edge takes its LEVEL from the sum of its key sources; everything else is as without: it processes
 * the sum of its inputs, carries the same state, keeps its wet mix, pan and gain.
 *   The key frames (kl[n], kr[n]) are the f32 sum of the key sources' outputs, each with its own pan and gain applied, summed in
 *   connect_key order by the arithmetic of sum_inputs (extensions.rs:310-319, as every input sum here); a duplicate key edge is
 *   summed twice.  They are summed per chunk / block pull: nothing new is carried.
 *   With one or more key edges, step 1 of the compressor (the level s[n], and through it d[n]) and steps 1 and 2 of the gate (the
 *   level and its class against To / Tc) read (kl, kr) where they read (l, r).  The NaN / infinite-frame rule is applied to the
 *   key frame: such a key frame stays out of the compressor's state (d[n] = 0), or forces nothing in the gate's step 2.  Every
 *   later step is unchanged and acts on the summed INPUT: a non-finite input frame comes out as what IEEE makes of it.
 *   A key is not an input: td_graph_check's "output receives no inputs" is unchanged, and a keyed vertex without inputs
 *   processes silence.  A dry vertex (wet < 0.0001) ignores its key edges: its output is bit for bit that of the same vertex
 *   without them.
 * Returns 0 (td_last_error) for an unknown name (td_graph_connect's messages); when `b` is not a compressor, gate, vocoder or filter vertex
 * ("connect_key: <b> takes no key input"); when the edge would close a loop.  The loop test of td_graph_connect and of
 * td_graph_connect_key runs over the union of input and key edges.  td_graph_reset clears key edges, as it clears edges.  A key
 * source is rendered like an input, also when only the key edge reaches it.
 * Under "band_mode" 2 / "sine_mode" 2 everything upstream of a key edge into a vertex that is not dry takes the exact forms (the
 * level decides a gain: no estimate is carried through it); a dry keyed vertex contributes nothing. */
int td_graph_connect_key(td_graph* g, const char* a, const char* b);
int td_graph_set_output(td_graph* g, const char* vertex);                 /* graph.rs:141-148 */
int td_graph_check(const td_graph* g);                                    /* check_graph graph.rs:150-174 */
void td_graph_set_time(td_graph* g, size_t time);                         /* graph.rs:123-128 */
size_t td_graph_change_time(td_graph* g, size_t delta, int plus);         /* graph.rs:130-135 */
size_t td_graph_get_time(const td_graph* g);                              /* graph.rs:137-139 */
void td_graph_reset_normalize_vertices(td_graph* g);                      /* graph.rs:207-211 */
float td_graph_get_normalization_value(const td_graph* g, const char* name); /* extensions.rs:301-307 */
size_t td_graph_vertex_count(const td_graph* g);

/* Graph::render graph.rs:182-193: renders ONE block at the current playhead, advances the playhead by
 * max_buffer_len, copies the output vertex' block to l / r (max_buffer_len floats each, either may be
 * NULL).  Returns 1 = Some(block), 0 = no output vertex (the reference's None), -1 = failure (td_last_error).
 * Like the reference it does not advance the FlowwBank -- the caller does (state.rs:572). */
int td_graph_render_block(td_graph* g, const td_samplebank* sb, td_flowwbank* fb, float* l, float* r);

/* Graph::true_normalize_scan graph.rs:222-237 over `chunks` blocks (whole timeline on the GPU). */
int td_graph_normalize_scan(td_graph* g, const td_samplebank* sb, td_flowwbank* fb, size_t chunks);

/* The accelerated entry: the body of State::render's loop (state.rs:562-575) for `n_blocks` blocks --
 * n_blocks x { Graph::render; quantise (x*amplitude) as i16|i32 (state.rs:515-532); fb.set_time_to_next_block }
 * then Graph::set_time(0).  The whole timeline is rendered by one kernel per vertex batch; the
 * result stays in HBM.  bits in {8,16,24,32}: <= 16 -> int16 words, otherwise int32 words, exactly the
 * integers the reference hands to hound.  Returns the number of frames rendered (0 on failure). */
size_t td_graph_render_all(td_graph* g, const td_samplebank* sb, td_flowwbank* fb, size_t n_blocks, int bits);
/* The `psr > render_sr` arm of State::render (state.rs:533-561): the same render followed by a down-sample
 * of the whole timeline from psr to render_sr and the quantise.  The reference streams the un-vendored
 * rubato resampler block by block; this engine uses its own documented sinc resampler with rubato's
 * parameter set (DESIGN.md "Resampler") -- parity with the reference is unpinned.  Returns output frames. */
size_t td_graph_render_all_resampled(td_graph* g, const td_samplebank* sb, td_flowwbank* fb, size_t n_blocks, int bits,
                                     size_t psr, size_t render_sr);
/* Device-resident results of the last td_graph_render_all (valid until the next render on g).  After the ASYNC forms the
 * contents are final only once td_graph_sync / td_batch_sync has returned: those settle what a render may have left
 * pending -- the single-pass Normalize's deferred check, the guard's verdict of "band_mode" 2 -- which a plain stream or
 * device synchronisation of the caller's own does not. */
const void* td_graph_output_pcm_device(const td_graph* g);    /* int16|int32 interleaved, frames*2 words */
const float* td_graph_output_f32_device(const td_graph* g);   /* float2 per frame, un-quantised output vertex */
/* D2H copies of the above (pcm: frames*2 words of 2 or 4 bytes; f32: frames*2 floats). */
int td_graph_read_pcm(const td_graph* g, void* out, size_t bytes);
int td_graph_read_f32(const td_graph* g, float* out, size_t n_floats);
/* Per-block absolute peak of the last render's un-quantised output (n_blocks floats) reduced on the
 * device to one float: used for the per-project peak table of the multi-GPU batch. */
float td_graph_output_peak(const td_graph* g);
/* Stems: vertices rendered to PCM of their own beside the output, in the same render.  Stem X of a render is what the render
 * would give with set_output(X) (graph.rs:141-148): X and everything upstream of it are computed, reaching the output or not,
 * exactly as that render would compute them.  The renders td_graph_render_all, _async and _resampled write every stem at the
 * output's bit depth, frame count and (resampled) rate; td_graph_render_block ignores the stems (block pulls compute the
 * output's plan alone: with stems set, every pull re-plans twice -- to the output's plan and back -- and settles a guarded
 * verdict still out first), and a td_batch render fails while a member graph has stems set.  A stem may sit downstream of
 * the output: the output's f32 frames are then kept whatever "output_f32" says.  Under the guarded modes ("band_mode"
 * 2, "sine_mode" 2) everything upstream of a stem other than the output takes the exact kernels.
 * td_graph_set_stems replaces the list (n = 0 clears it; td_graph_reset clears it too); an unknown or repeated name -> 0 and
 * the list unchanged.  A stem may name the output vertex: its bytes are then the output's. */
int td_graph_set_stems(td_graph* g, const char* const* names, size_t n);
size_t td_graph_stem_count(const td_graph* g);
/* Stem i of the last render: interleaved, the same words as td_graph_output_pcm_device (NULL: not rendered). */
const void* td_graph_stem_pcm_device(const td_graph* g, size_t i);
int td_graph_read_stem_pcm(const td_graph* g, size_t i, void* out, size_t bytes);
/* max |x| over the frames of stem i quantised in the last render (a NaN frame: NaN). */
float td_graph_stem_peak(const td_graph* g, size_t i);
/* Loudness of the last whole render (td_graph_render_all, _async, _resampled): ITU-R BS.1770-4 with the gating of EBU Tech 3341
 * and the loudness range of EBU Tech 3342.  The reference has no counterpart (its README lists a LUFS mastering tool under
 * "Goals for later").  What is measured is the PCM td_graph_read_pcm returns -- at the render's rate and bit depth, each word
 * scaled by 1 / 2^(bits-1) as a WAV reader scales it -- so the figures are a file meter's on the WAV td_state_render writes; the
 * graph is settled first as the read functions settle it (the deferred Normalize check, a guarded verdict).  Channels L and R,
 * weight 1.0 each; K-weighting from zero state at frame 0; hops of round(rate / 10) frames, whole hops only.  Eight doubles per
 * signal: [0] integrated LUFS, [1] momentary max LUFS, [2] short-term max LUFS, [3] loudness range LU, [4] true peak dBTP,
 * [5] sample peak dBFS, [6] frames measured, [7] sample rate.  Silence: -inf loudness and peaks, LRA 0; fewer than 4 hops:
 * integrated and momentary -inf; a NaN frame: [0]..[5] NaN.  DESIGN.md §3k gives the definitions, the filters and the kernel.
 * td_graph_loudness: n signals -- 0 the output, 1 + i stem i of the same render -- in ONE k_loudness launch; fails when there is
 * no whole render or n > 1 + the stems the render wrote.  The figures are bitwise reproducible. */
int td_graph_loudness(td_graph* g, double* out, size_t n);
/* The 400 ms block series (LUFS, one block per hop from hop 3 on) of signal `which` of the last td_graph_loudness: copies up to
 * cap values (out may be NULL) and returns the count; 0 and td_last_error when there is no such signal. */
size_t td_graph_momentary(const td_graph* g, size_t which, double* out, size_t cap);
/* The same meter over interleaved host frames (f32, L R), measured on the device: frames * 2 floats at rate sr. */
int td_loudness_f32(const float* lr, size_t frames, size_t sr, double out[8]);
/* Host only, no GPU: the meter's filters at rate sr -- kw: the K-weighting shelf b0 b1 b2 a1 a2 then high-pass b0 b1 b2 a1 a2
 * (a0 = 1); fir: the true-peak interpolator, *phases x *taps floats phase-major (phase 0 the unit impulse; 4 phases below 96 kHz,
 * 2 below 192 kHz, else 1).  fir may be NULL to ask for the sizes; a fir of capacity cap too small fails. */
int td_loudness_filters(size_t sr, double kw[10], float* fir, size_t cap, size_t* phases, size_t* taps);
/* Loudness mastering of the last whole render to a target integrated loudness T (LUFS, [-60, 0]) under a true-peak ceiling
 * C (dBTP, [-30, 0]; c = 10^(C/20)): gain plus a lookahead brickwall limiter.  No reference counterpart (its README lists a
 * "Lufs mastering tool" under "Goals for later"); DESIGN.md §3l.  Input x[n][c]: td_graph_loudness's signal -- the render's
 * words scaled by 1 / 2^(bits-1) at its rate fs (after _resampled) -- or the caller's f32 frames (td_master_f32).
 * Lookahead (ms, [0.1, 100], default 5): W = max(1, round(lookahead fs / 1000)) frames, half away from zero.  Release (ms,
 * [1, 10000], default 100): a = exp(-1 / (release fs / 1000)).  One pass at gain g under the internal ceiling c':
 *   1. p[n] = max over both channels of |x[n]| and of the meter's interpolated points at m + k/P (k = 1 .. P-1; the f32 FMA
 *      chain over the 12 taps of its FIR in tap order, x = 0 outside [0, N)) for m = n and m = n - 1: bitwise the meter's points.
 *   2. q[n] = max of p over [n, n + W - 1] (j < N).       3. h[n] = min(1, c' / (g q[n])); h = 1 where q = 0.
 *   4. e[n] = min(h[n], 1 - a (1 - e[n-1])), e[-1] = 1 (u = 1 - e: u[n] = max(1 - h[n], a u[n-1]), a parallel scan), in f64.
 *   5. G[n] = (1/W) sum of e[k] over k = n-W+1 .. n, in f64, with e[k < 0] = e[0] (the limiter settled on the opening peak):
 *      every e in the window of frame n is at most c' / (g p[n]), so every sample point stays under c'.
 *   6. words: saturate(trunc(w g G[n])) in f64 on the integer word w, to [-2^(bits-1), 2^(bits-1) - 1] (unity gain: the
 *      identity); f32: (float)(x g G[n]).
 * The pass loop (double, from the meter's figures): measure the input, L_in (-inf or NaN: "master: nothing to master");
 * g1 = 10^((T - L_in)/20), c'1 = c.  After pass k: done when |I_k - T| <= 0.1 LU and TP_k <= C; else g *= 10^((T - I_k)/20)
 * and, when TP_k > C, c' *= 10^((C - TP_k - 0.01)/20).  At most 4 passes aim at both; if pass 4 is still over C one more pass
 * runs with g held and c' corrected, and if that is still over C the call fails and the rendered words are put back.  Missing
 * the loudness target is not an error: report [14] says so.
 * Report, TD_MASTER_FIELDS doubles per signal: [0..7] the meter's figures of the mastered signal (bitwise what
 * td_graph_loudness returns right after), [8] input integrated LUFS, [9] input true peak dBTP, [10] the last pass' g,
 * [11] its c' (linear), [12] min over n of G (as f32; 1.0 when the limiter never engaged), [13] passes run, [14] 1 when both
 * targets were met.
 * td_graph_master masters in place: the first call after a render keeps the output's words (device to device) and every call
 * until the next render or td_graph_reset masters from that copy, so calls never compound.  Afterwards td_graph_read_pcm,
 * td_graph_output_pcm_device, td_graph_loudness and the State's file see the mastered words; the stems, the f32 output and
 * td_graph_output_peak stay as rendered.  The graph is settled first (as td_graph_loudness); no whole render fails. */
#define TD_MASTER_FIELDS 15
int td_graph_master(td_graph* g, double target_lufs, double ceiling_dbtp, double lookahead_ms, double release_ms, double* out);
/* The same interleaved f32 frames (L R) from the host, measured and mastered on the device: out_lr gets frames * 2 floats,
 * untouched when the call fails. */
int td_master_f32(const float* lr, size_t frames, size_t sr, double target_lufs, double ceiling_dbtp, double lookahead_ms,
                  double release_ms, float* out_lr, double* out);
/* Timing hook for bench.py: enqueue one full render on the graph's stream without the final host
 * synchronisation (td_graph_sync waits).  Same work as td_graph_render_all. */
size_t td_graph_render_all_async(td_graph* g, const td_samplebank* sb, td_flowwbank* fb, size_t n_blocks, int bits);
int td_graph_sync(td_graph* g);
/* How often a single-pass Normalize launch of this graph (or of the batch it belongs to) had to be redone by the check
 * kernel after the fact: a tile of the launch gave up its bounded wait for an earlier tile's running peak -- another
 * process or stream kept part of the grid off the device -- and td_graph_sync / td_batch_sync / the read functions then
 * ran k_norm_fix before returning.  The results are the same either way; nothing in the library traps or waits without
 * bound on work that may not be running.  0 in normal operation. */
size_t td_graph_norm_fix_runs(const td_graph* g);
/* (tests, tuning) How many reference blocks the single-pass Normalize launches of this graph (or of the batch it belongs to)
 * stored a SECOND time since the last call: a tile of the wide sum kernel may scale and store with the earlier tiles' peaks it
 * can see before it waits for the rest, and stores a block again where the running peak came out differently.  Counted only
 * while engine option debug.norm has bit 2 or bit 4 set (the launch carries no atomic otherwise); waits for the stream. */
size_t td_graph_norm_respec(td_graph* g);
/* HIP-event timing of the launches of the last render, per kernel family (ms).  names/ms are parallel
 * arrays of capacity cap; returns the number of entries. Enabled by td_graph_set_profiling(g, n): n = 1
 * times every render, n > 1 every n-th render only (the events themselves cost a few us per launch), 0 off. */
void td_graph_set_profiling(td_graph* g, int on);
size_t td_graph_last_kernel_times(const td_graph* g, const char** names, float* ms, size_t* launches, size_t cap);
/* Host-side time spent inside the renders since the last reset, by phase (ms): [0] event compile (cursor /
 * voice bookkeeping -> tables), [1] descriptor build, [2] table upload, [3] kernel launches.  Returns the
 * number of chunks accumulated. */
size_t td_graph_host_times(td_graph* g, double* ms4, int reset);
/* HBM bytes allocated for edge buffers / tables by this graph handle. */
size_t td_graph_device_bytes(const td_graph* g);
/* Device and page-locked memory given back by freed handles stays with the process and is handed out again to the next handle
 * that asks for a block of that size (no reference counterpart; budget: environment TD_ALLOC_CACHE_MB, default 2048, 0 = off;
 * DESIGN.md 3 "Memory").  td_trim_memory gives everything on the free lists back to the driver now; td_cached_memory_bytes
 * says how much is there. */
void td_trim_memory(void);
/* Diagnostic (no reference counterpart): out[i] = the engine's sine of in[i], evaluated on the device -- sine_mode 1: glibc's sinf
 * restated (what debug_sine / synth use under engine option "sine_mode" 1; tests compare it with the host's sinf on all 2^32 bit patterns), 0: the tolerance-class sine.  Host pointers, n values; 1 = done. */
int td_device_sinf(const float* in, float* out, size_t n, int sine_mode);
size_t td_cached_memory_bytes(void);
/* Engine options (no reference counterpart).  SEVEN supported keys:
 * "fuse_sources" 0|1 (default 1: sample_loop sources are gathered inside the consuming sum kernel instead of through an edge
 *   buffer -- same values, same order; 0 = SURVEY 8(d)'s edge-buffer model, `bench.py --no-fuse`);
 * "packed_samples" 0|1 (default 1: inlined sources gather the packed 16-bit form of samples that came from <= 16-bit integer
 *   PCM -- (float)int * scale is how the f32 bank entry was made, so values are identical);
 * "max_chunk_frames" n (edge-buffer chunk cap, default 2^24; smaller values force multi-chunk renders);
 * "output_f32" 0|1 (default 1; 0: a Normalize output vertex rendered to PCM keeps no f32 copy of its frames --
 *   td_graph_read_f32 then fails, the PCM is unchanged);
 * "band_mode" 0|1|2 (default 0 = exact: band_pass_gen, extensions.rs:654-689, bit-identical to the reference's serial
 *   recurrence -- the parity mode.  1 = scan: the same filter as a blocked affine scan, TOLERANCE class: another
 *   realisation of the reference's own f32 rounding noise -- measured 6.3e-8 RMS through 84 band-pass vertices in a row,
 *   +-1 LSB on the PCM; above 1e-6 of the output peak only where a band-pass vertex removes >= 30 dB of its input and a
 *   Normalize vertex brings the rest back up (8 of 18 000 random graphs, at most 3.3e-6).  A state that goes
 *   NaN / infinite stays NaN, as in the reference.  One launch per band-pass vertex, and ONE launch for a whole chain of
 *   `pass` band-pass vertices linked by single-input Sum / Adsr vertices, with the Sum vertex in front and the Normalize
 *   vertex behind.  Cut-offs below ~1.5 Hz keep the exact kernels.  A `pass` vertex' right-channel smoothers reach its
 *   output only as NaN once they are not finite (extensions.rs:685-687): the chain launch does not run them and tracks the
 *   first non-finite right input frame instead.  2 = the scan UNDER THE GUARD -- what a State defaults to: `pass` vertices take
 *   the chain launch wherever its own estimate of its deviation can be carried to the output (any static path, at most one
 *   Normalize vertex on it; no sample loop shorter than 2 048 frames upstream), every other band-pass vertex keeps the exact
 *   kernels, and a render whose estimate is over the bound is rendered again with the exact kernels when the graph is drained:
 *   td_graph_band_guard_stats);
 * "band_guard_ppb" n (default 200: the guard's bound on the estimated RMS deviation of a render, in 1e-9 of full scale -- for
 *   band_mode 2 and sine_mode 2 alike; 0: every audited render is done again);
 * "sine_mode" 0|1|2 (default 1 on a bare td_graph, 2 on a State's graph: debug_sine_gen / synth_gen, extensions.rs:450,501 `f32::sin`.
 *   1 = the oscillators evaluate glibc's sinf -- libm's, what `f32::sin` calls on Linux -- operation for operation in double
 *   precision (glibc 2.28 and later, x86-64 FMA variant; tools/sinf_restate.c agrees with the host's sinf on every finite float) and
 *   the envelopes adsr.rs's own divisions: the two kinds carry the reference's bits like every other kind (50 000 random graphs x 3
 *   renders bit for bit).  0 = the fast forms: a 14-instruction f32 sine (<= 3.3e-7 from sinf), reciprocal envelopes, the
 *   affine / one-grid Synth forms -- ~3e-8 RMS of the vertex' OWN scale (what a graph makes of that -- cancellation, then a Normalize
 *   vertex -- is not bounded), 0.09 instead of 0.32 ms for BASELINE config 3's oscillators.  2 = the fast forms UNDER THE GUARD:
 *   behind every fast launch k_sine_probe evaluates one frame in 256 the reference's way (mode 1's code) and measures the
 *   distance; the audit carries it to the output like a scan launch's estimate (static gains, the Normalize vertex' running
 *   1 / max at the sample's own block); over the bound the render is done again in mode 1's form.  A vertex whose path to the
 *   output the audit cannot follow (two Normalize vertices in a row) renders in mode 1's form from the start).
 * The defaults of td_graph_new and of a State's graph differ in exactly two keys, band_mode (0 | 2) and sine_mode (1 | 2)
 * (tests/test_host_logic.py::test_the_two_default_sets_differ_in_two_keys).
 *
 * Test hooks, "debug.<name>" -- not part of the supported surface: each selects an older or alternative form of a launch, or moves
 * a speculation parameter whose outcome the device verifies; value-neutral by construction, and each pinned by the test named:
 *   debug.norm n (bit 0: every single-pass Normalize tile gives up its wait at once -> the check kernel redoes the vertex;
 *     tests/test_gpu_bench_form.py; bit 1, timing only, WRONG peaks: the earlier tiles' words are not read at all;
 *     bit 2: a tile's one look at the earlier tiles' words sees nothing -- it stores with its own peaks and again after the
 *     wait wherever the running peak came out differently; bit 3: the OTHER order of store and wait than the default -- the
 *     default order is what the read-only option debug.norm_early_store reports (1: store first; kSpecEpilogueDefault); bit 4: count the
 *     blocks stored twice, td_graph_norm_respec, as bit 2 does; tests/test_gpu_sum_spec_epilogue.py) / debug.spec_normalize 0|1 / debug.single_pass_normalize 0|1 / debug.fuse_normalize 0|1
 *     (the two-launch Normalize forms; tests/test_gpu_spec_normalize.py, test_gpu_band_scan.py) /
 *   debug.sum_groups n (0: automatic; n: the wide packed sum in its ragged form on a grid of n workgroups, each carrying 4 .. 16
 *     quads of 256 frames -- a render whose timeline n cannot carry that way fails; tests/test_gpu_sum_ragged.py) /
 *   debug.inline_adsr 0|1 (an Adsr vertex materialised instead of read through; tests/test_gpu_parity.py) /
 *   debug.one_grid_sources 0|1 (a level's source launches one by one instead of as k_sources; tests/test_gpu_sources_grid.py) /
 *   debug.inline_probe 0|1 (sine_mode 2: k_sine_probe as a launch of its own instead of inside the guarded chain launch's tiles;
 *     tests/test_gpu_sine_guard.py) /
 *   debug.table_cache 0|1 (event tables recompiled every render; tests/test_gpu_parity.py) /
 *   debug.band_chain 0|1, debug.band_scan_nf 8|16, debug.band_scan n (scan mode: one launch per vertex, frames per lane, bit 0
 *     = every look-back poll times out and predecessors are recomputed; tests/test_gpu_band_scan.py) /
 *   debug.band_serial 0|1 (1: every band-pass vertex on the serial kernel; tests/test_gpu_parity.py) /
 *   debug.delay_tile 8|16|32|64 (steps per tile of the delay vertex' scan; tests/test_gpu_delay.py) /
 *   debug.sat_tile 128|256|384 (output frames per workgroup of the saturator vertex' k_sat; 256 is provisional: nothing was
 *     timed; tests/test_gpu_saturator.py) /
 *   debug.chorus_tile 256|512|1024 (output frames per workgroup of the chorus vertex' k_chorus; 256 is provisional: nothing was
 *     timed; tests/test_gpu_chorus.py) /
 *   debug.reverb_form 0|1 (the reverb vertex' k_reverb: 0 walks each comb's one-pole serially in the definition's order -- the
 *     numpy twin's bits -- 1 scans it across the wave; the default is the faster row of profiles/reverb_time.txt) /
 *   debug.reverb_block 64|128|256 (the cap of k_reverb's frames per window; tests/test_gpu_reverb.py) /
 *   debug.band_quick n, debug.band_medium n, debug.band_short n, debug.band_warmup n, debug.band_live_exp n, debug.band_depth n
 *     (the exact band-pass' speculative warm-up lengths in 1 / gamma frames and its liveness thresholds: speed only, the
 *     bit-wise check and repair of k_band_fix keep every result exact; tests/test_gpu_quirks.py, tools/band_*_sweep.py).
 * Gone in round 6, with the measurements that retired them in DESIGN.md 7: "branch_streams" (a HIP stream per independent
 * branch of a level: 1.64 against 1.10 ms), "graph_replay" (HIP-graph capture of an unchanged submission: GPU time unchanged,
 * short projects slower), "band_parallel" 0 (the serial band-pass kernel for everything: 58 against 0.7 ms; it remains the
 * fallback for cut-offs below 5 Hz and block pulls), "band_guess_min" / "band_scan_depth" (constants now). */
int td_graph_set_option(td_graph* g, const char* key, long value);
/* Reads any key td_graph_set_option takes (1 = found).  td_graph_option_key(n): the n-th key, NULL behind the last. */
int td_graph_get_option(const td_graph* g, const char* key, long* value);
const char* td_graph_option_key(size_t n);
/* Counters of the exact parallel band-pass for the last rendered chunk, summed over its band-pass
 * vertices: out[0] repair cascades started (segments whose entry state failed the bit-wise check, incl.
 * re-checks after optimistic repairs), out[1] segments recomputed, out[2] of those cut short by a fixed point
 * under constant input. */
int td_graph_band_stats(const td_graph* g, uint32_t out[3]);
/* The guard of "band_mode" 2 (the scan kernels with a bound that is checked, not assumed): every render that holds scan
 * launches ends in one small launch that adds up the launches' own estimates of how far their output lies from the
 * reference's f32 trajectory (band_pass_gen, extensions.rs:654-689: the rounding of the smoother's state, once per frame --
 * the one thing the scan gives up), carried to the graph's output through the gains behind them (normalize_gen's 1 / max
 * included, extensions.rs:321-329).  An estimate over "band_guard_ppb" x 1e-9 RMS (default 200 = 2e-7; the class's bar is
 * 1e-6) raises a word in page-locked memory; whoever drains the graph next (td_graph_sync, the read functions,
 * td_batch_sync, a render that continues from carried state) then renders the same thing again from the state the render
 * started in, with the exact kernels.  The banks handed to a render must therefore stay alive until the graph has been
 * synced.  out[0] renders that carried an audit, out[1] renders done again, out[2] the last estimate (RMS, full scale 1),
 * out[3] the largest one seen. */
int td_graph_band_guard_stats(const td_graph* g, double out[4]);

/* ---- Batch of independent projects (BASELINE config 5) ---------------------------------------
 * The reference renders one project per process: State::render's loop `for _ in 0..cs { g.render(..); write;
 * fb.set_time_to_next_block() }` (state.rs:563-575).  A batch runs that loop for many independent projects at
 * once on one GPU: every project keeps its own Graph / SampleBank / FlowwBank handles (added with td_batch_add,
 * still usable on their own afterwards), the batch compiles all of them into one table arena and merges
 * same-kind launches of different projects into one grid.  Results are exactly those of td_graph_render_all per
 * project.  Projects shard across GPUs as one batch per process; the only cross-GPU exchange is the per-project
 * peak table below (one all-reduce(max), RCCL). */
td_batch* td_batch_new(void);                              /* on the device selected by td_set_device */
void td_batch_free(td_batch* b);                           /* the projects' handles stay valid */
/* Adds one project; returns its index in the batch or -1.  The graph's device work moves to the batch's stream. */
long td_batch_add(td_batch* b, td_graph* g, const td_samplebank* sb, td_flowwbank* fb);
size_t td_batch_size(const td_batch* b);
/* For every project: Graph::reset_normalize_vertices (state.rs:467) + FlowwBank::set_time(0) -- the state
 * right after State::refresh, from which a fresh render starts. */
void td_batch_rewind(td_batch* b);
/* td_graph_render_all[_async] for every project (each project's PCM / f32 stays readable through its own
 * td_graph_read_pcm / td_graph_output_pcm_device).  Returns n_blocks x the FIRST project's block length (projects of a
 * batch may differ in block length: project i rendered n_blocks x its own), 0 on failure.  A step that fails while its
 * projects are being compiled (an out-of-range sample index, an impossible release note ...) leaves the HOST side of every
 * project where the step found it -- FlowwBank cursor, playhead, loop cursors, carried voices, a pending reset_normalization --
 * so the call can be repeated; what the device has already run cannot be taken back. */
size_t td_batch_render_all(td_batch* b, size_t n_blocks, int bits);
size_t td_batch_render_all_async(td_batch* b, size_t n_blocks, int bits);
int td_batch_sync(td_batch* b);
int td_batch_normalize_scan(td_batch* b, size_t chunks);    /* State::scan_exact (state.rs:473-475) per project */
/* State::render (state.rs:477-577) for every project END TO END -- render, PCM to the host, WAV file (hound::WavWriter,
 * state.rs:508-575: the same header and words td_state_render writes) -- as a pipeline: the projects render in groups of
 * `group` (<= 0: 8), one submission each, queued back to back, into ONE device arena (a project's PCM then lives in its slice
 * of it: td_graph_read_pcm keeps working); a copy stream moves each group's PCM -- one contiguous transfer -- into page-locked
 * host memory as soon as the group has rendered, while later groups render; `writers` host threads write paths[i] as soon as
 * project i's group has landed.  paths NULL (or writers 0): no files, the PCM stays readable through td_batch_host_pcm.
 * Returns 1 when everything is written.  times (may be NULL): 8 doubles -- [0] wall ms of the call, [1] of which buffer /
 * event setup (first call), [2] GPU ms first render start -> last render end, [3] copy-stream ms first copy start -> last
 * copy end, [4] sum of the copies' own ms, [5] PCM bytes, [6] host ms first file opened -> last file closed, [7] host ms
 * spent enqueueing. */
int td_batch_render_to_files(td_batch* b, size_t n_blocks, int bits, size_t render_sr, const char* const* paths, int group,
                             int writers, double* times);
/* Project i's PCM of the last td_batch_render_to_files in the library's page-locked buffer (valid until the next such call
 * or td_batch_free). */
const void* td_batch_host_pcm(const td_batch* b, size_t i, size_t* bytes);
/* Per-project peak after the last render: the output Normalize vertex' running peak (`max`, extensions.rs:323,
 * i.e. the project's pre-normalisation peak) or, for other output kinds, the absolute peak of the output.
 * td_batch_peaks: host copy, one float per project in td_batch_add order.  td_batch_peak_table_device: fills a
 * table of n_total floats in DEVICE memory (caller-owned, e.g. the tensor handed to the all-reduce): project i
 * goes to entry first + i * stride, all other entries are zeroed. */
int td_batch_peaks(td_batch* b, float* out);
int td_batch_peak_table_device(td_batch* b, float* d_table, size_t n_total, size_t first, size_t stride);
/* Loudness of every project's last render (td_graph_loudness's eight doubles per project, td_batch_add order), all in ONE
 * k_loudness launch; BS.1770-4 / EBU Tech 3341 / 3342, no reference counterpart.  A project's figures are bitwise those of
 * td_graph_loudness on its own graph. */
int td_batch_loudness(td_batch* b, double* out);
/* td_graph_master on every project's last render (TD_MASTER_FIELDS doubles per project, td_batch_add order): pass k of every
 * project in ONE launch per kernel, projects that are done drop out of later passes.  A project's words and report are bitwise
 * those of td_graph_master on its own graph.  td_batch_render_to_files writes unmastered files (out of scope). */
int td_batch_master(td_batch* b, double target_lufs, double ceiling_dbtp, double lookahead_ms, double release_ms, double* out);
/* ---- the job's one collective, behind the C ABI (round 6).  BASELINE config 5: 512 independent projects over the 8 GPUs of a
 * node, one process per GPU, "RCCL over xGMI only for the final peak all-reduce".  The reference renders one project per process
 * (State::render's loop, state.rs:563-575); a batch driver running that loop on every GPU ends with this exchange.
 * td_comm_unique_id: rank 0 makes the 128-byte id (ncclGetUniqueId) and hands it to the other ranks by whatever the host has
 *   (a file, a socket, MPI); td_comm_init: every rank, on its own device (td_set_device first), joins (ncclCommInitRank -- it
 *   returns when all `world` ranks have called it).  RCCL is dlopen'ed (librccl.so.1 as the process already holds it, else from the
 *   ROCm install, else $TD_RCCL_LIB): without it only td_comm_init fails.  td_comm_init_host: the same job over the HOST's own
 *   all-reduce -- `allreduce_max(ctx, table, n)` replaces table[0 .. n) (host memory) by its element-wise maximum over the ranks and
 *   returns 1 -- for hosts that bring MPI, and for tests that put two ranks on one GPU (RCCL refuses that).
 * td_batch_exchange_peaks: the table of per_rank * world floats -- this rank's project i (td_batch_add order) at entry
 *   rank + i * world, zeros elsewhere (td_batch_peak_table_device) -- then ONE ncclAllReduce(ncclMax, ncclFloat32), in place, on
 *   the batch's own stream right behind the renders: no host synchronisation between the last render and the collective.  Returns
 *   when it is enqueued (RCCL kind); td_batch_sync waits for it.  c NULL = a job of one rank (no collective).  Every rank passes
 *   the same per_rank (>= its own project count).  td_batch_peak_table: the table in device memory (valid after td_batch_sync,
 *   until the next exchange); td_batch_read_peak_table: synchronises and copies n entries out.
 * td_comm_backend: "rccl-native" | "host-callback"; td_comm_library: the RCCL library dlopen resolved ("" if none yet). */
int td_comm_unique_id(void* out, size_t bytes);
td_comm* td_comm_init(const void* unique_id, size_t bytes, int rank, int world);
typedef int (*td_allreduce_max_fn)(void* ctx, float* table, size_t n);
td_comm* td_comm_init_host(td_allreduce_max_fn allreduce_max, void* ctx, int rank, int world);
void td_comm_free(td_comm* c);
const char* td_comm_backend(const td_comm* c);
const char* td_comm_library(void);
int td_batch_exchange_peaks(td_batch* b, td_comm* c, size_t per_rank);
const float* td_batch_peak_table(const td_batch* b, size_t* n);
int td_batch_read_peak_table(td_batch* b, float* out, size_t n);
/* bench hooks, as for a graph */
void td_batch_set_profiling(td_batch* b, int on);
size_t td_batch_last_kernel_times(td_batch* b, const char** names, float* ms, size_t* launches, size_t cap);
size_t td_batch_host_times(td_batch* b, double* ms4, int reset);
/* ... and two marks on the batch's stream: td_batch_mark(b, 0) before a run of submissions, td_batch_mark(b, 1) behind it;
 * td_batch_marked_ms: the time between them on the device (HIP events; waits for the second; < 0: not both set). */
int td_batch_mark(td_batch* b, int which);
double td_batch_marked_ms(td_batch* b);

/* ---- Project front-end: State (state.rs:27-578) -------------------------------------------- */
/* State{..} as constructed at main.rs:75-98 (render_sr 48000, bd 16, output "outp.wav"). */
td_state* td_state_new(const char* wdir, size_t project_samplerate, size_t buffer_length);
/* Reads <wdir>/project.toml ([settings] main, buffer_length=1024, project_samplerate=44100; config.rs:19-76). */
td_state* td_state_open(const char* wdir);
void td_state_free(td_state* s);
/* Engine options of the State's graph (the keys of td_graph_set_option; they survive td_state_refresh).  TWO defaults differ
 * from a bare td_graph's -- a State trades the reference's bytes for speed inside the bound BASELINE's north_star sets for float
 * synth / filter paths (1e-6 RMS), a bare graph does not:
 *   "band_mode" 2: band-pass vertices (band_pass_gen, extensions.rs:654-689) as a blocked affine scan UNDER THE GUARD -- every
 *     render estimates its own deviation from the reference's serial recurrence and is rendered again with the exact kernels when
 *     the estimate is over 2e-7 (td_graph_band_guard_stats).  BASELINE config 4 (84 band-pass vertices): 0.39 ms instead of 12.2 ms;
 *     270 000 random-graph renders: none above 1e-6 by the filter arithmetic.  td_state_set_option(s, "band_mode", 0): the exact
 *     kernels outright, bit-identical to the reference's recurrence;
 *   "sine_mode" 0: debug_sine / synth with the tolerance-class device sine (<= 3.3e-7 from libm's sinf per oscillator; <= 1e-6 RMS of
 *     the vertex' scale) and the affine / one-grid Synth forms.  td_state_set_option(s, "sine_mode", 1): glibc's sinf operation for
 *     operation, the reference's bytes.
 * A project without band-pass, debug_sine and synth vertices renders the same bytes either way. */
int td_state_set_option(td_state* s, const char* key, long value);
/* State::refresh state.rs:50-471 on the given Lua source / on <wdir>/<main>. 1 = loaded. */
int td_state_refresh_source(td_state* s, const char* lua_source);
int td_state_refresh(td_state* s);
int td_state_scan_exact(td_state* s);                                     /* state.rs:473-475 */
/* State::render state.rs:477-577: renders cs blocks and writes the integer WAV to output_file
 * (relative to the process working directory, like hound::WavWriter::create at state.rs:514). path_override may be NULL. */
int td_state_render(td_state* s, const char* path_override);
/* Stems of the State's renders (td_graph_set_stems): the names are resolved at each render -- an unknown one fails the render
 * before any file is written.  td_state_render then writes stem X next to the output as "<path minus .wav>.<X>.wav", same
 * header; characters of X outside [A-Za-z0-9._-] become '_', and two stems that map to one file name are an error.
 * n = 0 clears the list. */
int td_state_set_stems(td_state* s, const char* const* names, size_t n);
/* Master every later render of the State (on = 1; 0: off, the default) to target_lufs under ceiling_dbtp with the default
 * lookahead (5 ms) and release (100 ms): td_graph_master after the render, before the read-back, so td_state_render,
 * _render_to_memory and _render_view return mastered words.  Stems are written unmastered. */
int td_state_set_master(td_state* s, int on, double target_lufs, double ceiling_dbtp);
/* The report (TD_MASTER_FIELDS doubles) of the State's last render; 0 when that render was not mastered. */
int td_state_master_report(const td_state* s, double* out);
/* Same render, PCM left in memory: copies frames*2 words to out (may be NULL to query the size). */
size_t td_state_render_to_memory(td_state* s, void* out, size_t bytes);
/* The same render, returned as a view of the library's own page-locked read-back buffer (interleaved PCM,
 * *bytes long; valid until the next render or td_state_free): no second copy.  NULL on failure. */
const void* td_state_render_view(td_state* s, size_t* bytes);
size_t td_state_chunk_count(const td_state* s);                            /* cs, state.rs:104 */
size_t td_state_buffer_length(const td_state* s);                          /* config.rs:58-60 */
size_t td_state_project_samplerate(const td_state* s);                     /* config.rs:62-64 */
size_t td_state_render_samplerate(const td_state* s);
size_t td_state_bitdepth(const td_state* s);
const char* td_state_output_file(const td_state* s);
td_graph* td_state_graph(td_state* s);
td_samplebank* td_state_samplebank(td_state* s);
td_flowwbank* td_state_flowwbank(td_state* s);
/* The recorded script calls in call order, one per line, canonical text (host-logic tests). */
const char* td_state_dump_calls(td_state* s);

#ifdef __cplusplus
}
#endif
#endif /* TERMDAW_AMD_H */
