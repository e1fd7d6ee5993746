// engine.cpp -- graph model, chunk compiler and launch scheduler behind the C ABI.
//
// Reference items are cited as file:line relative to /root/reference/src.  This file holds the
// *host* half of the path: graph construction rules (graph.rs:49-174), the FlowwBank cursor
// (floww.rs:70-141) and the sequential per-vertex bookkeeping (voice lists, f32 envelope clocks,
// one-shot cursors) that the reference interleaves with its per-sample loops.  Everything that is
// per-sample runs on the GPU (kernels.hip).  There is no CPU render fallback: every render entry
// point fails when no HIP device is usable.
#include <chrono>

#include "engine.h"
#include "chorus_math.h"
#include "gate_math.h"
#include "phaser_math.h"
#include "vocoder_math.h"
#include "filter_math.h"
#include "limiter_math.h"
#include "conv_math.h"
#include "multiband_math.h"
#include "comm.h"
#include "compile.h"
#include "delay_math.h"
#include "reverb_math.h"
#include "devmem.h"
#include "eq_math.h"
#include "midi.h"
#include "sat_math.h"
#include "sum_index.h"

#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <tuple>
#include <mutex>
#include <condition_variable>
#include <atomic>
#include <thread>
#include <limits>

#include "loudness.h"
#include "master.h"
#include "wav.h"

using namespace tdk;

namespace tde {

thread_local std::string g_error;
int fail(const std::string& msg) {
    g_error = msg;
    return 0;
}

#define TD_HIP(expr)                                                                      \
    do {                                                                                  \
        hipError_t _e = (expr);                                                           \
        if (_e != hipSuccess) {                                                           \
            g_error = std::string("HIP error: ") + hipGetErrorString(_e) + " at " #expr;  \
            return 0;                                                                     \
        }                                                                                 \
    } while (0)

size_t f32_as_usize(float x) {   // Rust `x as usize`
    if (!(x == x)) return 0;
    if (x <= 0.0f) return 0;
    if (x >= 18446744073709551616.0f) return std::numeric_limits<size_t>::max();
    return (size_t)x;
}

static thread_local int t_device = 0;

static int ensure_device(int dev) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
        return fail("termdaw_amd: no HIP device available (the render path has no CPU fallback)");
    if (dev >= n) return fail("termdaw_amd: device index out of range");
    TD_HIP(hipSetDevice(dev));
    return 1;
}

// ------------------------------------------------------------------------------------------------
// sample load pipeline (sample.rs:38-77, 125-147, 252-313) -- decisions on the host, data on the device
// ------------------------------------------------------------------------------------------------
enum LoadMethod { LM_STEREO, LM_LEFT, LM_RIGHT, LM_LOUDEST, LM_NORM, LM_MIX };
static LoadMethod method_from(const char* s) {   // sample.rs:199-210
    std::string m = s ? s : "";
    if (m == "left") return LM_LEFT;
    if (m == "right") return LM_RIGHT;
    if (m == "loudest") return LM_LOUDEST;
    if (m == "normalize-seperate") return LM_NORM;
    if (m == "mix-down") return LM_MIX;
    return LM_STEREO;
}

// Build-defined sinc resampler (DESIGN.md "Resampler"): the reference calls rubato::SincFixedIn<f32> with
// sinc_len 256, f_cutoff 0.95, Linear, oversampling 256, BlackmanHarris2 (sample.rs:152-158,
// state.rs:534-540); rubato's arithmetic is un-vendored, so this is this engine's own specification with
// that parameter set -- parity with the reference is unpinned, parity with oracle/ is bit-exact.
static void build_sinc_table(size_t from, size_t to, std::vector<float>* T) {
    const double ratio = (double)to / (double)from;
    const double fc = 0.95 * (ratio < 1.0 ? ratio : 1.0);
    const double pi = 3.14159265358979323846;
    auto tap = [&](double d) {   // window^2 x sinc at d input frames from the filter centre (|d| <= 128)
        const double z = fc * d;
        const double sinc = z == 0.0 ? 1.0 : sin(pi * z) / (pi * z);
        const double u = (d + 128.0) / 256.0;
        const double bh = 0.35875 - 0.48829 * cos(2.0 * pi * u) + 0.14128 * cos(4.0 * pi * u) - 0.01168 * cos(6.0 * pi * u);
        return sinc * bh * bh;
    };
    // normalisation as rubato's make_sincs does it (from the crate's published source, from memory -- unverified): the sum
    // of ALL sinc_len * oversampling points of the windowed sinc, divided by the oversampling factor
    double sum = 0.0;
    for (int x = 0; x < kSincLen * kSincOver; ++x) sum += tap((double)(x - kSincLen * kSincOver / 2) / (double)kSincOver);
    const double norm = sum / (double)kSincOver;
    T->resize((size_t)(kSincOver + 1) * kSincLen);
    for (int p = 0; p <= kSincOver; ++p)
        for (int k = 0; k < kSincLen; ++k)
            (*T)[(size_t)p * kSincLen + k] = (float)(tap((double)k - 127.0 - (double)p / (double)kSincOver) / norm);
}
// Resamples `len` frames at `in` (device) from rate `from` to rate `to` into a fresh device buffer.
int resample_device(const float2* in, size_t len, size_t from, size_t to, float2** out, size_t* nout_p, hipStream_t st) {
    if (from == 0 || to == 0) return fail("resample: sample rate 0");
    const size_t nout = (size_t)(((unsigned __int128)len * to + from - 1) / from);
    std::vector<float> T;
    build_sinc_table(from, to, &T);
    float* d_T = nullptr;
    float2* d_out = nullptr;
    TD_HIP(hipMalloc(&d_T, T.size() * sizeof(float)));
    if (hipMalloc(&d_out, (nout + (nout & 1) + 17) * sizeof(float2)) != hipSuccess) {
        (void)hipFree(d_T);
        return fail("termdaw_amd: out of device memory for the resampled sample");
    }
    auto bail = [&](hipError_t e, const char* what) {
        (void)hipFree(d_T);
        (void)hipFree(d_out);
        return fail(std::string("HIP error: ") + hipGetErrorString(e) + " at " + what);
    };
    hipError_t he;
    if ((he = hipMemcpyAsync(d_T, T.data(), T.size() * sizeof(float), hipMemcpyHostToDevice, st)) != hipSuccess) return bail(he, "table upload");
    // the pad behind the last frame (odd tail + wrap frames) starts out as zeros
    if ((he = hipMemsetAsync(d_out + nout, 0, ((nout & 1) + 17) * sizeof(float2), st)) != hipSuccess) return bail(he, "pad memset");
    if (nout == 0) {
        (void)hipStreamSynchronize(st);
        (void)hipFree(d_T);
        *out = d_out;
        *nout_p = 0;
        return 1;
    }
    ResampleDesc d{in, d_out, d_T, len, nout, from, to};
    launch_resample(d, st);
    // frames nout .. nout + 14 = the first frames again (wrap frames, as in every bank entry)
    for (size_t i = 0; nout && i < 15;) {
        const size_t src = i % nout, cnt = std::min<size_t>(15 - i, nout - src);
        if ((he = hipMemcpyAsync(d_out + nout + i, d_out + src, cnt * sizeof(float2), hipMemcpyDeviceToDevice, st)) != hipSuccess)
            return bail(he, "wrap frames");
        i += cnt;
    }
    if ((he = hipStreamSynchronize(st)) != hipSuccess) return bail(he, "resample");
    if ((he = hipGetLastError()) != hipSuccess) return bail(he, "resample launch");
    (void)hipFree(d_T);
    *out = d_out;
    *nout_p = nout;
    return 1;
}

}  // namespace tde

void* td_samplebank::alloc(int pool, size_t bytes) {
    bytes = (bytes + 255) & ~(size_t)255;
    auto& v = slabs[pool];
    if (v.empty() || v.back().cap - v.back().used < bytes) {
        Slab s;
        s.cap = std::max<size_t>(bytes, (size_t)16 << 20);
        if (hipMalloc(&s.base, s.cap) != hipSuccess) {
            tde::fail("termdaw_amd: out of device memory for the sample bank");
            return nullptr;
        }
        v.push_back(s);
    }
    Slab& s = v.back();
    void* p = s.base + s.used;
    s.used += bytes;
    s.live += 1;
    return p;
}
namespace tde {
// Arenas with a deferred k_norm_fix outstanding (Arena::pending_fix).  The fix, if it runs, gathers again from the sample
// tables: a bank about to give memory back settles every such arena on its device first.
static std::mutex g_fix_mu;
static std::vector<Arena*> g_fix_arenas;
static int settle_arena(Arena& ar, hipStream_t stream);
static int cur_device() {
    int d = 0;
    (void)hipGetDevice(&d);
    return d;
}
static void note_pending(Arena& ar, hipStream_t stream, int device) {
    ar.fix_stream = stream;
    ar.fix_device = device;
    if (ar.listed) return;
    std::lock_guard<std::mutex> lk(g_fix_mu);
    g_fix_arenas.push_back(&ar);
    ar.listed = true;
}
static void unlist_arena(Arena& ar) {
    if (!ar.listed) return;
    std::lock_guard<std::mutex> lk(g_fix_mu);
    g_fix_arenas.erase(std::remove(g_fix_arenas.begin(), g_fix_arenas.end(), &ar), g_fix_arenas.end());
    ar.listed = false;
}
static void drop_pending(Arena& ar) {
    ar.pending_fix.clear();
    unlist_arena(ar);
}
static void settle_device_arenas(int device) {
    std::vector<Arena*> todo;
    {
        std::lock_guard<std::mutex> lk(g_fix_mu);
        for (Arena* a : g_fix_arenas)
            if (a->fix_device == device && !a->pending_fix.empty()) todo.push_back(a);
    }
    for (Arena* a : todo) (void)settle_arena(*a, a->fix_stream);
}
}  // namespace tde

void td_samplebank::release(void* p) {
    if (!p) return;
    for (auto& v : slabs)
        for (size_t i = 0; i < v.size(); ++i) {
            Slab& s = v[i];
            if ((unsigned char*)p >= s.base && (unsigned char*)p < s.base + s.cap) {
                if (s.live) --s.live;
                if (s.live == 0) {               // nothing left in it: reuse from the start, or give it back
                    // (kernels queued by td_graph_render_all_async / td_batch_render_all_async on the engines' non-blocking
                    // streams may still gather from this memory: the per-sample hipFree of the old path synchronised implicitly)
                    (void)hipSetDevice(device);   // (the BANK's device, whatever the calling thread last selected)
                    tde::settle_device_arenas(device);   // (... and a deferred k_norm_fix would gather from it once more)
                    (void)hipDeviceSynchronize();
                    if (i + 1 == v.size()) s.used = 0;
                    else { (void)hipFree(s.base); v.erase(v.begin() + (long)i); }
                }
                return;
            }
        }
    (void)hipFree(p);   // a stand-alone allocation (resampled entries)
}
void td_samplebank::release_all() {
    tde::settle_device_arenas(device);
    (void)hipDeviceSynchronize();
    for (auto& v : slabs) {
        for (auto& s : v) (void)hipFree(s.base);
        v.clear();
    }
}

namespace tde {

// SampleBank::add after the WAV header is known (sample.rs:240-313).  The host only takes the decisions
// that depend on counts (channel / length checks, Sample::from's Err arms); decode, de-interleave, load
// mode, peak scan and normalisation run on the device.  Exactly one of `linear` (already decoded f32 stream)
// and `raw` (little-endian PCM words) is given.
static int bank_add_stream(td_samplebank* sb, const std::string& name, const float* linear, const uint8_t* raw,
                           uint32_t raw_format, size_t n_values, int channels, size_t sr, size_t bd, LoadMethod method) {
    if (sb->names.count(name))
        return fail("TermDaw: SampleBank: there is already a sample with name \"" + name + "\" present.");
    if (method == LM_STEREO && channels != 2)
        return fail("TermDaw: SampleBank: only 2 channel samples are supported for stereo samples.");
    if (method != LM_STEREO && channels > 2)
        return fail("TermDaw: SampleBank: only 1,2 channel samples are supported for left or right samples.");
    if (channels < 1) return fail("TermDaw: SampleBank: sample has no channels.");
    if (n_values > 0xFFFFFFF0ull) return fail("termdaw_amd: sample too long");
    sb->max_sr = std::max(sb->max_sr, sr);
    sb->max_bd = std::max(sb->max_bd, bd);
    // lengths of the de-interleaved l / r (sample.rs:275-292)
    size_t nl, nr;
    if (channels == 1) {
        nl = method == LM_LEFT ? n_values : 0;
        nr = method == LM_LEFT ? 0 : n_values;
    } else {
        nl = n_values / 2 + (n_values & 1);   // a dangling last value goes to l
        nr = n_values / 2;
    }
    // Sample::from (sample.rs:38-77): which decoded channel feeds l and r; src 0/1 = channel index
    uint32_t src_l = 0, src_r = channels == 2 ? 1u : 0u;
    bool pick_loudest = false;
    switch (method) {
        case LM_LEFT:
            if (nl == 0) return fail("TermDaw: Sample::from: l has length 0.");
            nr = nl;
            src_r = src_l = 0;
            break;
        case LM_RIGHT:
            if (nr == 0) return fail("TermDaw: Sample::from: r has length 0.");
            nl = nr;
            src_l = src_r = channels == 2 ? 1u : 0u;
            break;
        case LM_LOUDEST: pick_loudest = true; break;
        default:
            if (nl != nr) return fail("TermDaw: Sample::from: l and r do not have the same length.");
            if (nl == 0) return fail("TermDaw: Sample::from: l and r have length 0.");
    }
    if (!ensure_device(sb->device)) return 0;
    hipStream_t st = nullptr;   // load time: the default stream is fine
    const size_t nmax = std::max(nl, nr);
    float *d_lin = nullptr, *d_l = nullptr, *d_r = nullptr, *d_s = nullptr;
    uint8_t* d_raw = nullptr;
    auto cleanup = [&]() {};   // (the scratch belongs to the bank)
    {
        auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
        const size_t bps_raw = linear ? 0 : (raw_format == PCM_U8 ? 1 : raw_format == PCM_S16 ? 2 : raw_format == PCM_S24 ? 3 : 4);
        const size_t b_lin = up(std::max<size_t>(n_values, 1) * sizeof(float)), b_ch = up(std::max<size_t>(nmax, 1) * sizeof(float));
        const size_t b_raw = up(std::max<size_t>(n_values * bps_raw, 1));
        const size_t need = b_lin + 2 * b_ch + 256 + b_raw;
        if (need > sb->tmp_cap) {
            TD_HIP(hipDeviceSynchronize());
            if (sb->tmp) (void)hipFree(sb->tmp);
            sb->tmp = nullptr;
            sb->tmp_cap = 0;
            TD_HIP(hipMalloc(&sb->tmp, need + need / 2));
            sb->tmp_cap = need + need / 2;
        }
        unsigned char* p = sb->tmp;
        d_lin = reinterpret_cast<float*>(p); p += b_lin;
        d_l = reinterpret_cast<float*>(p); p += b_ch;
        d_r = reinterpret_cast<float*>(p); p += b_ch;
        d_s = reinterpret_cast<float*>(p); p += 256;
        d_raw = p;
    }
    if (linear) {
        TD_HIP(hipMemcpyAsync(d_lin, linear, n_values * sizeof(float), hipMemcpyHostToDevice, st));
    } else {
        const size_t bps = raw_format == PCM_U8 ? 1 : raw_format == PCM_S16 ? 2 : raw_format == PCM_S24 ? 3 : 4;
        TD_HIP(hipMemcpyAsync(d_raw, raw, n_values * bps, hipMemcpyHostToDevice, st));
        launch_pcm_decode(d_raw, d_lin, (uint32_t)n_values, raw_format, st);
    }
    if (pick_loudest) {
        // Loudest (sample.rs:54-62): mean |l| > mean |r| ? l : r, with the means summed left to right in f32
        if (channels == 1) {   // one of the two is empty: mean_energy(empty) = 0
            launch_sample_split(d_lin, 1, 0, 0, d_l, d_r, (uint32_t)nl, (uint32_t)nr, st);
        } else {
            launch_sample_split(d_lin, 2, 0, 1, d_l, d_r, (uint32_t)nl, (uint32_t)nr, st);
        }
        launch_abs_sum_serial(d_l, (uint32_t)nl, d_s + 4, st);
        launch_abs_sum_serial(d_r, (uint32_t)nr, d_s + 5, st);
        float sums[2];
        TD_HIP(hipMemcpyAsync(sums, d_s + 4, 8, hipMemcpyDeviceToHost, st));
        TD_HIP(hipStreamSynchronize(st));
        const float lm = nl ? sums[0] / (float)nl : 0.0f, rm = nr ? sums[1] / (float)nr : 0.0f;
        const bool take_l = lm > rm;
        const size_t n_take = take_l ? nl : nr;
        if (n_take == 0) { cleanup(); return fail("termdaw_amd: loudest channel is empty"); }
        // both outputs become the chosen channel
        TD_HIP(hipMemcpyAsync(take_l ? d_r : d_l, take_l ? d_l : d_r, n_take * sizeof(float), hipMemcpyDeviceToDevice, st));
        nl = nr = n_take;
    } else {
        launch_sample_split(d_lin, (uint32_t)channels, src_l, src_r, d_l, d_r, (uint32_t)nl, (uint32_t)nr, st);
    }
    size_t n = nl;
    const float *p_max_l = d_s, *p_max_r = d_s + 1;
    if (method == LM_NORM) {   // normalize_seperate (sample.rs:132-137)
        launch_absmax(d_l, (uint32_t)nl, d_s, st);
        launch_absmax(d_r, (uint32_t)nr, d_s + 1, st);
    } else if (method == LM_MIX) {   // mix_down (sample.rs:139-147): zip stops at the shorter channel
        n = std::min(nl, nr);
        launch_add_planar(d_l, d_r, d_l, (uint32_t)n, st);
        launch_absmax(d_l, (uint32_t)n, d_s, st);
        TD_HIP(hipMemcpyAsync(d_r, d_l, n * sizeof(float), hipMemcpyDeviceToDevice, st));
        p_max_r = d_s;
    } else {   // normalize(usize::MAX) (sample.rs:125-130): one common peak
        launch_absmax(d_l, (uint32_t)nl, d_s, st);
        launch_absmax(d_r, (uint32_t)nr, d_s + 1, st);
        // max(absmax(l), absmax(r)): both are >= 0, so the uint pattern orders like the float
        launch_absmax(d_s, 2, d_s + 2, st);
        p_max_l = p_max_r = d_s + 2;
    }
    if (nl != nr && method != LM_MIX) { cleanup(); return fail("termdaw_amd: channel lengths differ after load"); }
    if (n == 0) { cleanup(); return fail("TermDaw: Sample::from: l and r have length 0."); }
    SampleEntry e;
    e.len = n;
    // n frames, then the first 15 again (wrap frames for looping readers), padded to an even count
    // (every failure return below hands the entry's memory back to the bank)
    e.d = static_cast<float2*>(sb->alloc(0, (n + 16 + (n & 1)) * sizeof(float2)));
    if (!e.d) return 0;
    struct Guard {
        td_samplebank* sb; SampleEntry* e; bool armed = true;
        ~Guard() { if (armed) { sb->release(e->d); sb->release(e->d16); } }
    } guard{sb, &e};
    TD_HIP(hipMemsetAsync(e.d + n, 0, (16 + (n & 1)) * sizeof(float2), st));
    launch_sample_pack(d_l, d_r, p_max_l, p_max_r, e.d, (uint32_t)n, st);
    // packed 16-bit twin: only when l / r are still the raw integer PCM values times one scale per channel
    // (every mode but mix-down) and no resample follows
    bool want16 = method != LM_MIX && sr == sb->sample_rate && n >= 1 && n < 0x3FFFFFF0u;
    if (want16) {
        e.d16 = static_cast<uint32_t*>(sb->alloc(1, (size_t)tdsi::packed_words((uint32_t)n) * sizeof(uint32_t)));   // the loop + its first 255 frames again (sum_index.h)
        if (!e.d16) return 0;
        TD_HIP(hipMemsetAsync(d_s + 8, 0, sizeof(uint32_t), st));
        launch_sample_pack16(d_l, d_r, e.d16, (uint32_t)n, reinterpret_cast<uint32_t*>(d_s + 8), st);
    }
    float host_s[12] = {0};
    TD_HIP(hipMemcpyAsync(host_s, d_s, sizeof host_s, hipMemcpyDeviceToHost, st));
    TD_HIP(hipStreamSynchronize(st));
    TD_HIP(hipGetLastError());
    if (want16) {
        uint32_t bad;
        memcpy(&bad, &host_s[8], 4);
        const float ml = host_s[p_max_l - d_s], mr = host_s[p_max_r - d_s];
        if (bad) {
            sb->release(e.d16);
            e.d16 = nullptr;
        } else {
            e.scale_l = 1.0f / ml;   // the same `1.0 / max` k_sample_pack multiplied by
            e.scale_r = 1.0f / mr;
        }
    }
    cleanup();
    if (sr != sb->sample_rate) {   // sample.rs:305-310: Sample::resample after the normalisation
        float2* rs = nullptr;
        size_t nout = 0;
        if (!resample_device(e.d, e.len, sr, sb->sample_rate, &rs, &nout, st)) return 0;
        sb->release(e.d);
        e.d = rs;   // (a stand-alone allocation: release() tells it from slab memory)
        if (nout == 0) return fail("termdaw_amd: resampled sample is empty");
        e.len = nout;
    }
    guard.armed = false;
    sb->samples.push_back(e);
    sb->names[name] = sb->samples.size() - 1;
    return 1;
}

}  // namespace tde

using namespace tde;

// ------------------------------------------------------------------------------------------------
// FlowwBank cursor (floww.rs:70-91)
// ------------------------------------------------------------------------------------------------
uint64_t td_flowwbank::next_version() {
    static std::atomic<uint64_t> counter{1};
    return counter.fetch_add(1);
}
void td_flowwbank::set_start_indices_to_frame(size_t t_frame, bool do_skip) {
    for (size_t i = 0; i < flowws.size(); ++i) {
        const auto& fl = flowws[i];
        for (size_t j = do_skip ? start_indices[i] : 0; j < fl.size(); ++j) {
            if (frame_of(fl[j]) >= t_frame) {
                start_indices[i] = j;
                break;
            }
        }
    }
}
void td_flowwbank::set_time(size_t t) {
    set_start_indices_to_frame(t, false);
    frame = t;
}
void td_flowwbank::set_time_to_next_block() {
    frame += bl;
    set_start_indices_to_frame(frame, true);
}

namespace tde {
int upload_tables(td_graph* g, TableCache& tc, const Staging& tmp) {
    const size_t bytes = std::max<size_t>(tmp.b.size(), 16);
    if (bytes > tc.cap) {
        TD_HIP(hipStreamSynchronize(g->stream));   // (kernels of earlier renders may still read the old buffer)
        if (tc.d) { (void)hipFree(tc.d); g->device_bytes -= tc.cap; }
        if (tc.h) (void)hipHostFree(tc.h);
        tc.d = tc.h = nullptr;
        tc.cap = 0;
        tc.inflight = false;
        const size_t cap = bytes + bytes / 4 + 256;
        TD_HIP(hipMalloc(&tc.d, cap));
        TD_HIP(hipHostMalloc(&tc.h, cap, hipHostMallocDefault));
        if (!tc.copied) TD_HIP(hipEventCreateWithFlags(&tc.copied, hipEventDisableTiming));
        tc.cap = cap;
        g->device_bytes += cap;
    }
    if (tc.inflight) TD_HIP(hipEventSynchronize(tc.copied));
    tc.inflight = false;
    memcpy(tc.h, tmp.b.data(), tmp.b.size());
    if (debug_sync() & 1) TD_HIP(hipStreamSynchronize(g->stream));
    TD_HIP(hipMemcpyAsync(tc.d, tc.h, tmp.b.size(), hipMemcpyHostToDevice, g->stream));
    TD_HIP(hipEventRecord(tc.copied, g->stream));
    tc.inflight = true;
    if (debug_sync() & 2) TD_HIP(hipEventSynchronize(tc.copied));
    if (debug_sync() & 4) { fprintf(stderr, "U tables %zu\n", tmp.b.size()); (void)hipStreamSynchronize(g->stream); fprintf(stderr, "ok\n"); }
    debug_verify_upload("tables", (const uint8_t*)tc.d, (const uint8_t*)tc.h, tmp.b.size(), g->stream);
    return 1;
}
static void free_tables(td_graph* g) {   // (device selected, stream synchronised by the caller)
    for (auto& v : g->vertices)
        if (v.tables) {
            if (v.tables->d) { (void)hipFree(v.tables->d); g->device_bytes -= v.tables->cap; }
            if (v.tables->h) (void)hipHostFree(v.tables->h);
            if (v.tables->copied) (void)hipEventDestroy(v.tables->copied);
            v.tables.reset();
        }
}

static int ensure_graph_device(td_graph* g) {
    if (!ensure_device(g->device)) return 0;
    if (!g->stream) {   // (also after a td_batch_free whose stream creation failed: made on next use)
        TD_HIP(hipStreamCreateWithFlags(&g->stream, hipStreamNonBlocking));
        g->owns_stream = true;
    }
    if (!g->d_scalar) TD_HIP(hipMalloc(&g->d_scalar, 256));
    if (!g->guard.h_word) {   // (band_mode 2: k_band_audit's verdict lands here)
        TD_HIP(hipHostMalloc((void**)&g->guard.h_word, 64, hipHostMallocMapped | hipHostMallocCoherent));
        g->guard.h_word[0] = 0u;
        g->guard.h_word[1] = 0u;
        TD_HIP(hipHostGetDevicePointer((void**)&g->guard.d_word, g->guard.h_word, 0));
    }
    return 1;
}

static int ensure_state_slots(td_graph* g) {
    const size_t need = g->hstate.size();
    if (need > g->dstate_cap) {
        const size_t cap = std::max<size_t>(64, need * 2);
        StateSlot* nd = nullptr;
        TD_HIP(hipMalloc(&nd, cap * sizeof(StateSlot)));
        if (g->dstate) {
            TD_HIP(hipStreamSynchronize(g->stream));
            TD_HIP(hipMemcpy(nd, g->dstate, g->dstate_cap * sizeof(StateSlot), hipMemcpyDeviceToDevice));
            TD_HIP(hipFree(g->dstate));
        }
        g->dstate = nd;
        g->dstate_cap = cap;
    }
    if (g->state_host_dirty && need) {
        // host mirror is authoritative only right after construction / explicit host edits
        TD_HIP(hipStreamSynchronize(g->stream));
        TD_HIP(hipMemcpy(g->dstate, g->hstate.data(), need * sizeof(StateSlot), hipMemcpyHostToDevice));
        g->state_host_dirty = false;
    }
    return 1;
}

// The effect kind of a vertex that carries state slots (FxKind::state_slots) and has them; nullptr: any other vertex
static const FxKind* slot_kind(const Vertex& v) {
    const FxKind* fx = fx_kind(v.kind);
    return fx && fx->state_slots && v.state_slot >= 0 ? fx : nullptr;
}
static int drain(td_graph* g);   // stream drained + deferred k_norm_fix settled (defined with the render loop)
static int pull_state(td_graph* g) {
    if (g->state_dev_dirty && g->dstate && !g->hstate.empty()) {
        if (!drain(g)) return 0;
        TD_HIP(hipMemcpy(g->hstate.data(), g->dstate, g->hstate.size() * sizeof(StateSlot), hipMemcpyDeviceToHost));
        g->state_dev_dirty = false;
        for (const auto& v : g->vertices) {   // (a set_time not yet carried to the device by a submission)
            if (!v.first_pending) continue;
            if (v.kind == K_BAND_PASS && v.state_slot >= 0) g->hstate[(size_t)v.state_slot].band.first = 1u;
            if (const FxKind* fx = slot_kind(v)) fx->put_rest(g, v, &g->hstate[(size_t)v.state_slot]);
        }
    }
    return 1;
}

int ensure_buffers(td_graph* g, size_t frames) {
    frames = (frames + 3) & ~(size_t)3;   // (whole fours: the planar-in-4 copy of a band-pass vertex' input covers the last, partial four too)
    if (frames > g->cap_frames) {
        if (!drain(g)) return 0;
        for (float2* p : g->pool) {
            (void)hipFree(p);
            g->device_bytes -= g->cap_frames * sizeof(float2);
        }
        g->pool.clear();
        g->cap_frames = frames;
    }
    g->free_bufs = g->pool;
    return 1;
}
// The block a delay, saturator, chorus, reverb, vocoder, limiter or multiband vertex carries (Vertex::line): allocated when the vertex is first compiled into a
// submission (never cleared: a word is read only once the vertex has written it, Line::total), freed with the graph's vertices.
void* take_line(td_graph* g, Vertex& v, size_t bytes) {
    if (v.line.d) return v.line.d;
    void* p = nullptr;
    if (hipMalloc(&p, bytes) != hipSuccess) return nullptr;
    g->device_bytes += bytes;
    v.line = {p, bytes, 0, 0};
    return p;
}
// A convolution vertex' spectra block (Vertex::spectra): allocated when the vertex is first compiled into a submission, again when
// the response has another partition count; *build whenever the sample behind the index is not the one the block was built from.
// A line whose size no longer fits the response goes with it: the vertex then restarts from silence.
void* take_spectra(td_graph* g, Vertex& v, size_t bytes, const void* src, size_t src_len, size_t line_bytes, bool* build) {
    Vertex::Spectra& sp = v.spectra;
    *build = !sp.d || sp.bytes != bytes || sp.src != src || sp.src_len != src_len;
    if (sp.d && sp.bytes != bytes) {
        (void)hipFree(sp.d);   // (waits for the device)
        g->device_bytes -= sp.bytes;
        sp = {};
    }
    if (v.line.d && v.line.bytes != line_bytes) {
        (void)hipFree(v.line.d);
        g->device_bytes -= v.line.bytes;
        v.line = {};
    }
    if (!sp.d) {
        void* p = nullptr;
        if (hipMalloc(&p, bytes) != hipSuccess) return nullptr;
        g->device_bytes += bytes;
        sp.d = p;
        sp.bytes = bytes;
    }
    sp.src = src;
    sp.src_len = src_len;
    return sp.d;
}
// The twiddle table of the convolution vertices' transforms: computed once per process in long double, uploaded once per device,
// kept for the life of the process.
const double* take_twiddles(td_graph* g) {
    static std::mutex mu;
    static std::map<int, double*> by_device;
    std::lock_guard<std::mutex> lock(mu);
    auto it = by_device.find(g->device);
    if (it != by_device.end()) return it->second;
    std::vector<double> h((size_t)conv::kN);
    conv::twiddles(h.data());
    double* p = nullptr;
    if (hipMalloc(&p, h.size() * sizeof(double)) != hipSuccess) return nullptr;
    if (hipMemcpy(p, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) { (void)hipFree(p); return nullptr; }
    by_device[g->device] = p;
    return p;
}
// (a chunk that failed to compile or to submit may have claimed spectra whose k_conv_ir never ran: they are built again)
static void forget_spectra(td_graph* g) {
    for (auto& v : g->vertices) v.spectra.src = nullptr;
    g->conv_checks.clear();
}
// the line a vertex would continue from in its next submission (nullptr: none -- it has none yet, or it starts afresh)
static const void* carried_line(const Vertex& v) {
    return !v.first_pending && v.line.total ? v.line.d : nullptr;
}
static bool has_lines(const td_graph* g) {
    for (const auto& v : g->vertices)
        if (v.line.d || v.spectra.d) return true;
    return false;
}
// (give_back false: no device to give them back to -- they leave the books with their vertices all the same)
static void free_lines(td_graph* g, bool give_back) {
    for (auto& v : g->vertices) {
        if (v.spectra.d) {
            if (give_back) (void)hipFree(v.spectra.d);
            g->device_bytes -= v.spectra.bytes;
            v.spectra = {};
        }
        if (!v.line.d) continue;
        if (give_back) (void)hipFree(v.line.d);
        g->device_bytes -= v.line.bytes;
        v.line = {};
    }
}
float2* take_buffer(td_graph* g) {
    if (!g->free_bufs.empty()) {
        float2* p = g->free_bufs.back();
        g->free_bufs.pop_back();
        return p;
    }
    float2* p = nullptr;
    if (hipMalloc(&p, g->cap_frames * sizeof(float2)) != hipSuccess) return nullptr;
    g->pool.push_back(p);
    g->device_bytes += g->cap_frames * sizeof(float2);
    return p;
}

// Waits for `stream`, then looks at the arena's host-visible word: a single-pass Normalize tile of the last submission gave
// up its bounded wait for an earlier tile (SumDesc modes 4 / 5) and the check launch was not enqueued behind it -> k_norm_fix
// redoes the vertex now, from the block peaks the launch left behind.  The normal case costs one load of page-locked memory.
static int settle_arena(Arena& ar, hipStream_t stream) {
    if (!stream) return 1;
    TD_HIP(hipStreamSynchronize(stream));
    if (!ar.h_flag || !*(volatile uint32_t*)ar.h_flag) {
        drop_pending(ar);   // (settled: the launch needed no fix)
        return 1;
    }
    for (const auto& f : ar.pending_fix) launch_norm_fix((const SumDesc*)(ar.d + f.off), f.n, f.M, f.bl, stream);
    TD_HIP(hipGetLastError());
    TD_HIP(hipStreamSynchronize(stream));
    *(volatile uint32_t*)ar.h_flag = 0u;
    drop_pending(ar);
    ar.fix_runs += 1;
    return 1;
}

static int ensure_arena(Arena& ar, size_t bytes, hipStream_t stream) {
    if (!ar.h_flag) {
        TD_HIP(hipHostMalloc((void**)&ar.h_flag, 64, hipHostMallocMapped | hipHostMallocCoherent));
        *ar.h_flag = 0u;
        TD_HIP(hipHostGetDevicePointer((void**)&ar.d_flag, ar.h_flag, 0));
    }
    if (!ar.d_respec) {
        TD_HIP(hipMalloc((void**)&ar.d_respec, 256));
        TD_HIP(hipMemset(ar.d_respec, 0, 256));
    }
    if (bytes <= ar.cap) return 1;
    const size_t cap = std::max<size_t>(bytes * 2, 1 << 20);
    if (stream && !settle_arena(ar, stream)) return 0;   // (a pending fix reads descriptors in the buffer about to go)
    drop_pending(ar);
    if (ar.h) (void)hipHostFree(ar.h);
    if (ar.d) (void)hipFree(ar.d);
    ar.h = nullptr;
    ar.d = nullptr;
    ar.cap = 0;
    ar.device_bytes = 0;
    TD_HIP(hipHostMalloc(&ar.h, cap, hipHostMallocDefault));
    TD_HIP(hipMalloc(&ar.d, cap));
    if (!ar.copied) TD_HIP(hipEventCreateWithFlags(&ar.copied, hipEventDisableTiming));
    ar.cap = cap;
    ar.device_bytes = cap;
    ar.inflight = false;
    ar.valid = 0;
    ar.esync_len = 0;   // (new memory: the epoch-tagged words are zeroed by the next submission that has any)
    return 1;
}
static void free_arena(Arena& ar) {
    drop_pending(ar);
    if (ar.h) (void)hipHostFree(ar.h);
    if (ar.d) (void)hipFree(ar.d);
    if (ar.copied) (void)hipEventDestroy(ar.copied);
    if (ar.h_flag) (void)hipHostFree(ar.h_flag);
    if (ar.d_respec) (void)hipFree(ar.d_respec);
    ar = Arena{};
}


static hipEvent_t get_event(ProfCtx& pc) {
    if (!pc.free_ev.empty()) {
        hipEvent_t e = pc.free_ev.back();
        pc.free_ev.pop_back();
        return e;
    }
    hipEvent_t e = nullptr;
    (void)hipEventCreate(&e);
    return e;
}

struct Prof {
    ProfCtx& pc;
    int fam;
    hipStream_t s;
    hipEvent_t a = nullptr, b = nullptr;
    Prof(ProfCtx& pc_, int fam_, hipStream_t s_) : pc(pc_), fam(fam_), s(s_) {
        if (pc.now) {
            a = get_event(pc);
            b = get_event(pc);
            (void)hipEventRecord(a, s);
        }
    }
    ~Prof() {
        if (pc.now) {
            (void)hipEventRecord(b, s);
            pc.pending.push_back({a, b, fam});
        }
    }
};

// Steps 3 and 4 for everything compiled into `cb`: patch pointers, upload the tables (skipped when the device
// copy is already byte-identical), launch level by level on `stream`.  With several graphs in `cb` (a batch)
// the launches are first merged: same level, family, launch parameters -> ONE grid whose blockIdx.y runs over
// the descriptors of all the graphs (their descriptors are copied into one contiguous array behind the tables).
// *scratch_base = device address the scratch offsets of this submission refer to.  (Launches of one level go out on the ONE
// stream in launch order: a stream per independent branch -- built in round 2 -- cost more in fork / join events than the
// branches overlapped, 1.64 against 1.10 ms on the 60 s drum project; same-kind branches share a batched launch anyway.)
static int submit_chunk(Arena& ar, ChunkBuild& cb, hipStream_t stream, ProfCtx& prof, td_graph* /* the graph when there is ONE: unused */,
                        const uint8_t** scratch_base, double* host_ms /* [2]: upload, launches */) {
    const auto tp2 = std::chrono::steady_clock::now();
    Staging& st = *cb.st;
    std::vector<Launch>& launches = cb.launches;
    prof.now = prof.every && (prof.count++ % prof.every) == 0;
    struct Copy { size_t dst, src, bytes; };
    std::vector<Copy> copies;
    if (cb.n_graphs > 1) {
        auto key_less = [](const Launch& a, const Launch& b) {
            if (a.level != b.level) return a.level < b.level;
            if (a.fam != b.fam) return a.fam < b.fam;
            if (a.M != b.M) return a.M < b.M;
            if (a.bl != b.bl) return a.bl < b.bl;
            if (a.is_scan != b.is_scan) return a.is_scan < b.is_scan;
            if (is_delay_family(a.fam) && ((a.aux ^ b.aux) & kDelaySingleBit)) return a.aux < b.aux;   // (k_delay_apply's two instantiations stay apart)
            if (!is_band_family(a.fam) && !is_delay_family(a.fam) && a.aux != b.aux) return a.aux < b.aux;   // (those two: aux is the largest grid of the launch's descriptors)
            return false;
        };
        std::stable_sort(launches.begin(), launches.end(), key_less);
        std::vector<Launch> merged;
        merged.reserve(launches.size());
        for (size_t i = 0; i < launches.size();) {
            size_t j = i + 1;
            int n = launches[i].n;
            uint32_t aux = launches[i].aux;
            while (j < launches.size() && !key_less(launches[i], launches[j]) && !key_less(launches[j], launches[i])) {
                n += launches[j].n;
                aux = std::max(aux, launches[j].aux);   // (equal unless a band family: its largest segment count; or a delay family: its largest grid)
                ++j;
            }
            Launch L = launches[i];
            if (j - i > 1) {
                const size_t dsz = desc_size(L.fam);
                size_t dst = st.alloc((size_t)n * dsz);
                L.off = dst;
                L.n = n;
                L.aux = aux;
                for (size_t q = i; q < j; ++q) {
                    copies.push_back({dst, launches[q].off, (size_t)launches[q].n * dsz});
                    dst += (size_t)launches[q].n * dsz;
                }
            }
            merged.push_back(L);
            i = j;
        }
        launches.swap(merged);
    }
    // ---- 3. upload
    const size_t upload = (st.b.size() + 255) & ~(size_t)255;
    const size_t sync_at = upload + ((cb.scratch_bytes + 255) & ~(size_t)255);
    const size_t esync_at = sync_at + ((cb.sync_bytes + 255) & ~(size_t)255);
    if (!ensure_arena(ar, esync_at + cb.esync_bytes + 256, stream)) return 0;
    for (auto& f : cb.sync_fix) {
        uint64_t p = (uint64_t)(uintptr_t)(ar.d + sync_at + f.off);
        memcpy(&st.b[f.at], &p, 8);
    }
    for (auto& f : cb.esync_fix) {
        uint64_t p = (uint64_t)(uintptr_t)(ar.d + esync_at + f.off);
        memcpy(&st.b[f.at], &p, 8);
    }
    for (size_t at : cb.flag_fix) {
        uint64_t p = (uint64_t)(uintptr_t)ar.d_flag;
        memcpy(&st.b[at], &p, 8);
    }
    for (size_t at : cb.respec_fix) {
        uint64_t p = (uint64_t)(uintptr_t)ar.d_respec;
        memcpy(&st.b[at], &p, 8);
    }
    for (auto& f : cb.table_fix) {
        uint64_t p = (uint64_t)(uintptr_t)(ar.d + f.off);
        memcpy(&st.b[f.at], &p, 8);
    }
    for (auto& f : cb.scratch_fix) {
        uint64_t p = (uint64_t)(uintptr_t)(ar.d + upload + f.off);
        memcpy(&st.b[f.at], &p, 8);
    }
    for (auto& c : copies) memcpy(&st.b[c.dst], &st.b[c.src], c.bytes);
    *scratch_base = ar.d + upload;
    if (ar.inflight) TD_HIP(hipEventSynchronize(ar.copied));
    ar.inflight = false;
    // re-rendering unchanged projects from the same state compiles to byte-identical tables: the copy
    // already on the device is reused (kernels never write the uploaded region)
    if (!(ar.valid == st.b.size() && memcmp(ar.h, st.b.data(), st.b.size()) == 0)) {
        memcpy(ar.h, st.b.data(), st.b.size());
        if (debug_sync() & 1) TD_HIP(hipStreamSynchronize(stream));
        if (debug_sync() & 4) fprintf(stderr, "U arena %zu\n", st.b.size());
        TD_HIP(hipMemcpyAsync(ar.d, ar.h, st.b.size(), hipMemcpyHostToDevice, stream));
        TD_HIP(hipEventRecord(ar.copied, stream));
        if (debug_sync() & 2) TD_HIP(hipEventSynchronize(ar.copied));
        if (debug_sync() & 4) { (void)hipStreamSynchronize(stream); fprintf(stderr, "ok\n"); }
        debug_verify_upload("arena", ar.d, ar.h, st.b.size(), stream);
        ar.inflight = true;
        ar.valid = st.b.size();
    }
    for (auto& z : cb.zero) TD_HIP(hipMemsetAsync(ar.d + upload + z.off, 0, z.bytes, stream));
    if (debug_sync() & 4) { fprintf(stderr, "Z zero %zu\n", cb.zero.size()); (void)hipStreamSynchronize(stream); fprintf(stderr, "ok\n"); }
    // The launches of a level that read no edge buffer -- affine Synth, wavetable voice, SampleLerp, the envelope buffers -- go
    // out as ONE grid (k_sources, kernels.hip): the first launch of each kind, the longest-running kind first.  `pick`: the
    // launch index per SourceKind, -1: none; returns the common frame count, 0: no such grid for launches [li, lj).
    auto sources_grid = [&](size_t li, size_t lj, long pick[4]) -> uint32_t {
        pick[0] = pick[1] = pick[2] = pick[3] = -1;
        if (!cb.one_grid_sources || lj - li > 64) return 0u;
        uint32_t M0 = 0;
        int found = 0, n_desc = 0;
        for (size_t q = li; q < lj; ++q) {
            const Launch& L = launches[q];
            int kd = -1;
            switch (L.fam) {
                case F_SYNTH: kd = (L.aux & 1u) ? (int)SRC_SYNTH_AFFINE : -1; break;
                case F_SAMPSYN: kd = (int)SRC_SAMPSYN; break;
                case F_LERP: kd = (int)SRC_LERP; break;
                case F_ENV: kd = (int)SRC_ENV; break;
                default: break;
            }
            if (kd < 0 || pick[kd] >= 0 || !L.n || !L.M) continue;
            if (found && L.M != M0) continue;
            M0 = L.M;
            pick[kd] = (long)q;
            n_desc += L.n;
            ++found;
        }
        // (a large batch gains nothing -- its grids have no ramp or tail to speak of -- and the envelope part would run at the
        // Synth part's register budget: 32 config-3 projects measured 2 % slower in one grid, 8 the same)
        return (found >= 2 && n_desc <= 16) ? M0 : 0u;
    };
    // The zeroed hand-off words: by a fill kernel of their own -- or, when the submission opens with a k_sources grid, by that
    // grid's threads (everything that reads the words is behind it on the stream): one launch less in front of a scan render.
    bool zero_in_sources = false;
    if (cb.sync_bytes) {
        size_t l0 = 0;
        while (l0 < launches.size() && launches[l0].level == launches[0].level) ++l0;
        long pick0[4];
        zero_in_sources = !launches.empty() && cb.sync_bytes <= ((size_t)1 << 28) && sources_grid(0, l0, pick0) != 0u;
        if (!zero_in_sources) TD_HIP(hipMemsetAsync(ar.d + sync_at, 0, cb.sync_bytes, stream));
    }
    // The tile words of the stand-alone single-pass Normalize launches carry the submission's EPOCH beside their value (a
    // kernel argument: the descriptors stay byte-identical from render to render and are not uploaded again).  A word of an
    // earlier submission never compares equal, so the region is not zeroed between launches -- the memset was 2 us of the
    // headline render's 66.  It is zeroed once whenever it lies elsewhere than last time (what was there before is not
    // known to be words), when the arena is new, and before the epoch counter would wrap.  A captured submission
    uint32_t sum_tag = 1u;
    if (!cb.esync_bytes) ar.esync_len = 0;   // (this submission may write anything where the words lay)
    if (cb.esync_bytes) {
        if (ar.esync_at != esync_at || ar.esync_len != cb.esync_bytes || ar.epoch == 0xFFFFFFFFu) {
            TD_HIP(hipMemsetAsync(ar.d + esync_at, 0, cb.esync_bytes, stream));
            ar.esync_at = esync_at;
            ar.esync_len = cb.esync_bytes;
            if (ar.epoch == 0xFFFFFFFFu) ar.epoch = 1u;
        }
        sum_tag = ++ar.epoch;
    }

    // ---- 4. launch, level by level
    const auto tp3 = std::chrono::steady_clock::now();
    // (what an un-settled earlier submission left: prepare_render has settled it where its result is still needed.  If its
    // host-visible word is already up, the word is cleared ON THE STREAM -- behind that submission's launches, in front of this
    // one's -- so that it does not count against this submission at the next settle; the normal case is one host load.  A word
    // raised after this look costs one unnecessary k_norm_fix later, never a wrong result.)
    if (!ar.pending_fix.empty() && ar.h_flag && *(volatile uint32_t*)ar.h_flag)
        TD_HIP(hipMemsetD32Async((hipDeviceptr_t)ar.d_flag, 0, 1, stream));
    ar.pending_fix.clear();
    size_t li = 0;
    while (li < launches.size()) {
        size_t lj = li;
        while (lj < launches.size() && launches[lj].level == launches[li].level) ++lj;
        uint64_t in_one_grid = 0;   // bit q - li: launched as a part of the level's k_sources grid
        {
            long pick[4];
            const uint32_t M0 = sources_grid(li, lj, pick);
            if (M0) {
                SourceParts P{};
                for (int kd = 0; kd < 4; ++kd) {
                    if (pick[kd] < 0) continue;
                    const Launch& L = launches[(size_t)pick[kd]];
                    const void* d = ar.d + L.off;
                    switch (kd) {
                        case SRC_SYNTH_AFFINE: P.synth = (const SynthDesc*)d; P.n_synth = L.n; break;
                        case SRC_SAMPSYN: P.sampsyn = (const SampsynDesc*)d; P.n_sampsyn = L.n; break;
                        case SRC_LERP: P.lerp = (const LerpDesc*)d; P.n_lerp = L.n; break;
                        default: P.env = (const AdsrVDesc*)d; P.n_env = L.n; break;
                    }
                    in_one_grid |= 1ull << ((size_t)pick[kd] - li);
                }
                const bool z = zero_in_sources && li == 0;   // (the submission's first grid clears the hand-off words)
                Prof pr(prof, F_SOURCES, stream);
                if (debug_sync() & 4) fprintf(stderr, "L k_sources M=%u\n", M0);
                launch_sources(P, M0, z ? ar.d + sync_at : nullptr, z ? (cb.sync_bytes + 15) & ~(size_t)15 : 0, stream);
                if (debug_sync() & 4) { (void)hipStreamSynchronize(stream); fprintf(stderr, "ok\n"); }
            }
        }
        for (size_t q = li; q < lj; ++q) {
            const Launch& L = launches[q];
            if (in_one_grid & (1ull << (q - li))) continue;
            if (L.fam == F_NORMFIX && (L.aux & 1u)) {   // deferred: launched by settle_arena() only if a tile raised the host-visible word
                ar.pending_fix.push_back({L.off, L.n, L.M, L.bl});
                continue;
            }
            const void* d = ar.d + L.off;
            hipStream_t s = stream;
            Prof pr(prof, L.fam, s);
            if (debug_sync() & 4) fprintf(stderr, "L %s n=%d M=%u bl=%u aux=%x\n", kFamilyName[L.fam], L.n, L.M, L.bl, L.aux);
            struct Crumb { hipStream_t s; ~Crumb() { if (debug_sync() & 4) { (void)hipStreamSynchronize(s); fprintf(stderr, "ok\n"); } } } crumb{s};
            switch (L.fam) {
                case F_LOOP: launch_sample_loop((const LoopDesc*)d, L.n, L.M, s); break;
                case F_MULTI: launch_sample_multi((const MultiDesc*)d, L.n, L.M, s); break;
                case F_LERP: launch_sample_lerp((const LerpDesc*)d, L.n, L.M, s); break;
                case F_SINE: launch_debug_sine((const SineDesc*)d, L.n, L.M, L.bl, s); break;
                case F_SYNTH: launch_synth((const SynthDesc*)d, L.n, L.M, (L.aux & 1u) != 0u, s); break;
                case F_SAMPSYN: launch_sampsyn((const SampsynDesc*)d, L.n, L.M, s); break;
                case F_ENV: launch_adsr_env((const AdsrVDesc*)d, L.n, L.M, s); break;
                case F_PROBE: launch_sine_probe((const ProbeDesc*)d, L.n, L.M, L.aux, s); break;
                case F_SUM:
                    if ((L.aux >> 12) & 0xFu) launch_norm1((const SumDesc*)d, L.n, L.M, L.aux & 0xFFu, (int)((L.aux >> 12) & 0xFu), sum_tag, s);   // single-pass Normalize, narrow forms
                    else launch_sum((const SumDesc*)d, L.n, L.M, L.bl, L.aux & 0xFFFF00FFu, (L.aux & 0x100u) != 0u, (L.aux & 0x200u) != 0u, sum_tag, s);   // (bits 16 ..: the ragged form's grid)
                    break;
                case F_SCALE: launch_scale((const ScaleDesc*)d, L.n, L.M, L.bl, L.is_scan, s); break;
                case F_NORMFIX: launch_norm_fix((const SumDesc*)d, L.n, L.M, L.bl, s); break;
                case F_ADSR: launch_adsr((const AdsrVDesc*)d, L.n, L.M, L.aux & 0xFFu, s); break;
                case F_BAND: launch_band_pass((const BandDesc*)d, L.n, L.M, s); break;
                case F_BAND_SPEC: launch_band_spec((const BandSpecDesc*)d, L.n, L.M, L.aux, s); break;
                case F_BAND_FIX: launch_band_fix((const BandSpecDesc*)d, L.n, L.M, L.aux, s); break;
                case F_BAND_FILL: break;
                case F_BAND_SCAN:
                    if (L.aux & 0x10000u) launch_band_chain((const BandScanDesc*)d, L.n, L.M, L.aux & 0xFFu, (L.aux & 0x20000u) != 0u, s);
                    else launch_band_scan((const BandScanDesc*)d, L.n, L.M, L.aux & 0xFFu, (int)((L.aux >> 8) & 0xFFu), s);
                    break;
                case F_QUANT: launch_quantise((const QuantDesc*)d, L.n, L.M, s); break;
                case F_AUDIT: launch_band_audit((const AuditHead*)d, L.n, s); break;
                case F_STEMS: launch_stems((const StemDesc*)d, L.n, L.M, s); break;   // (prepare_render has checked it exists)
                default:   // an effect kind's family (likewise: prepare_render has checked that its kernels exist)
                    if (const FxKind* fx = fx_of_family(L.fam)) fx->launch(L, d, s);
                    break;
            }
        }
        li = lj;
    }
    TD_HIP(hipGetLastError());
    if (!ar.pending_fix.empty()) note_pending(ar, stream, cur_device());
    const auto tp4 = std::chrono::steady_clock::now();
    host_ms[0] += ms_between(tp2, tp3);   // arena upload (or the compare that skips it)
    host_ms[1] += ms_between(tp3, tp4);   // launches
    return 1;
}

// A render of n_blocks blocks runs in chunks of whole blocks (normally one).  The three pieces below are shared by the
// single-graph path (graph_render_chunks) and the batch path (batch_render_chunks), which interleaves them over its graphs.
struct RenderPlan {
    size_t n_blocks = 0, chunk_blocks = 1, total = 0;
    bool multi = false, want_pcm = false;
    int qmode = 0, bits = 16;
    float amplitude = 0.f;
    size_t word = 0;
};
// The stems' device side for a render of `frames` frames: PCM of `word`-byte samples (0: none), the peaks, the f32 copies of a
// resampled render.  Nothing in flight reads them: the caller has drained what used them before growing anything.
static int prepare_stems(td_graph* g, size_t frames, size_t word) {
    if (!launch_stems) return fail("termdaw_amd: this build has no k_stems kernel: stems cannot be rendered");
    const size_t n = g->stems.size();
    if (word) {
        const size_t stride = (frames * 2 * word + 64 + 255) & ~(size_t)255;
        if (n * stride > g->stem_pcm_cap) {
            if (!drain(g)) return 0;
            if (g->d_stem_pcm) { (void)hipFree(g->d_stem_pcm); g->device_bytes -= g->stem_pcm_cap; }
            g->d_stem_pcm = nullptr;
            g->stem_pcm_cap = 0;
            TD_HIP(hipMalloc(&g->d_stem_pcm, n * stride));
            g->stem_pcm_cap = n * stride;
            g->device_bytes += n * stride;
        }
        g->stem_stride = stride;
        g->stem_pcm_bytes = frames * 2 * word;
    }
    if (n > g->stem_peak_cap) {
        if (!drain(g)) return 0;
        if (g->d_stem_peak) { (void)hipFree(g->d_stem_peak); g->device_bytes -= g->stem_peak_cap * 4; }
        g->d_stem_peak = nullptr;
        g->stem_peak_cap = 0;
        TD_HIP(hipMalloc(&g->d_stem_peak, n * 4));
        g->stem_peak_cap = n;
        g->device_bytes += n * 4;
    }
    if (g->stem_f32_wanted) {
        const size_t stride = frames + 2;   // (float2 frames)
        if (n * stride * sizeof(float2) > g->stem_f32_cap) {
            if (!drain(g)) return 0;
            if (g->d_stem_f32) { (void)hipFree(g->d_stem_f32); g->device_bytes -= g->stem_f32_cap; }
            g->d_stem_f32 = nullptr;
            g->stem_f32_cap = 0;
            TD_HIP(hipMalloc(&g->d_stem_f32, n * stride * sizeof(float2)));
            g->stem_f32_cap = n * stride * sizeof(float2);
            g->device_bytes += g->stem_f32_cap;
        }
        g->stem_f32_stride = stride;
    }
    return 1;
}
// Does anything else in the render read the output's frames -- the output is a stem, or a stem sits downstream of it?  (Then
// compile_chunk keeps them in f32 whatever "output_f32" says: compile.cpp `out_read`.)
static bool output_read(const td_graph* g) {
    for (size_t sv : g->stems)
        if ((long)sv == g->output_vertex) return true;
    for (size_t vi : g->order) {
        for (size_t u : g->edges[vi])
            if ((long)u == g->output_vertex) return true;
        for (size_t u : g->key_edges[vi])
            if ((long)u == g->output_vertex) return true;
    }
    return false;
}
static int prepare_render(td_graph* g, size_t n_blocks, int bits, bool want_pcm, RenderPlan* rp) {
    if (!ensure_graph_device(g)) return 0;
    if (g->output_vertex < 0) return fail("TermDaw: error: output vertex not found.");
    if (g->plan_dirty) build_plan(g);
    if (!ensure_state_slots(g)) return 0;
    // the effect kinds' kernels are linked (a dry vertex compiles to a Sum: it needs none), the first kind of the table first
    for (int k = 0; k < K_COUNT; ++k) {
        const FxKind* fx = fx_kind((Kind)k);
        if (!fx || fx->built) continue;
        for (size_t vi : g->order)
            if (g->vertices[vi].kind == fx->kind && !(g->vertices[vi].wet < 0.0001f))
                return fail(std::string("termdaw_amd: this build has no k_") + fx->k + " kernels: " + fx->name + " vertices cannot be rendered");
    }
    for (size_t vi : g->order) {   // ... and the keyed forms, where a key edge asks for them (td_graph_connect_key)
        const Vertex& v = g->vertices[vi];
        if (g->key_edges[vi].empty() || v.wet < 0.0001f) continue;
        const FxKind* fx = fx_kind(v.kind);
        if (fx && !fx->keyed_built)
            return fail(std::string("termdaw_amd: this build has no keyed ") + fx->keyed_name + " kernels: a vertex with a key edge cannot be rendered");
    }
    const size_t bl = g->bl;
    if (bl == 0) return fail("termdaw_amd: buffer length 0");
    rp->n_blocks = n_blocks;
    rp->total = n_blocks * bl;
    rp->chunk_blocks = std::max<size_t>(1, g->max_chunk_frames / bl);
    rp->chunk_blocks = std::min(rp->chunk_blocks, std::max<size_t>(n_blocks, 1));
    rp->multi = n_blocks > rp->chunk_blocks;
    rp->want_pcm = want_pcm;
    rp->bits = bits;
    if (want_pcm) { g->loud_frames = 0; g->master_kept = false; }   // (d_pcm is about to be overwritten: measurable again when the render has finished)
    if (want_pcm) {
        if (!(bits == 8 || bits == 16 || bits == 24 || bits == 32))   // state.rs:495-501
            return fail("Bitdepth not supported: choose bitdepth in {8, 16, 24, 32}.");
        rp->qmode = bits > 16 ? 2 : 1;                                    // write_16s / write_32s, state.rs:567-571
        rp->amplitude = bits < 32 ? (float)((1 << (bits - 1)) - 1) : (float)INT32_MAX;   // state.rs:515-516
        rp->word = rp->qmode == 1 ? 2 : 4;
        const size_t need = rp->total * 2 * rp->word + 64;
        if (need > g->pcm_cap) {
            if (!drain(g)) return 0;
            if (g->d_pcm && !g->pcm_borrowed) { (void)hipFree(g->d_pcm); g->device_bytes -= g->pcm_cap; }
            g->d_pcm = nullptr;
            g->pcm_cap = 0;
            g->pcm_borrowed = false;
            TD_HIP(hipMalloc(&g->d_pcm, need));
            g->pcm_cap = need;
            g->device_bytes += need;
        }
        g->pcm_bytes = rp->total * 2 * rp->word;
    }
    if (!g->stems.empty() && (want_pcm || g->stem_f32_wanted) && !prepare_stems(g, rp->total, rp->word)) return 0;
    if (rp->multi) {
        const size_t need = (rp->total + 2) * sizeof(float2);
        if (need > g->out_f32_cap) {
            if (!drain(g)) return 0;
            if (g->d_out_f32) { (void)hipFree(g->d_out_f32); g->device_bytes -= g->out_f32_cap; }
            g->d_out_f32 = nullptr;
            g->out_f32_cap = 0;
            TD_HIP(hipMalloc(&g->d_out_f32, need));
            g->out_f32_cap = need;
            g->device_bytes += need;
        }
    }
    return 1;
}
// Snapshots the FlowwBank cursor of the next nb blocks (advancing the bank one block at a time exactly like
// state.rs:572 / graph.rs:232) and compiles the chunk into cb.
static int compile_next_chunk(td_graph* g, const td_samplebank* sb, td_flowwbank* fb, const RenderPlan& rp, size_t done,
                              size_t nb, bool is_scan, bool advance_graph_time, size_t scan_t0, ChunkBuild& cb) {
    const size_t bl = g->bl;
    std::vector<BlockCursor>& cur = g->cursor;   // (capacity kept from render to render)
    const size_t nfl = fb->start_indices.size();
    cur.resize(nb);
    g->cursor_starts.resize(nb * nfl + 1);
    for (size_t b = 0; b < nb; ++b) {
        size_t* s = g->cursor_starts.data() + b * nfl;
        for (size_t i = 0; i < nfl; ++i) s[i] = fb->start_indices[i];
        cur[b] = {fb->frame, s, nfl};
        fb->set_time_to_next_block();
    }
    const uint64_t t0 = advance_graph_time ? g->t : scan_t0 + done * bl;
    g->chunk_frame0 = done * bl;
    void* pcm_dst = rp.want_pcm ? (uint8_t*)g->d_pcm + done * bl * 2 * rp.word : nullptr;
    return compile_chunk(g, sb, fb, cur, t0, is_scan, pcm_dst, rp.qmode, rp.amplitude, cb);
}
static int finish_chunk(td_graph* g, const RenderPlan& rp, size_t done, size_t nb, bool advance_graph_time,
                        const uint8_t* scratch_base) {
    g->band_stats_base = scratch_base;
    if (!g->conv_checks.empty()) {
        // the submission built the spectra of convolution vertices with `norm`: an all-zero response has no energy to normalise to
        const std::vector<size_t> checks = g->conv_checks;
        g->conv_checks.clear();
        TD_HIP(hipStreamSynchronize(g->stream));
        for (size_t vi : checks) {
            double e[2] = {0.0, 0.0};
            TD_HIP(hipMemcpy(e, g->vertices[vi].spectra.d, sizeof e, hipMemcpyDeviceToHost));
            if (!(std::max(e[0], e[1]) > 0.0)) {
                forget_spectra(g);
                return fail("convolution: norm is 1 and the response of vertex '" + g->vertices[vi].name + "' is all zero (or not finite)");
            }
        }
    }
    if (advance_graph_time) g->t += nb * g->bl;
    if (rp.multi)
        TD_HIP(hipMemcpyAsync(g->d_out_f32 + done * g->bl, g->vbuf[(size_t)g->output_vertex], nb * g->bl * sizeof(float2),
                              hipMemcpyDeviceToDevice, g->stream));
    return 1;
}
static void finish_render(td_graph* g, const RenderPlan& rp) {
    g->last_out_f32 = rp.multi ? g->d_out_f32 : (rp.n_blocks ? g->vbuf[(size_t)g->output_vertex] : nullptr);
    if (!g->output_f32 && !output_read(g) && rp.want_pcm && g->vertices[(size_t)g->output_vertex].kind == K_NORMALIZE)
        g->last_out_f32 = nullptr;   // (the f32 frames of the output were never written)
    g->last_frames = rp.total;
    g->last_bits = rp.bits;
    if (rp.want_pcm) { g->loud_frames = rp.total; g->loud_bits = rp.bits; g->loud_sr = g->sr; }
}

// Everything queued for the graph has completed AND a deferred k_norm_fix has run if one was called for (settle_arena): the
// point from which results -- PCM, f32 frames, carried Normalize state -- may be read.
static int guard_settle(td_graph* g);
static int graph_set_time_impl(td_graph* g, size_t time);
static int drain(td_graph* g) {
    if (!g->stream) return 1;
    if (!ensure_device(g->device)) return 0;
    if (!settle_arena(g->arena, g->stream)) return 0;
    if (g->batch && g->batch->stream && !settle_arena(g->batch->arena, g->batch->stream)) return 0;
    return guard_settle(g);
}
// A render whose output Normalize vertex continues from its carried max needs the previous render's deferred fix settled
// first (a render that starts from reset_normalization does not read it: back-to-back fresh renders never wait here).
// ---- the guard (band_mode 2): engine.h tde::Guard
// Does the render about to start read any carried device state?  Not if every reachable vertex with a state slot starts
// afresh: a Normalize vertex with reset_normalization pending, a band-pass vertex with set_time pending.
static bool starts_afresh(const td_graph* g) {
    for (size_t vi : g->order) {
        const Vertex& v = g->vertices[vi];
        if (v.kind == K_NORMALIZE && !v.has_init_override) return false;
        if (((v.kind == K_BAND_PASS && v.state_slot >= 0) || slot_kind(v)) && !v.first_pending) return false;
        if (v.line.d && !v.first_pending) return false;
    }
    return true;
}
static bool has_reachable_band(const td_graph* g) {
    for (size_t vi : g->order)
        if (g->vertices[vi].kind == K_BAND_PASS) return true;
    return false;
}
// May the render about to start carry an audit?  band_mode 2 with a band-pass vertex on the way to the output, or sine_mode 2
// with a debug_sine / synth vertex there (k_sine_probe's measurements: kernels.h ProbeDesc).
static bool may_be_audited(const td_graph* g) {
    if (g->guard.in_redo) return false;
    if (g->band_mode == 2 && has_reachable_band(g)) return true;
    if (g->sine_mode == 2)
        for (size_t vi : g->order)
            if (g->vertices[vi].kind == K_DEBUG_SINE || g->vertices[vi].kind == K_SYNTH) return true;
    return false;
}
// In front of a render that may carry an audit: what it takes to do the render again (called once the plan and the state
// slots are in place, before the first chunk compiles).
static int guard_begin(td_graph* g, const td_samplebank* sb, td_flowwbank* fb, size_t n_blocks, bool is_scan, int bits,
                       bool advance, size_t scan_t0, bool want_pcm) {
    Guard& q = g->guard;
    q.sb = sb; q.fb = fb; q.n_blocks = n_blocks; q.is_scan = is_scan; q.bits = bits; q.advance = advance; q.scan_t0 = scan_t0;
    q.want_pcm = want_pcm;
    q.post = 0;
    q.snap.take(g, fb);
    q.have_backup = false;
    if (!starts_afresh(g) && g->dstate && !g->hstate.empty()) {
        const size_t n = g->hstate.size();
        if (n > q.backup_cap) {
            if (q.d_backup) (void)hipFree(q.d_backup);
            q.d_backup = nullptr;
            q.backup_cap = 0;
            TD_HIP(hipMalloc(&q.d_backup, n * 2 * sizeof(StateSlot)));
            q.backup_cap = n * 2;
        }
        TD_HIP(hipMemcpyAsync(q.d_backup, g->dstate, n * sizeof(StateSlot), hipMemcpyDeviceToDevice, g->stream));
        q.have_backup = true;
    }
    // the lines of the delay, saturator, chorus and reverb vertices that continue from what they hold (a vertex with a set_time pending reads nothing
    // of its line)
    q.lines.clear();
    size_t need = 0;
    for (size_t vi : g->order) {
        const Vertex& v = g->vertices[vi];
        if (!carried_line(v)) continue;
        q.lines.push_back({vi, need, v.line.bytes});
        need += v.line.bytes;
    }
    if (need > q.lines_cap) {
        if (q.d_lines) (void)hipFree(q.d_lines);
        q.d_lines = nullptr;
        q.lines_cap = 0;
        uint8_t* p = nullptr;
        TD_HIP(hipMalloc(&p, need));
        q.d_lines = p;
        q.lines_cap = need;
    }
    for (const auto& l : q.lines)
        TD_HIP(hipMemcpyAsync((uint8_t*)q.d_lines + l.off, g->vertices[l.vertex].line.d, l.bytes, hipMemcpyDeviceToDevice, g->stream));
    return 1;
}
// The stream has drained: look at the verdict of the last guarded render, and do that render again with the exact kernels
// if its estimate was over the bound.
static int guard_settle(td_graph* g) {
    Guard& q = g->guard;
    if (!q.armed || q.in_redo || !q.h_word) return 1;
    q.armed = false;
    const uint32_t raised = *(volatile uint32_t*)q.h_word;
    const uint32_t bits = *(volatile uint32_t*)(q.h_word + 1);
    memcpy(&q.last_est, &bits, 4);
    if (q.last_est > q.max_est || !(q.last_est == q.last_est)) q.max_est = q.last_est;
    if (!raised) return 1;
    *(volatile uint32_t*)q.h_word = 0u;
    q.in_redo = true;
    const int mode = g->band_mode;
    g->band_mode = 0;
    // The host side of the project as it stands NOW -- behind the render, behind whatever its caller did next (set_time(0) of
    // State::render, a FlowwBank cursor put back, reset_normalize_vertices for the next render): none of it depends on the
    // band-pass arithmetic, so the second render leaves the host side exactly where the first left it, and what stands now is
    // what has to stand afterwards.  Only the device side -- filter states, running peaks, the frames -- differs.
    HostSnapshot now;
    now.take(g, q.fb);
    q.snap.put(g, q.fb);
    int ok = 1;
    if (q.have_backup && hipMemcpyAsync(g->dstate, q.d_backup, g->hstate.size() * sizeof(StateSlot), hipMemcpyDeviceToDevice, g->stream) != hipSuccess)
        ok = fail("HIP error: the guard could not restore the carried state");
    for (const auto& l : q.lines)
        if (ok && l.vertex < g->vertices.size() && g->vertices[l.vertex].line.d && g->vertices[l.vertex].line.bytes == l.bytes &&   // (a convolution vertex whose response changed size has a new line)
            hipMemcpyAsync(g->vertices[l.vertex].line.d, (const uint8_t*)q.d_lines + l.off, l.bytes, hipMemcpyDeviceToDevice, g->stream) != hipSuccess)
            ok = fail("HIP error: the guard could not restore a delay line");
    g->state_dev_dirty = true;
    if (ok) ok = graph_render_chunks(g, q.sb, q.fb, q.n_blocks, q.is_scan, q.bits, q.advance, q.scan_t0, q.want_pcm);
    now.put(g, q.fb);
    g->band_mode = mode;
    q.in_redo = false;
    q.redos += 1;
    if (!ok) return 0;
    return settle_arena(g->arena, g->stream);   // (the second render's own deferred check, and its completion)
}

static int settle_before_render(td_graph* g) {
    // (a guarded render's verdict is still out and this render continues from the state it left: settle it first)
    if (g->guard.armed && !g->guard.in_redo && !(g->plan_dirty ? false : starts_afresh(g)) && !drain(g)) return 0;
    const bool pending = !g->arena.pending_fix.empty() || (g->batch && !g->batch->arena.pending_fix.empty());
    if (!pending || g->output_vertex < 0) return 1;
    const Vertex& ov = g->vertices[(size_t)g->output_vertex];
    if (ov.kind == K_NORMALIZE && ov.has_init_override) return 1;
    return drain(g);
}

// What compiling a chunk changes on the host side of a project -- loop cursors, the carried state of event-driven vertices,
// a pending reset_normalization, the playhead, the FlowwBank cursor -- so that a step that fails while compiling a LATER project
// of the batch (or a later chunk) can put every project back where the step found it: a retry then renders the same thing.
void HostSnapshot::take(const td_graph* g, const td_flowwbank* fb) {
    t = g->t;
    fb_frame = fb->frame;
    fb_start = fb->start_indices;
    v.resize(g->vertices.size());
    for (size_t i = 0; i < v.size(); ++i) {
        const Vertex& x = g->vertices[i];
        v[i].loop_t = x.loop_t;
        v[i].total = x.line.total;
        v[i].parity = x.line.parity;
        v[i].has_init_override = x.has_init_override;
        v[i].peak_known = x.peak_known;
        v[i].first_pending = x.first_pending;
        v[i].init_override = x.init_override;
        v[i].state.clear();
        save_state(x, v[i].state);
    }
}
void HostSnapshot::put(td_graph* g, td_flowwbank* fb) const {
    g->t = t;
    fb->frame = fb_frame;
    fb->start_indices = fb_start;
    for (size_t i = 0; i < v.size() && i < g->vertices.size(); ++i) {
        Vertex& x = g->vertices[i];
        x.loop_t = v[i].loop_t;
        x.line.total = v[i].total;
        x.line.parity = v[i].parity;
        x.has_init_override = v[i].has_init_override;
        x.peak_known = v[i].peak_known;
        x.first_pending = v[i].first_pending;
        x.init_override = v[i].init_override;
        load_state(x, v[i].state);
    }
}

// Renders n_blocks blocks in chunks.  advance_graph_time: Graph::render semantics (t += bl per block);
// otherwise the scan's explicit j*bl clock starting at scan_t0 (graph.rs:229-233).
int graph_render_chunks(td_graph* g, const td_samplebank* sb, td_flowwbank* fb, size_t n_blocks, bool is_scan,
                        int bits, bool advance_graph_time, size_t scan_t0, bool want_pcm) {
    RenderPlan rp;
    if (!settle_before_render(g)) return 0;
    if (!prepare_render(g, n_blocks, bits, want_pcm, &rp)) return 0;
    g->defer_fix = !rp.multi;   // (a later chunk reads the carried max; the f32 copy of a multi-chunk render reads the frames)
    g->batch_projects = 1;
    const bool guarded = may_be_audited(g);
    if (guarded && !guard_begin(g, sb, fb, n_blocks, is_scan, bits, advance_graph_time, scan_t0, want_pcm)) return 0;
    if (!g->stems.empty() && !is_scan && (want_pcm || g->stem_f32_wanted)) {   // (the stems' peaks accumulate over the render's chunks)
        TD_HIP(hipMemsetAsync(g->d_stem_peak, 0, g->stems.size() * 4, g->stream));
        g->stems_rendered = g->stems.size();
    }
    bool audited = false;
    ChunkBuild& cb = g->build;
    cb.st = &g->staging;
    // (a graph that belongs to a batch may still render alone: it then uses its own arena on the shared stream)
    size_t done = 0;
    while (done < n_blocks) {
        const size_t nb = std::min(rp.chunk_blocks, n_blocks - done);
        cb.clear();
        g->snapshot.take(g, fb);   // (a chunk that fails to compile or to submit leaves the host state where it found it)
        if (!compile_next_chunk(g, sb, fb, rp, done, nb, is_scan, advance_graph_time, scan_t0, cb)) {
            g->snapshot.put(g, fb);
            forget_spectra(g);
            return 0;
        }
        audited = audited || (guarded && g->guard.chunk_audited);
        const uint8_t* scratch_base = nullptr;
        if (!submit_chunk(g->arena, cb, g->stream, g->prof, g, &scratch_base, &g->host_ms[2])) {
            g->snapshot.put(g, fb);
            forget_spectra(g);
            return 0;
        }
        g->host_chunks += 1;
        if (!finish_chunk(g, rp, done, nb, advance_graph_time, scratch_base)) return 0;
        done += nb;
    }
    finish_render(g, rp);
    if (audited) { g->guard.armed = true; g->guard.audits += 1; }
    return 1;
}

static int graph_set_time_impl(td_graph* g, size_t time) {   // graph.rs:123-128 + extensions.rs:196-204
    g->t = time;
    bool any_band = false;
    for (auto& v : g->vertices) {
        switch (v.kind) {
            case K_SAMPLE_LOOP: v.loop_t = time; break;
            case K_DEBUG_SINE: v.sine_notes.clear(); break;
            case K_SYNTH: v.notes.clear(); break;
            case K_BAND_PASS:
                if (v.state_slot >= 0) {
                    g->hstate[v.state_slot].band.first = 1u;
                    v.first_pending = true;
                    any_band = true;
                }
                break;
            default: {   // an effect kind: its slots restart from the state at time 0, of its line the next submission reads no word (an LFO runs on: the graph's time)
                const FxKind* fx = fx_kind(v.kind);
                if (!fx || (fx->state_slots && v.state_slot < 0)) break;
                if (fx->state_slots) fx->put_rest(g, v, &g->hstate[(size_t)v.state_slot]);
                v.first_pending = true;
                break;
            }
        }
    }
    (void)any_band;   // (no device work: the next submission's descriptors carry the vertices' first_override)
    return 1;
}

// ------------------------------------------------------------------------------------------------
// batch: many independent projects per submission (BASELINE config 5)
// ------------------------------------------------------------------------------------------------
// The same chunk loop as graph_render_chunks, interleaved over the graphs of the batch: every graph compiles its
// chunk into the batch's ChunkBuild, ONE submission uploads the tables and launches the merged grids.  Graphs
// may differ in everything (structure, block length, chunk cap); launches merge only where level, family and
// launch parameters agree.
// Projects [lo, hi) of the batch.  allow_defer: nothing is submitted through the batch's arena before the caller settles it
// (a deferred k_norm_fix lives in the arena's LAST submission only).
static int batch_render_range(td_batch* b, size_t lo, size_t hi, size_t n_blocks, bool is_scan, int bits, bool advance_graph_time,
                              bool want_pcm, bool allow_defer) {
    if (hi <= lo) return 1;
    for (size_t i = lo; i < hi; ++i)
        if (!b->graphs[i]->stems.empty()) return fail("td_batch: project " + std::to_string(i) + " has stems set: batches do not render stems");
    if (!ensure_device(b->device)) return 0;
    const size_t P = hi - lo;
    std::vector<RenderPlan> rp(P);
    for (size_t i = 0; i < P; ++i) {
        td_graph* g = b->graphs[lo + i];
        if (!settle_before_render(g)) return 0;
        if (!prepare_render(g, n_blocks, bits, want_pcm, &rp[i])) return 0;
    }
    // A deferred k_norm_fix lives in the arena's LAST submission only: where any project of the range takes several chunks --
    // several submissions through this arena -- no project's check may be deferred (the later submissions would drop it).
    bool any_multi = false;
    for (size_t i = 0; i < P; ++i) any_multi = any_multi || rp[i].multi;
    for (size_t i = 0; i < P; ++i) {
        td_graph* g = b->graphs[lo + i];
        g->defer_fix = allow_defer && !any_multi;
        g->batch_projects = P;
        if (may_be_audited(g) &&
            !guard_begin(g, b->sbs[lo + i], b->fbs[lo + i], n_blocks, is_scan, bits, advance_graph_time, 0, want_pcm)) return 0;
    }
    ChunkBuild& cb = b->build;
    cb.st = &b->staging;
    std::vector<size_t> done(P, 0), nb(P, 0);
    for (;;) {
        const auto t0 = std::chrono::steady_clock::now();
        cb.clear();
        bool any = false;
        // (a failing step must not leave the projects compiled before the failure half-advanced: cursors, loop positions,
        // carried voices, a consumed reset_normalization all go back to where this step found them)
        auto roll_back = [&]() {
            for (size_t q = 0; q < P; ++q)
                if (nb[q]) { b->graphs[lo + q]->snapshot.put(b->graphs[lo + q], b->fbs[lo + q]); forget_spectra(b->graphs[lo + q]); }
        };
        for (size_t i = 0; i < P; ++i) nb[i] = std::min(rp[i].chunk_blocks, n_blocks - done[i]);
        for (size_t i = 0; i < P; ++i)
            if (nb[i]) b->graphs[lo + i]->snapshot.take(b->graphs[lo + i], b->fbs[lo + i]);
        for (size_t i = 0; i < P; ++i) {
            if (!nb[i]) continue;
            any = true;
            if (!compile_next_chunk(b->graphs[lo + i], b->sbs[lo + i], b->fbs[lo + i], rp[i], done[i], nb[i], is_scan, advance_graph_time, 0, cb)) {
                roll_back();
                return 0;
            }
            // (this project's chunk carries an audit: its verdict is looked at when the batch is settled)
            if (b->graphs[lo + i]->guard.chunk_audited && !b->graphs[lo + i]->guard.armed) { b->graphs[lo + i]->guard.armed = true; b->graphs[lo + i]->guard.audits += 1; }
        }
        if (!any) break;
        const uint8_t* scratch_base = nullptr;
        b->host_ms[0] += ms_between(t0, std::chrono::steady_clock::now());
        if (!submit_chunk(b->arena, cb, b->stream, b->prof, nullptr, &scratch_base, &b->host_ms[2])) {
            roll_back();   // (host side only: what the device has already run of this step cannot be taken back)
            return 0;
        }
        for (size_t i = 0; i < P; ++i) {
            if (!nb[i]) continue;
            if (!finish_chunk(b->graphs[lo + i], rp[i], done[i], nb[i], advance_graph_time, scratch_base)) return 0;
            done[i] += nb[i];
        }
        b->host_steps += 1;
    }
    for (size_t i = 0; i < P; ++i) finish_render(b->graphs[lo + i], rp[i]);
    return 1;
}
static int batch_render_chunks(td_batch* b, size_t n_blocks, bool is_scan, int bits, bool advance_graph_time, bool want_pcm) {
    return batch_render_range(b, 0, b->graphs.size(), n_blocks, is_scan, bits, advance_graph_time, want_pcm, true);
}

}  // namespace tde

// ---- what the C ABI's td_graph_add_* share: a vertex, a state slot, an effect vertex (add_fx: the project front end's too, compile.h) ----
// A guarded render whose verdict is still out is settled before the graph it was rendered from changes shape (band_mode 2:
// the render is done again from a snapshot of THIS graph's vertices).
static void settle_guard_before_edit(td_graph* g) {
    if (g->guard.armed && !g->guard.in_redo) (void)drain(g);
}
static Vertex& add_vertex(td_graph* g, const char* name, float gain, float angle, float wet, Kind kind) {
    settle_guard_before_edit(g);
    Vertex v;
    v.kind = kind;
    v.name = name;
    v.gain = gain;
    v.angle = fmaxf(fminf(angle, 90.0f), -90.0f);   // graph.rs:255
    v.wet = fmaxf(fminf(wet, 1.0f), 0.0f);          // graph.rs:256
    g->vertices.push_back(v);
    g->edges.emplace_back();
    g->key_edges.emplace_back();
    g->name_map[name] = g->vertices.size() - 1;     // later duplicates overwrite (graph.rs:54)
    g->plan_dirty = true;
    return g->vertices.back();
}
static int new_slot(td_graph* g) {
    // a freshly constructed slot makes the host mirror authoritative: fetch device values first
    pull_state(g);
    StateSlot s;
    memset(&s, 0, sizeof s);
    g->hstate.push_back(s);
    g->state_host_dirty = true;
    return (int)g->hstate.size() - 1;
}
// A kind's check of a block, by name: "<kind>: <reason>"
static int fx_check(Kind k, size_t sr, const FxParams& p) {
    const FxKind* fx = fx_kind(k);
    if (const char* why = fx->check(sr, p, false)) return fail(std::string(fx->name) + ": " + why);
    return 1;
}
// An effect vertex (compile.h): its kind's check, the state slots the kind carries (FxKind::state_slots), the vertex, the block as
// the kind keeps it.  The slots first: new_slot pulls the state of the vertices that exist.  They are zeroed: every kind's state
// at time 0 but the gate's, which needs the vertex' parameters (FxKind::rest).
int tde::add_fx(td_graph* g, Kind k, const char* name, float gain, float angle, float wet, const FxParams& p, size_t sample_index) {
    if (!fx_check(k, g->sr, p)) return 0;
    const FxKind* fx = fx_kind(k);
    const int n = fx->state_slots, slot = n ? new_slot(g) : -1;
    for (int i = 1; i < n; ++i) new_slot(g);
    Vertex& v = add_vertex(g, name, gain, angle, wet, k);
    v.state_slot = slot;
    v.sample_index = sample_index;
    v.fx = p;
    if (fx->settle) fx->settle(v.fx);
    v.first_pending = fx->starts_pending;
    if (fx->rest) fx->put_rest(g, v, &g->hstate[(size_t)v.state_slot]);
    return 1;
}

// =================================================================================================
// C ABI
// =================================================================================================
extern "C" {

const char* td_last_error(void) { return g_error.c_str(); }

int td_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}
int td_set_device(int device) {
    if (!ensure_device(device)) return 0;
    t_device = device;
    return 1;
}

// ---- SampleBank ----
td_samplebank* td_samplebank_new(size_t sample_rate) {
    td_samplebank* sb = new td_samplebank();
    sb->sample_rate = sample_rate;
    sb->device = t_device;
    return sb;
}
void td_samplebank_free(td_samplebank* sb) {
    if (!sb) return;
    if (hipSetDevice(sb->device) == hipSuccess) {
        for (auto& e : sb->samples) { sb->release(e.d); sb->release(e.d16); }
        sb->release_all();
        if (sb->tmp) (void)hipFree(sb->tmp);
    }
    delete sb;
}
int td_samplebank_add_decoded(td_samplebank* sb, const char* name, const float* linear, size_t n, int channels,
                              size_t sample_rate, size_t bits, const char* method) {
    return bank_add_stream(sb, name, linear, nullptr, PCM_F32, n, channels, sample_rate, bits, method_from(method));
}
int td_samplebank_add_file(td_samplebank* sb, const char* name, const char* path, const char* method) {
    if (sb->names.count(name))
        return fail(std::string("TermDaw: SampleBank: there is already a sample with name \"") + name + "\" present.");
    tdw::WavRaw w;
    std::string err;
    if (!tdw::read_wav_raw(path, &w, &err)) return fail(err);
    const uint32_t fmt = w.is_float ? PCM_F32 : (w.bits == 8 ? PCM_U8 : w.bits == 16 ? PCM_S16 : w.bits == 24 ? PCM_S24 : PCM_S32);
    return bank_add_stream(sb, name, nullptr, w.bytes.data(), fmt, w.n_values, w.channels, w.sample_rate, w.bits, method_from(method));
}
long td_samplebank_get_index(const td_samplebank* sb, const char* name) {
    auto it = sb->names.find(name);
    return it == sb->names.end() ? -1 : (long)it->second;
}
size_t td_samplebank_sample_len(const td_samplebank* sb, size_t index) {
    return index < sb->samples.size() ? sb->samples[index].len : 0;
}
int td_samplebank_read(const td_samplebank* sb, size_t index, float* l, float* r) {
    if (index >= sb->samples.size()) return fail("sample index out of range");
    if (!ensure_device(sb->device)) return 0;
    const SampleEntry& e = sb->samples[index];
    std::vector<float2> tmp(e.len);
    TD_HIP(hipMemcpy(tmp.data(), e.d, e.len * sizeof(float2), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < e.len; ++i) {
        l[i] = tmp[i].x;
        r[i] = tmp[i].y;
    }
    return 1;
}
void td_samplebank_get_max_sr_bd(const td_samplebank* sb, size_t* max_sr, size_t* max_bd) {
    if (max_sr) *max_sr = sb->max_sr;
    if (max_bd) *max_bd = sb->max_bd;
}

// ---- FlowwBank ----
td_flowwbank* td_flowwbank_new(size_t sr, size_t bl) {
    td_flowwbank* fb = new td_flowwbank();
    fb->sr = sr;
    fb->bl = bl;
    return fb;
}
void td_flowwbank_free(td_flowwbank* fb) { delete fb; }
void td_flowwbank_reset(td_flowwbank* fb) {
    fb->frame = 0;
    fb->flowws.clear();
    fb->start_indices.clear();
    fb->names.clear();
    fb->stream_list.clear();
    fb->versions.clear();
}
long td_flowwbank_add_events(td_flowwbank* fb, const char* name, const td_event* events, size_t n) {
    fb->flowws.emplace_back(events, events + n);
    fb->versions.push_back(td_flowwbank::next_version());
    fb->start_indices.push_back(0);
    const size_t index = fb->flowws.size() - 1;
    fb->names[name] = index;
    return (long)index;
}
long td_flowwbank_declare_stream(td_flowwbank* fb, const char* name) {
    long i = td_flowwbank_add_events(fb, name, nullptr, 0);
    fb->stream_list.push_back((size_t)i);
    return i;
}
long td_flowwbank_add_midi(td_flowwbank* fb, const char* name, const char* path) {
    std::vector<td_event> ev;
    std::string err;
    if (!tde::read_midi_file(path, &ev, &err)) {
        fail(std::string("Could not read midi file: \"") + path + "\" (" + err + ").");   // floww.rs:45-46
        return -1;
    }
    return td_flowwbank_add_events(fb, name, ev.data(), ev.size());
}
long td_flowwbank_append_stream(td_flowwbank* fb, const char* name, const td_event* events, size_t n) {
    auto it = fb->names.find(name);
    if (it == fb->names.end()) return -1;
    auto& f = fb->flowws[it->second];
    f.insert(f.end(), events, events + n);
    fb->versions[it->second] = td_flowwbank::next_version();
    return (long)f.size();
}
void td_flowwbank_trim_streams(td_flowwbank* fb) {   // start_indices are not rewound (floww.rs:59-64)
    for (size_t index : fb->stream_list) {
        auto& f = fb->flowws[index];
        f.erase(f.begin(), f.begin() + (long)std::min(fb->start_indices[index], f.size()));
        fb->versions[index] = td_flowwbank::next_version();
    }
}
size_t td_flowwbank_get_events(const td_flowwbank* fb, size_t index, td_event* out, size_t cap) {
    if (index >= fb->flowws.size()) return 0;
    const auto& f = fb->flowws[index];
    for (size_t i = 0; i < f.size() && i < cap; ++i) out[i] = f[i];
    return f.size();
}
long td_flowwbank_get_index(const td_flowwbank* fb, const char* name) {
    auto it = fb->names.find(name);
    return it == fb->names.end() ? -1 : (long)it->second;
}
void td_flowwbank_set_time(td_flowwbank* fb, size_t t) { fb->set_time(t); }
void td_flowwbank_set_time_to_next_block(td_flowwbank* fb) { fb->set_time_to_next_block(); }

// ---- Graph ----
td_graph* td_graph_new(size_t max_buffer_len, size_t sr) {
    td_graph* g = new td_graph();
    g->bl = max_buffer_len;
    g->sr = sr;
    g->device = t_device;
    return g;
}
static void free_prof(ProfCtx& pc) {
    for (auto& e : pc.pending) { (void)hipEventDestroy(e.a); (void)hipEventDestroy(e.b); }
    for (auto e : pc.free_ev) (void)hipEventDestroy(e);
    pc.pending.clear();
    pc.free_ev.clear();
}
void td_graph_free(td_graph* g) {
    if (!g) return;
    // (a deferred k_norm_fix -- the graph's own arena's or its batch's -- holds pointers into this graph's state: settled first)
    g->guard.armed = false;   // (nobody will read a render of this graph again: its verdict is dropped, not acted on)
    if (g->stream && hipSetDevice(g->device) == hipSuccess) (void)drain(g);
    if (g->batch) {   // leave the batch first: it must not keep a dangling handle
        td_batch* b = g->batch;
        for (size_t i = 0; i < b->graphs.size(); ++i)
            if (b->graphs[i] == g) {
                b->graphs.erase(b->graphs.begin() + (long)i);
                b->sbs.erase(b->sbs.begin() + (long)i);
                b->fbs.erase(b->fbs.begin() + (long)i);
                break;
            }
    }
    const bool has_device_state = g->stream || !g->pool.empty() || !g->wavetables.empty() || has_lines(g) || g->dstate || g->arena.d || g->d_pcm ||
                                  g->d_out_f32 || g->d_resampled || g->d_scalar || g->d_stem_pcm || g->d_stem_peak || g->d_stem_f32 ||
                                  g->d_loud || g->d_master_src || g->d_master;
    if (has_device_state && hipSetDevice(g->device) == hipSuccess) {
        if (g->stream) (void)hipStreamSynchronize(g->stream);
        else (void)hipDeviceSynchronize();   // (a graph whose stream could not be re-made after td_batch_free)
        for (float2* p : g->pool) (void)hipFree(p);
        for (float* p : g->wavetables) (void)hipFree(p);
        free_lines(g, true);
        free_tables(g);
        if (g->dstate) (void)hipFree(g->dstate);
        free_arena(g->arena);
        if (g->d_pcm && !g->pcm_borrowed) (void)hipFree(g->d_pcm);
        if (g->d_out_f32) (void)hipFree(g->d_out_f32);
        if (g->d_resampled) (void)hipFree(g->d_resampled);
        if (g->d_stem_pcm) (void)hipFree(g->d_stem_pcm);
        if (g->d_stem_peak) (void)hipFree(g->d_stem_peak);
        if (g->d_stem_f32) (void)hipFree(g->d_stem_f32);
        if (g->d_loud) (void)hipFree(g->d_loud);
        if (g->d_master_src) (void)hipFree(g->d_master_src);
        if (g->d_master) (void)hipFree(g->d_master);
        if (g->d_scalar) (void)hipFree(g->d_scalar);
        if (g->guard.d_backup) (void)hipFree(g->guard.d_backup);
        if (g->guard.d_lines) (void)hipFree(g->guard.d_lines);
        if (g->guard.h_word) (void)hipHostFree(g->guard.h_word);
        free_prof(g->prof);
        if (g->owns_stream && g->stream) (void)hipStreamDestroy(g->stream);
    }
    drop_pending(g->arena);   // (off the process-wide list whatever happened above: the list holds the arena's address)
    delete g;
}
void td_graph_reset(td_graph* g) {
    g->guard.armed = false;   // (the vertices a pending verdict is about are going)
    if ((g->stream || !g->wavetables.empty() || has_lines(g)) && hipSetDevice(g->device) == hipSuccess) {
        if (g->stream) (void)drain(g);   // (a deferred k_norm_fix belongs to the vertices about to go)
        for (float* p : g->wavetables) (void)hipFree(p);
        free_lines(g, true);
        free_tables(g);
    }
    g->wavetables.clear();
    free_lines(g, false);   // (lines that could not be given back above -- no device)
    g->guard.lines.clear();
    g->vertices.clear();
    g->edges.clear();
    g->key_edges.clear();
    g->name_map.clear();
    g->output_vertex = -1;
    g->stems.clear();
    g->stems_rendered = 0;
    g->stem_taps = 0;
    g->loud_frames = 0;
    g->master_kept = false;
    g->momentary.clear();
    g->t = 0;
    g->hstate.clear();
    g->state_host_dirty = true;
    g->state_dev_dirty = false;
    g->plan_dirty = true;
}

static bool conf_from(const float* arr, int n, AdsrConfD* c) {   // adsr.rs:94-114
    if (n == 0) { *c = AdsrConfD{0, 0, 0, 0, 0, 0, 0, 0, 0}; return true; }
    if (n == 6) { *c = AdsrConfD{0.0f, arr[0], 1.0f, arr[1], arr[2], arr[3], arr[4], arr[5], 0.0f}; return true; }
    if (n == 9) { *c = AdsrConfD{arr[0], arr[1], arr[2], arr[3], arr[4], arr[5], arr[6], arr[7], arr[8]}; return true; }
    return false;
}

int td_graph_add_sum(td_graph* g, const char* name, float gain, float angle) {
    add_vertex(g, name, gain, angle, 0.0f, K_SUM);
    return 1;
}
int td_graph_add_normalize(td_graph* g, const char* name, float gain, float angle) {
    const int slot = new_slot(g);
    Vertex& v = add_vertex(g, name, gain, angle, 0.0f, K_NORMALIZE);
    v.state_slot = slot;
    g->hstate[slot].norm = {0.0f, 0.0f, 0u, 0u};   // extensions.rs:87-92
    return 1;
}
int td_graph_add_sampleloop(td_graph* g, const char* name, float gain, float angle, size_t sample_index) {
    Vertex& v = add_vertex(g, name, gain, angle, 0.0f, K_SAMPLE_LOOP);
    v.sample_index = sample_index;
    return 1;
}
int td_graph_add_sample_multi(td_graph* g, const char* name, float gain, float angle, size_t sample_index,
                              size_t floww_index, int note) {
    Vertex& v = add_vertex(g, name, gain, angle, 0.0f, K_SAMPLE_MULTI);
    v.sample_index = sample_index;
    v.floww_index = floww_index;
    v.has_note = !(note < 0);   // state.rs:358-359
    v.note = v.has_note ? (size_t)note : 0;
    return 1;
}
int td_graph_add_sample_lerp(td_graph* g, const char* name, float gain, float angle, size_t sample_index,
                             size_t floww_index, int note, int lerp_len) {
    Vertex& v = add_vertex(g, name, gain, angle, 0.0f, K_SAMPLE_LERP);
    v.sample_index = sample_index;
    v.floww_index = floww_index;
    v.has_note = !(note < 0);   // state.rs:368-369
    v.note = v.has_note ? (size_t)note : 0;
    v.lerp_len = (size_t)std::max(lerp_len, 0);   // state.rs:370
    return 1;
}
int td_graph_add_debug_sine(td_graph* g, const char* name, float gain, float angle, size_t floww_index) {
    Vertex& v = add_vertex(g, name, gain, angle, 0.0f, K_DEBUG_SINE);
    v.exact_sin = g->sine_mode != 0;
    v.floww_index = floww_index;
    return 1;
}
int td_graph_add_synth(td_graph* g, const char* name, float gain, float angle, size_t floww_index, float square_vel,
                       float square_z, const float* square_adsr, int square_adsr_len, float topflat_vel,
                       float topflat_z, const float* topflat_adsr, int topflat_adsr_len, float triangle_vel,
                       const float* triangle_adsr, int triangle_adsr_len) {
    AdsrConfD sq, tf, tr;
    if (!conf_from(square_adsr, square_adsr_len, &sq) || !conf_from(topflat_adsr, topflat_adsr_len, &tf) ||
        !conf_from(triangle_adsr, triangle_adsr_len, &tr))
        return fail("ADSR config must have 6 or 9 elements");   // state.rs:393 panics
    Vertex& v = add_vertex(g, name, gain, angle, 0.0f, K_SYNTH);
    v.exact_sin = g->sine_mode != 0;
    v.floww_index = floww_index;
    v.square = {square_vel, fmaxf(square_z, 0.0001f), sq};   // state.rs:400
    v.topflat = {topflat_vel, topflat_z, tf};
    v.triangle = {triangle_vel, 0.0f, tr};
    return 1;
}
// Wavetable resource of add_sampsyn: this engine's own format (the reference parses with the un-vendored
// sampsyn crate, state.rs:415-422):  "TDWT" u32 version=1, u32 n_frames, u32 frame_len, f32 table_seconds,
// then n_frames*frame_len f32 little-endian.  Anything else -> the default table (one sine cycle of 2048),
// like the reference's "using default table!" arm.
static bool parse_wavetable(const uint8_t* b, size_t n, uint32_t* nf, uint32_t* fl, float* secs, std::vector<float>* data) {
    if (!b || n < 20 || memcmp(b, "TDWT", 4) != 0) return false;
    uint32_t ver;
    memcpy(&ver, b + 4, 4); memcpy(nf, b + 8, 4); memcpy(fl, b + 12, 4); memcpy(secs, b + 16, 4);
    if (ver != 1 || *nf == 0 || *fl < 2 || (uint64_t)*nf * *fl > (1u << 26) || n < 20 + (size_t)*nf * *fl * 4) return false;
    if (!(*secs > 0.0f)) return false;
    data->resize((size_t)*nf * *fl);
    memcpy(data->data(), b + 20, data->size() * 4);
    return true;
}
int td_graph_add_sampsyn(td_graph* g, const char* name, float gain, float angle, size_t floww_index, const float* adsr,
                         int adsr_len, const void* table_bytes, size_t table_len) {
    AdsrConfD c;
    if (!conf_from(adsr, adsr_len, &c)) return fail("ADSR config must have 6 or 9 elements");   // state.rs:410
    uint32_t nf = 1, fl = 2048;
    float secs = 1.0f;
    std::vector<float> data;
    if (!parse_wavetable((const uint8_t*)table_bytes, table_len, &nf, &fl, &secs, &data)) {
        nf = 1; fl = 2048; secs = 1.0f;
        data.resize(2048);
        for (int i = 0; i < 2048; ++i) data[i] = (float)sin(2.0 * 3.14159265358979323846 * (double)i / 2048.0);
    }
    if (!ensure_device(g->device)) return 0;
    // device layout: one 16-byte quad per (frame, index) holding the four samples the oscillator's two lerps read
    // (tdk::WaveTableD): one gather per voice-frame instead of four
    std::vector<float> quads(data.size() * 4);
    for (uint32_t f = 0; f < nf; ++f) {
        const uint32_t f1 = f + 1u < nf ? f + 1u : nf - 1u;
        for (uint32_t i = 0; i < fl; ++i) {
            const uint32_t i1 = i + 1u == fl ? 0u : i + 1u;
            float* q = &quads[((size_t)f * fl + i) * 4];
            q[0] = data[(size_t)f * fl + i];  q[1] = data[(size_t)f * fl + i1];
            q[2] = data[(size_t)f1 * fl + i]; q[3] = data[(size_t)f1 * fl + i1];
        }
    }
    float* d_t = nullptr;
    TD_HIP(hipMalloc(&d_t, quads.size() * sizeof(float)));
    TD_HIP(hipMemcpy(d_t, quads.data(), quads.size() * sizeof(float), hipMemcpyHostToDevice));
    g->wavetables.push_back(d_t);
    g->device_bytes += quads.size() * sizeof(float);
    Vertex& v = add_vertex(g, name, gain, angle, 0.0f, K_SAMPSYN);
    v.floww_index = floww_index;
    v.conf = c;
    v.wavetable = WaveTableD{(const float4*)d_t, nf, fl, secs, 0u};
    return 1;
}
int td_graph_add_adsr(td_graph* g, const char* name, float gain, float angle, float wet, size_t floww_index,
                      int use_off, int use_max, int note, const float* adsr, int adsr_len) {
    AdsrConfD c;
    if (!conf_from(adsr, adsr_len, &c)) return fail("ADSR config must have 6 or 9 elements");   // state.rs:444
    Vertex& v = add_vertex(g, name, gain, angle, wet, K_ADSR);
    v.floww_index = floww_index;
    v.use_off = use_off != 0;
    v.use_max = use_max != 0;
    v.has_note = !(note < 0);   // state.rs:439-440
    v.note = v.has_note ? (size_t)note : 0;
    v.conf = c;
    return 1;
}
static float band_gamma(float hz, size_t sampling_hz) {   // extensions.rs:176-183
    const float co = fmaxf(fminf(hz, 20000.0f), 0.0f);
    return 1.0f - powf(2.71828182845904523536f, -2.0f * 3.14159274101257324f * co / (float)sampling_hz);
}
int td_graph_add_bandpass(td_graph* g, const char* name, float gain, float angle, float wet, float cut_off_hz_low,
                          float cut_off_hz_high, int pass) {
    const int slot = new_slot(g);
    Vertex& v = add_vertex(g, name, gain, angle, wet, K_BAND_PASS);
    v.lgamma = band_gamma(cut_off_hz_low, g->sr);
    v.hgamma = band_gamma(cut_off_hz_high, g->sr);
    v.pass = pass != 0;
    v.state_slot = slot;
    g->hstate[slot].band = {0.f, 0.f, 0.f, 0.f, 1u, {0, 0, 0}};
    return 1;
}
// This engine's own effect vertices (no reference counterpart; the definitions are in include/termdaw_amd.h): each packs its
// arguments into its kind's block (fx_params.h) for add_fx; the td_<kind>_params beside them judge theirs by the same check.  The
// state a kind carries beyond its slots is a line (Vertex::line; the convolution's response spectra beside it), allocated when the
// vertex is first compiled into a submission.
int td_graph_add_compressor(td_graph* g, const char* name, float gain, float angle, float wet, float threshold_db, float ratio,
                            float attack_ms, float release_ms, float knee_db, float makeup_db) {
    FxParams p{};
    p.comp = {threshold_db, ratio, attack_ms, release_ms, knee_db, makeup_db};
    return add_fx(g, K_COMPRESSOR, name, gain, angle, wet, p);
}

int td_graph_add_eq(td_graph* g, const char* name, float gain, float angle, float wet, int kind, float freq_hz, float q, float gain_db) {
    FxParams p{};
    p.eq = {kind, freq_hz, q, gain_db};
    return add_fx(g, K_EQ, name, gain, angle, wet, p);
}
int td_eq_coefficients(int kind, size_t sr, float freq_hz, float q, float gain_db, double out[6]) {
    if (!out) return fail("eq_coefficients: out is null");
    FxParams p{};
    p.eq = {kind, freq_hz, q, gain_db};
    if (!fx_check(K_EQ, sr, p)) return 0;
    eq::coefficients(kind, sr, freq_hz, q, gain_db, out);
    out[5] = eq::hmax(out);
    return 1;
}

int td_graph_add_delay(td_graph* g, const char* name, float gain, float angle, float wet, float time_ms, float feedback, float cross) {
    FxParams p{};
    p.delay = {time_ms, feedback, cross};
    return add_fx(g, K_DELAY, name, gain, angle, wet, p);
}
int td_delay_params(size_t sr, float time_ms, float feedback, float cross, double out[4]) {
    if (!out) return fail("delay_params: out is null");
    FxParams p{};
    p.delay = {time_ms, feedback, cross};
    if (!fx_check(K_DELAY, sr, p)) return 0;
    delay::params(sr, time_ms, feedback, cross, out);
    return 1;
}

int td_graph_add_saturator(td_graph* g, const char* name, float gain, float angle, float wet, int kind, float drive_db, float bias,
                           float out_db, int oversample) {
    FxParams p{};
    p.sat = {kind, drive_db, bias, out_db, oversample};
    return add_fx(g, K_SATURATOR, name, gain, angle, wet, p);
}
int td_saturator_taps(int oversample, double* taps, size_t cap) {
    if (!sat::oversample_ok(oversample)) return fail("saturator_taps: oversample must be 1, 2, 4 or 8");
    const std::vector<double>& h = sat::taps(oversample);
    if (taps)
        for (size_t i = 0; i < h.size() && i < cap; ++i) taps[i] = h[i];
    return (int)h.size();
}
int td_saturator_params(int kind, int oversample, float drive_db, float bias, float out_db, double out[6]) {
    if (!out) return fail("saturator_params: out is null");
    FxParams p{};
    p.sat = {kind, drive_db, bias, out_db, oversample};
    if (!fx_check(K_SATURATOR, 0, p)) return 0;   // (no range of it depends on the rate)
    sat::params(kind, oversample, drive_db, bias, out_db, out);
    return 1;
}

int td_graph_add_chorus(td_graph* g, const char* name, float gain, float angle, float wet, int voices, float delay_ms, float depth_ms,
                        float rate_hz, float stereo, int shape) {
    FxParams p{};
    p.chorus = {voices, delay_ms, depth_ms, rate_hz, stereo, shape};
    return add_fx(g, K_CHORUS, name, gain, angle, wet, p);
}
int td_chorus_params(size_t sr, int voices, float delay_ms, float depth_ms, float rate_hz, float stereo, int shape, double out[6]) {
    if (!out) return fail("chorus_params: out is null");
    FxParams p{};
    p.chorus = {voices, delay_ms, depth_ms, rate_hz, stereo, shape};
    if (!fx_check(K_CHORUS, sr, p)) return 0;
    chorus::params(sr, voices, delay_ms, depth_ms, rate_hz, stereo, shape, out);
    return 1;
}

int td_graph_add_reverb(td_graph* g, const char* name, float gain, float angle, float wet, float room, float damp, float width, float size) {
    FxParams p{};
    p.reverb = {room, damp, width, size};
    return add_fx(g, K_REVERB, name, gain, angle, wet, p);
}
int td_reverb_params(size_t sr, float room, float damp, float width, float size, double out[31]) {
    if (!out) return fail("reverb_params: out is null");
    FxParams p{};
    p.reverb = {room, damp, width, size};
    if (!fx_check(K_REVERB, sr, p)) return 0;
    reverb::params(sr, room, damp, width, size, out);
    return 1;
}

int td_graph_add_gate(td_graph* g, const char* name, float gain, float angle, float wet, float threshold_db, float hysteresis_db,
                      float hold_ms, float attack_ms, float release_ms, float range_db) {
    FxParams p{};
    p.gate = {threshold_db, hysteresis_db, hold_ms, attack_ms, release_ms, range_db};
    return add_fx(g, K_GATE, name, gain, angle, wet, p);
}
int td_gate_params(size_t sr, float threshold_db, float hysteresis_db, float hold_ms, float attack_ms, float release_ms, float range_db,
                   double out[6]) {
    if (!out) return fail("gate_params: out is null");
    FxParams p{};
    p.gate = {threshold_db, hysteresis_db, hold_ms, attack_ms, release_ms, range_db};
    if (!fx_check(K_GATE, sr, p)) return 0;
    gate::params(sr, threshold_db, hysteresis_db, hold_ms, attack_ms, release_ms, range_db, out);
    return 1;
}

int td_graph_add_phaser(td_graph* g, const char* name, float gain, float angle, float wet, int stages, float lo_hz, float hi_hz,
                        float rate_hz, float feedback, float stereo, int shape) {
    FxParams p{};
    p.phaser = {stages, lo_hz, hi_hz, rate_hz, feedback, stereo, shape};
    return add_fx(g, K_PHASER, name, gain, angle, wet, p);
}
int td_phaser_params(size_t sr, int stages, float lo_hz, float hi_hz, float rate_hz, float feedback, float stereo, int shape, double out[7]) {
    if (!out) return fail("phaser_params: out is null");
    FxParams p{};
    p.phaser = {stages, lo_hz, hi_hz, rate_hz, feedback, stereo, shape};
    if (!fx_check(K_PHASER, sr, p)) return 0;
    phaser::params(sr, stages, lo_hz, hi_hz, rate_hz, feedback, stereo, shape, out);
    return 1;
}

int td_graph_add_vocoder(td_graph* g, const char* name, float gain, float angle, float wet, int bands, float lo_hz, float hi_hz, float q,
                         float response_ms, float out_db) {
    FxParams p{};
    p.vocoder = {bands, lo_hz, hi_hz, q, response_ms, out_db};
    return add_fx(g, K_VOCODER, name, gain, angle, wet, p);
}
int td_vocoder_params(size_t sr, int bands, float lo_hz, float hi_hz, float q, float response_ms, float out_db, double* out, size_t cap) {
    if (!out) return fail("vocoder_params: out is null");
    FxParams p{};
    p.vocoder = {bands, lo_hz, hi_hz, q, response_ms, out_db};
    if (!fx_check(K_VOCODER, sr, p)) return 0;
    if (cap < vocoder::n_params(bands)) return fail("vocoder_params: out holds fewer than 6 bands + 2 doubles");
    vocoder::params(sr, bands, lo_hz, hi_hz, q, response_ms, out_db, out);
    return 1;
}

int td_graph_add_filter(td_graph* g, const char* name, float gain, float angle, float wet, int kind, float freq_hz, float q,
                        float lfo_oct, float rate_hz, float stereo, int shape, float env_oct, float sens_db, float attack_ms, float release_ms) {
    FxParams p{};
    p.filter = {kind, freq_hz, q, lfo_oct, rate_hz, stereo, shape, env_oct, sens_db, attack_ms, release_ms};
    return add_fx(g, K_FILTER, name, gain, angle, wet, p);
}
int td_filter_params(size_t sr, int kind, float freq_hz, float q, float lfo_oct, float rate_hz, float stereo, int shape, float env_oct,
                     float sens_db, float attack_ms, float release_ms, double* out, size_t cap) {
    if (!out) return fail("filter_params: out is null");
    FxParams p{};
    p.filter = {kind, freq_hz, q, lfo_oct, rate_hz, stereo, shape, env_oct, sens_db, attack_ms, release_ms};
    if (!fx_check(K_FILTER, sr, p)) return 0;
    if (cap < (size_t)filter::kParams) return fail("filter_params: out holds fewer than 11 doubles");
    filter::params(sr, kind, freq_hz, q, lfo_oct, rate_hz, stereo, shape, env_oct, sens_db, attack_ms, release_ms, out);
    return 1;
}

int td_graph_add_limiter(td_graph* g, const char* name, float gain, float angle, float wet, float ceiling_db, float lookahead_ms,
                         float release_ms, float drive_db) {
    FxParams p{};
    p.limiter = {ceiling_db, lookahead_ms, release_ms, drive_db};
    return add_fx(g, K_LIMITER, name, gain, angle, wet, p);
}
int td_limiter_params(size_t sr, float ceiling_db, float lookahead_ms, float release_ms, float drive_db, double out[5]) {
    if (!out) return fail("limiter_params: out is null");
    FxParams p{};
    p.limiter = {ceiling_db, lookahead_ms, release_ms, drive_db};
    if (!fx_check(K_LIMITER, sr, p)) return 0;
    limiter::params(sr, ceiling_db, lookahead_ms, release_ms, drive_db, out);
    return 1;
}

// (nullptr: the per-band pointers do not each point at three floats, g_error says so)
static const MbParams* mb_block(MbParams* p, float lo_hz, float hi_hz, const float threshold_db[3], const float ratio[3], float attack_ms,
                                float release_ms, float knee_db, const float makeup_db[3]) {
    if (!threshold_db || !ratio || !makeup_db) {
        fail("multiband: threshold_db, ratio and makeup_db must point at three floats each");
        return nullptr;
    }
    *p = MbParams{lo_hz, hi_hz, {threshold_db[0], threshold_db[1], threshold_db[2]}, {ratio[0], ratio[1], ratio[2]}, attack_ms, release_ms, knee_db,
                  {makeup_db[0], makeup_db[1], makeup_db[2]}};
    return p;
}
int td_graph_add_multiband(td_graph* g, const char* name, float gain, float angle, float wet, float lo_hz, float hi_hz,
                           const float threshold_db[3], const float ratio[3], float attack_ms, float release_ms, float knee_db,
                           const float makeup_db[3]) {
    FxParams p{};
    if (!mb_block(&p.mb, lo_hz, hi_hz, threshold_db, ratio, attack_ms, release_ms, knee_db, makeup_db)) return 0;
    return add_fx(g, K_MULTIBAND, name, gain, angle, wet, p);
}
int td_multiband_params(size_t sr, float lo_hz, float hi_hz, const float threshold_db[3], const float ratio[3], float attack_ms,
                        float release_ms, float knee_db, const float makeup_db[3], double* out, size_t n) {
    if (!out) return fail("multiband_params: out is null");
    FxParams p{};
    if (!mb_block(&p.mb, lo_hz, hi_hz, threshold_db, ratio, attack_ms, release_ms, knee_db, makeup_db) || !fx_check(K_MULTIBAND, sr, p)) return 0;
    if (n < (size_t)multiband::kParams) return fail("multiband_params: out holds fewer than 27 doubles");
    multiband::params(sr, lo_hz, hi_hz, attack_ms, release_ms, out);
    return 1;
}

// (the response is the bank's sample, which only a render brings: its length is judged there, and where the bank is at hand)
int td_graph_add_convolution(td_graph* g, const char* name, float gain, float angle, float wet, size_t sample_index, float length_ms,
                             float predelay_ms, float out_db, int norm) {
    FxParams p{};
    p.conv = {length_ms, predelay_ms, out_db, norm};
    return add_fx(g, K_CONVOLUTION, name, gain, angle, wet, p, sample_index);
}
int td_convolution_params(size_t sr, size_t sample_len, float length_ms, float predelay_ms, float out_db, int norm, double out[6]) {
    if (!out) return fail("convolution_params: out is null");
    FxParams p{};
    p.conv = {length_ms, predelay_ms, out_db, norm};
    if (!fx_check(K_CONVOLUTION, sr, p)) return 0;
    if (const char* why = conv::check_len(sr, sample_len, length_ms)) return fail(std::string("convolution: ") + why);
    conv::params(sr, sample_len, length_ms, predelay_ms, out_db, out);
    return 1;
}
size_t td_convolution_twiddles(double* out, size_t cap) {
    if (out && cap >= (size_t)conv::kN) conv::twiddles(out);
    return (size_t)conv::kN;
}

static bool has_loop(size_t x, size_t b, const td_graph* g) {   // graph.rs:66-72
    if (x == b) return true;
    for (size_t y : g->edges[x])
        if (has_loop(y, b, g)) return true;
    for (size_t y : g->key_edges[x])
        if (has_loop(y, b, g)) return true;
    return false;
}
int td_graph_connect(td_graph* g, const char* a, const char* b) {   // graph.rs:58-96
    settle_guard_before_edit(g);
    auto ia = g->name_map.find(a), ib = g->name_map.find(b);
    if (ia == g->name_map.end()) return fail(std::string("TermDaw: warning: vertex \"") + a + "\" cannot be found and thus can't be connected.");
    if (ib == g->name_map.end()) return fail(std::string("TermDaw: warning: vertex \"") + b + "\" cannot be found and thus can't be connected to.");
    const size_t ai = ia->second, bi = ib->second;
    if (ai == bi) return fail("connect: self edge");
    if (!g->vertices[bi].has_input()) return fail("connect: target vertex takes no input");
    if (has_loop(ai, bi, g)) return fail("connect: edge would close a loop");
    g->edges[bi].push_back(ai);
    g->plan_dirty = true;
    return 1;
}
int td_graph_connect_key(td_graph* g, const char* a, const char* b) {
    settle_guard_before_edit(g);
    auto ia = g->name_map.find(a), ib = g->name_map.find(b);
    if (ia == g->name_map.end()) return fail(std::string("TermDaw: warning: vertex \"") + a + "\" cannot be found and thus can't be connected.");
    if (ib == g->name_map.end()) return fail(std::string("TermDaw: warning: vertex \"") + b + "\" cannot be found and thus can't be connected to.");
    const size_t ai = ia->second, bi = ib->second;
    const FxKind* fx = fx_kind(g->vertices[bi].kind);
    if (!(fx && fx->takes_key)) return fail(std::string("connect_key: ") + b + " takes no key input");
    if (ai == bi) return fail("connect_key: self edge");
    if (has_loop(ai, bi, g)) return fail("connect_key: edge would close a loop");
    g->key_edges[bi].push_back(ai);
    g->plan_dirty = true;
    return 1;
}
int td_graph_set_output(td_graph* g, const char* vertex) {
    auto it = g->name_map.find(vertex);
    if (it == g->name_map.end()) return fail("set_output: vertex not found");
    settle_guard_before_edit(g);
    g->output_vertex = (long)it->second;
    g->plan_dirty = true;
    return 1;
}
int td_graph_check(const td_graph* g) {   // graph.rs:150-174
    if (g->output_vertex < 0) return fail("TermDaw: error: output vertex not found.");
    const size_t out = (size_t)g->output_vertex;
    if (g->edges[out].empty() && g->vertices[out].has_input()) return fail("TermDaw: error: output receives no inputs.");
    return 1;
}
void td_graph_set_time(td_graph* g, size_t time) { graph_set_time_impl(g, time); }
size_t td_graph_change_time(td_graph* g, size_t delta, int plus) {   // graph.rs:130-135
    const size_t nt = plus ? g->t + delta : g->t - std::min(delta, g->t);
    graph_set_time_impl(g, nt);
    return nt;
}
size_t td_graph_get_time(const td_graph* g) { return g->t; }
void td_graph_reset_normalize_vertices(td_graph* g) {   // extensions.rs:295-299
    // No device traffic: the value is handed to the next render as the initial max (SumDesc::init_max).
    for (auto& vx : g->vertices) {
        if (vx.kind != K_NORMALIZE) continue;
        vx.has_init_override = true;
        vx.init_override = 0.000001f;
        vx.peak_known = false;
    }
}
float td_graph_get_normalization_value(const td_graph* gc, const char* name) {
    td_graph* g = const_cast<td_graph*>(gc);
    auto it = g->name_map.find(name);
    if (it == g->name_map.end()) return -1.0f;
    const Vertex& v = g->vertices[it->second];
    if (v.kind != K_NORMALIZE) return -1.0f;
    if (v.has_init_override) return v.init_override;
    pull_state(g);
    return g->hstate[v.state_slot].norm.max;
}
size_t td_graph_vertex_count(const td_graph* g) { return g->vertices.size(); }

int td_graph_render_block(td_graph* g, const td_samplebank* sb, td_flowwbank* fb, float* l, float* r) {
    if (g->output_vertex < 0) return 0;   // None
    // Graph::render leaves the FlowwBank alone: run one block on a cursor snapshot
    const size_t frame = fb->frame;
    const std::vector<size_t> starts = fb->start_indices;
    // (block pulls ignore the stems: the plan of the output alone, as the reference's Graph::render walks it)
    struct Unstem {
        td_graph* g;
        std::vector<size_t> kept;
        explicit Unstem(td_graph* x) : g(x) { if (!g->stems.empty()) { settle_guard_before_edit(g); kept.swap(g->stems); g->plan_dirty = true; } }
        ~Unstem() { if (!kept.empty()) { (void)drain(g); kept.swap(g->stems); g->plan_dirty = true; } }
    } unstem(g);
    const int ok = graph_render_chunks(g, sb, fb, 1, false, 16, true, 0, false);
    fb->frame = frame;
    fb->start_indices = starts;
    if (!ok) return -1;
    std::vector<float2> tmp(g->bl);
    if (!drain(g)) return -1;
    if (hipMemcpyAsync(tmp.data(), g->last_out_f32, g->bl * sizeof(float2), hipMemcpyDeviceToHost, g->stream) != hipSuccess ||
        hipStreamSynchronize(g->stream) != hipSuccess) {
        fail("HIP error: block read-back failed");
        return -1;
    }
    for (size_t i = 0; i < g->bl; ++i) {
        if (l) l[i] = tmp[i].x;
        if (r) r[i] = tmp[i].y;
    }
    return 1;
}

// Graph::true_normalize_scan (graph.rs:222-237) around the dry run itself
static int scan_begin(td_graph* g, td_flowwbank* fb) {
    if (!ensure_graph_device(g)) return 0;
    if (g->plan_dirty) build_plan(g);
    if (!ensure_state_slots(g)) return 0;
    for (auto& v : g->vertices)   // reset_scan_normalization
        if (v.kind == K_NORMALIZE)
            TD_HIP(hipMemsetD32Async((hipDeviceptr_t)&g->dstate[v.state_slot].norm.scan_max, 0, 1, g->stream));
    fb->set_time(0);
    return 1;
}
static int scan_end(td_graph* g, td_flowwbank* fb) {
    for (auto& v : g->vertices)   // apply_scan_normalization: max = scan_max (every Normalize vertex, reached or not)
        if (v.kind == K_NORMALIZE) {
            v.has_init_override = false;
            v.peak_known = true;
            TD_HIP(hipMemcpyAsync(&g->dstate[v.state_slot].norm.max, &g->dstate[v.state_slot].norm.scan_max, 4,
                                  hipMemcpyDeviceToDevice, g->stream));
        }
    g->state_dev_dirty = true;
    if (!graph_set_time_impl(g, 0)) return 0;
    fb->set_time(0);
    return 1;
}
int td_graph_normalize_scan(td_graph* g, const td_samplebank* sb, td_flowwbank* fb, size_t chunks) {   // graph.rs:222-237
    if (g->output_vertex < 0) return 1;
    if (!scan_begin(g, fb)) return 0;
    if (!graph_render_chunks(g, sb, fb, chunks, true, 16, false, 0, false)) return 0;
    if (g->guard.armed && !drain(g)) return 0;   // (band_mode 2: a dry run over the bound is done again BEFORE its peaks are applied)
    if (!scan_end(g, fb)) return 0;
    return drain(g);
}

size_t td_graph_render_all_async(td_graph* g, const td_samplebank* sb, td_flowwbank* fb, size_t n_blocks, int bits) {
    if (!graph_render_chunks(g, sb, fb, n_blocks, false, bits, true, 0, true)) return 0;
    if (!graph_set_time_impl(g, 0)) return 0;   // state.rs:575
    return n_blocks * g->bl;
}
int td_graph_sync(td_graph* g) { return drain(g); }
size_t td_graph_norm_respec(td_graph* g) {
    if (!g->stream || !drain(g)) return 0;
    size_t n = 0;
    for (Arena* ar : {&g->arena, g->batch ? &g->batch->arena : (Arena*)nullptr}) {
        if (!ar || !ar->d_respec) continue;
        uint32_t v = 0;
        if (hipMemcpy(&v, ar->d_respec, 4, hipMemcpyDeviceToHost) != hipSuccess || hipMemset(ar->d_respec, 0, 4) != hipSuccess) return 0;
        n += v;
    }
    return n;
}
size_t td_graph_norm_fix_runs(const td_graph* g) { return g->arena.fix_runs + (g->batch ? g->batch->arena.fix_runs : 0); }
size_t td_graph_render_all(td_graph* g, const td_samplebank* sb, td_flowwbank* fb, size_t n_blocks, int bits) {
    const size_t n = td_graph_render_all_async(g, sb, fb, n_blocks, bits);
    if (!n) return 0;
    if (!td_graph_sync(g)) return 0;
    return n;
}
// The stems of a resampled render: every stem's whole-timeline f32 frames (d_stem_f32, written by the render's k_stems
// launches) through the same resampler as the output's, then ONE k_stems launch quantises all of them -- and takes their
// peaks over the resampled frames.  Not the hot path: a stream synchronisation per stem.
static int resample_stems(td_graph* g, size_t total, size_t psr, size_t render_sr, size_t nout, float amplitude, int qmode) {
    const size_t n = g->stems.size(), word = qmode == 1 ? 2 : 4;
    if (!prepare_stems(g, nout, word)) return 0;
    std::vector<float2*> rs(n, nullptr);
    std::vector<StemDesc> d(n);
    StemDesc* dd = nullptr;
    int ok = 1;
    for (size_t k = 0; k < n && ok; ++k) {
        size_t nk = 0;
        ok = resample_device(g->d_stem_f32 + k * g->stem_f32_stride, total, psr, render_sr, &rs[k], &nk, g->stream);
        if (ok && nk != nout) ok = fail("termdaw_amd: internal: a stem resampled to another length than the output");
        d[k] = StemDesc{};
        d[k].src.p = rs[k];
        d[k].pcm = g->d_stem_pcm + k * g->stem_stride;
        d[k].peak = g->d_stem_peak + k;
        d[k].amplitude = amplitude;
        d[k].qmode = (uint32_t)qmode;
    }
    if (ok && hipMalloc(&dd, n * sizeof(StemDesc)) != hipSuccess) ok = fail("termdaw_amd: out of device memory for the stem descriptors");
    if (ok && (hipMemsetAsync(g->d_stem_peak, 0, n * 4, g->stream) != hipSuccess ||
               hipMemcpyAsync(dd, d.data(), n * sizeof(StemDesc), hipMemcpyHostToDevice, g->stream) != hipSuccess))
        ok = fail("HIP error: stem descriptors");
    if (ok) launch_stems(dd, (int)n, (uint32_t)nout, g->stream);
    if (hipStreamSynchronize(g->stream) != hipSuccess && ok) ok = fail("HIP error: the stems' quantise");
    for (float2* p : rs) if (p) (void)hipFree(p);
    if (dd) (void)hipFree(dd);
    g->stems_rendered = ok ? n : 0;
    return ok;
}
// State::render's `psr > render_sr` arm (state.rs:533-561): render, then resample the whole timeline with
// the build-defined resampler (the reference streams rubato block by block -- parity unpinned), quantise.
size_t td_graph_render_all_resampled(td_graph* g, const td_samplebank* sb, td_flowwbank* fb, size_t n_blocks, int bits,
                                     size_t psr, size_t render_sr) {
    if (!(bits == 8 || bits == 16 || bits == 24 || bits == 32)) {
        fail("Bitdepth not supported: choose bitdepth in {8, 16, 24, 32}.");
        return 0;
    }
    g->loud_frames = 0;
    g->master_kept = false;
    g->stem_f32_wanted = !g->stems.empty();   // (the stems' whole-timeline frames are resampled like the output's)
    int rendered = graph_render_chunks(g, sb, fb, n_blocks, false, bits, true, 0, false);
    rendered = rendered && graph_set_time_impl(g, 0) && drain(g);   // (the resampler reads the output vertex' frames)
    g->stem_f32_wanted = false;
    if (!rendered) return 0;
    const size_t total = n_blocks * g->bl;
    float2* rs = nullptr;
    size_t nout = 0;
    if (!resample_device(g->last_out_f32, total, psr, render_sr, &rs, &nout, g->stream)) return 0;
    if (g->d_resampled) (void)hipFree(g->d_resampled);
    g->d_resampled = rs;
    const int qmode = bits > 16 ? 2 : 1;
    const size_t word = qmode == 1 ? 2 : 4;
    const float amplitude = bits < 32 ? (float)((1 << (bits - 1)) - 1) : (float)INT32_MAX;
    const size_t need = nout * 2 * word + 64;
    if (need > g->pcm_cap) {
        if (hipStreamSynchronize(g->stream) != hipSuccess) return 0;
        if (g->d_pcm && !g->pcm_borrowed) { (void)hipFree(g->d_pcm); g->device_bytes -= g->pcm_cap; }
        g->d_pcm = nullptr;
        g->pcm_cap = 0;
        g->pcm_borrowed = false;
        if (hipMalloc(&g->d_pcm, need) != hipSuccess) { fail("out of device memory"); return 0; }
        g->pcm_cap = need;
        g->device_bytes += need;
    }
    QuantDesc qd{rs, g->d_pcm, amplitude, (uint32_t)qmode};
    if (hipMemcpyAsync(g->d_scalar + 8, &qd, sizeof qd, hipMemcpyHostToDevice, g->stream) != hipSuccess) return 0;
    if (hipStreamSynchronize(g->stream) != hipSuccess) return 0;   // qd lives on this stack frame
    launch_quantise((const QuantDesc*)(g->d_scalar + 8), 1, (uint32_t)nout, g->stream);
    if (hipStreamSynchronize(g->stream) != hipSuccess) return 0;
    g->pcm_bytes = nout * 2 * word;
    g->last_out_f32 = rs;
    g->last_frames = nout;
    g->last_bits = bits;
    if (!g->stems.empty() && !resample_stems(g, total, psr, render_sr, nout, amplitude, qmode)) return 0;
    g->loud_frames = nout;
    g->loud_bits = bits;
    g->loud_sr = render_sr;
    return nout;
}
const void* td_graph_output_pcm_device(const td_graph* g) { return g->d_pcm; }

// ---- stems (include/termdaw_amd.h; the semantics of set_output, graph.rs:141-148, for every named vertex) ----
int td_graph_set_stems(td_graph* g, const char* const* names, size_t n) {
    std::vector<size_t> v;
    for (size_t i = 0; i < n; ++i) {
        auto it = names && names[i] ? g->name_map.find(names[i]) : g->name_map.end();
        if (it == g->name_map.end()) return fail(std::string("set_stems: vertex not found: ") + (names && names[i] ? names[i] : "(null)"));
        if (std::find(v.begin(), v.end(), it->second) != v.end()) return fail(std::string("set_stems: vertex named twice: ") + names[i]);
        v.push_back(it->second);
    }
    settle_guard_before_edit(g);
    g->stems = v;
    g->stems_rendered = 0;
    g->stem_taps = 0;
    g->plan_dirty = true;
    return 1;
}
size_t td_graph_stem_count(const td_graph* g) { return g->stems.size(); }
const void* td_graph_stem_pcm_device(const td_graph* g, size_t i) {
    if (i >= g->stems_rendered || !g->d_stem_pcm) return nullptr;
    return g->d_stem_pcm + i * g->stem_stride;
}
int td_graph_read_stem_pcm(const td_graph* g, size_t i, void* out, size_t bytes) {
    if (i >= g->stems_rendered || !g->d_stem_pcm || bytes > g->stem_pcm_bytes) return fail("read_stem_pcm: no such stem rendered / size too large");
    if (!drain(const_cast<td_graph*>(g))) return 0;
    TD_HIP(hipMemcpy(out, g->d_stem_pcm + i * g->stem_stride, bytes, hipMemcpyDeviceToHost));
    return 1;
}
float td_graph_stem_peak(const td_graph* gc, size_t i) {
    td_graph* g = const_cast<td_graph*>(gc);
    if (i >= g->stems_rendered || !g->d_stem_peak) { fail("stem_peak: no such stem rendered"); return 0.0f; }
    if (!drain(g)) return 0.0f;
    uint32_t bits = 0;
    if (hipMemcpy(&bits, g->d_stem_peak + i, 4, hipMemcpyDeviceToHost) != hipSuccess) { fail("HIP error: stem peak read-back"); return 0.0f; }
    float v;
    memcpy(&v, &bits, 4);
    return v;
}
// ---- loudness (include/termdaw_amd.h td_graph_loudness): ONE k_loudness launch over every signal asked for,
// the hop energies and peak words back, the figures in double on the host ----
static int measure_loudness(hipStream_t stream, uint8_t** d_work, size_t* cap, ProfCtx* prof, const std::vector<loud::Signal>& sig,
                            double* out, std::vector<std::vector<double>>* mom) {
    if (!launch_loudness) return fail("termdaw_amd: this build has no k_loudness kernel: loudness cannot be measured");
    const size_t n = sig.size();
    std::vector<LoudDesc> d(n);
    std::vector<size_t> e_off(n);
    size_t hops_total = 0;
    uint32_t max_tiles = 0;
    for (size_t i = 0; i < n; ++i) {
        const char* why = "";
        if (!loud::describe(sig[i], d[i], &why)) return fail(why);
        e_off[i] = hops_total;
        hops_total += loud::hops(d[i]);
        max_tiles = std::max(max_tiles, d[i].n_tiles);
    }
    const size_t desc_b = n * sizeof(LoudDesc), peak_b = (n * 8 + 7) & ~(size_t)7, need = desc_b + peak_b + hops_total * 16;
    if (need > *cap) {
        TD_HIP(hipStreamSynchronize(stream));
        if (*d_work) (void)hipFree(*d_work);
        *d_work = nullptr;
        *cap = 0;
        TD_HIP(hipMalloc(d_work, need));
        *cap = need;
    }
    uint32_t* d_peak = (uint32_t*)(*d_work + desc_b);
    double* d_energy = (double*)(*d_work + desc_b + peak_b);
    for (size_t i = 0; i < n; ++i) {
        d[i].pcm = sig[i].pcm;
        d[i].peak = d_peak + 2 * i;
        d[i].energy = d_energy + 2 * e_off[i];
    }
    TD_HIP(hipMemcpyAsync(*d_work, d.data(), desc_b, hipMemcpyHostToDevice, stream));
    TD_HIP(hipMemsetAsync(d_peak, 0, peak_b, stream));
    {
        ProfCtx none;
        ProfCtx& pc = prof ? *prof : none;
        pc.now = pc.every != 0;   // (every measurement is timed while profiling is on)
        Prof pr(pc, F_LOUD, stream);
        launch_loudness((const LoudDesc*)*d_work, (int)n, max_tiles, stream);
    }
    TD_HIP(hipGetLastError());
    std::vector<uint8_t> back(peak_b + hops_total * 16);
    TD_HIP(hipMemcpyAsync(back.data(), d_peak, back.size(), hipMemcpyDeviceToHost, stream));
    TD_HIP(hipStreamSynchronize(stream));
    const uint32_t* peak = (const uint32_t*)back.data();
    const double* energy = (const double*)(back.data() + peak_b);
    if (mom) mom->assign(n, {});
    std::vector<double> scratch;
    for (size_t i = 0; i < n; ++i)
        loud::figures(energy + 2 * e_off[i], loud::hops(d[i]), d[i].hop, peak + 2 * i, sig[i].frames, sig[i].sr, out + 8 * i,
                      mom ? &(*mom)[i] : &scratch);
    return 1;
}
// The output (0) or stem i - 1 of the last whole render, as a WAV reader would see it
static loud::Signal render_signal(const td_graph* g, size_t which) {
    loud::Signal s;
    s.pcm = which ? (const void*)(g->d_stem_pcm + (which - 1) * g->stem_stride) : (const void*)g->d_pcm;
    s.kind = g->loud_bits > 16 ? 1u : 0u;
    s.scale = loud::word_scale(g->loud_bits);
    s.frames = g->loud_frames;
    s.sr = g->loud_sr;
    return s;
}
int td_graph_loudness(td_graph* g, double* out, size_t n) {
    if (!g->loud_frames || !g->d_pcm) return fail("loudness: no whole render to measure (td_graph_render_all / _async / _resampled)");
    if (n > 1 + g->stems_rendered)
        return fail("loudness: " + std::to_string(n) + " signals asked for, the last render has the output and " +
                    std::to_string(g->stems_rendered) + " stems");
    if (!drain(g)) return 0;   // (the deferred Normalize check and a guarded verdict settle first: the final bytes are measured)
    if (!g->loud_frames || !g->d_pcm) return fail("loudness: no whole render to measure");
    if (!n) return 1;
    std::vector<loud::Signal> sig;
    for (size_t i = 0; i < n; ++i) sig.push_back(render_signal(g, i));
    return measure_loudness(g->stream, &g->d_loud, &g->loud_cap, &g->prof, sig, out, &g->momentary);
}
size_t td_graph_momentary(const td_graph* g, size_t which, double* out, size_t cap) {
    if (which >= g->momentary.size()) { fail("momentary: no such signal in the last td_graph_loudness"); return 0; }
    const std::vector<double>& m = g->momentary[which];
    if (out) std::copy(m.begin(), m.begin() + (long)std::min(cap, m.size()), out);
    return m.size();
}
int td_batch_loudness(td_batch* b, double* out) {
    if (b->graphs.empty()) return 1;
    for (size_t i = 0; i < b->graphs.size(); ++i)
        if (!b->graphs[i]->loud_frames || !b->graphs[i]->d_pcm)
            return fail("loudness: project " + std::to_string(i) + " has no whole render to measure");
    if (!ensure_device(b->device)) return 0;
    for (td_graph* g : b->graphs)
        if (!drain(g)) return 0;
    std::vector<loud::Signal> sig;
    for (td_graph* g : b->graphs) sig.push_back(render_signal(g, 0));
    hipStream_t st = b->stream ? b->stream : b->graphs[0]->stream;
    return measure_loudness(st, &b->d_loud, &b->loud_cap, &b->prof, sig, out, nullptr);
}
int td_loudness_f32(const float* lr, size_t frames, size_t sr, double out[8]) {
    if (!ensure_device(cur_device())) return 0;
    if (frames && !lr) return fail("loudness_f32: null frames");
    loud::Signal s;
    s.kind = 2;
    s.frames = frames;
    s.sr = sr;
    void* d_in = nullptr;
    uint8_t* d_work = nullptr;
    size_t cap = 0;
    int ok = hipMalloc(&d_in, frames * 8 + 8) == hipSuccess ? 1 : fail("loudness_f32: out of device memory");
    if (ok && frames && hipMemcpy(d_in, lr, frames * 8, hipMemcpyHostToDevice) != hipSuccess) ok = fail("HIP error: loudness_f32 upload");
    s.pcm = d_in;
    if (ok) ok = measure_loudness(nullptr, &d_work, &cap, nullptr, {s}, out, nullptr);
    if (d_work) (void)hipFree(d_work);
    if (d_in) (void)hipFree(d_in);
    return ok;
}
int td_loudness_filters(size_t sr, double kw[10], float* fir, size_t cap, size_t* phases, size_t* taps) {
    if (!sr) return fail("loudness_filters: the sample rate must be positive");
    if (kw) loud::kweight((double)sr, kw);
    const size_t P = loud::phases(sr);
    if (phases) *phases = P;
    if (taps) *taps = kLoudTaps;
    if (fir) {
        if (cap < P * kLoudTaps) return fail("loudness_filters: the FIR needs " + std::to_string(P * kLoudTaps) + " floats");
        float f[4][kLoudTaps];
        loud::fir(sr, f);
        memcpy(fir, f, P * kLoudTaps * sizeof(float));
    }
    return 1;
}
// ---- mastering (include/termdaw_amd.h td_graph_master): k_master_detect once, then per pass k_master_scan,
// k_master_carry, k_master_apply and ONE k_loudness launch over the signals still running; the decisions in double on the host ----
static int grow_device(hipStream_t stream, uint8_t** d, size_t* cap, size_t need) {
    if (need <= *cap) return 1;
    TD_HIP(hipStreamSynchronize(stream));
    if (*d) (void)hipFree(*d);
    *d = nullptr;
    *cap = 0;
    TD_HIP(hipMalloc(d, need));
    *cap = need;
    return 1;
}
static size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }
static loud::Signal meter_view(const void* pcm, const mst::Signal& s) {
    loud::Signal m;
    m.pcm = pcm;
    m.kind = s.kind;
    m.scale = s.kind == 2u ? 1.0 : loud::word_scale(s.bits);
    m.frames = s.frames;
    m.sr = s.sr;
    return m;
}
static int have_master_kernels() {
    if (!launch_master_detect || !launch_master_scan || !launch_master_carry || !launch_master_apply)
        return fail("termdaw_amd: this build has no k_master kernels: mastering is not available");
    return 1;
}
// Every dst back to its src (best effort: an error already set stays the call's error); 0 when a copy failed.
static int restore_words(const std::vector<mst::Signal>& sig, hipStream_t stream) {
    bool ok = true;
    for (const mst::Signal& s : sig) {
        const size_t bytes = s.frames * (s.kind == 0u ? 4 : 8);
        if (bytes) ok &= hipMemcpyAsync(s.dst, s.src, bytes, hipMemcpyDeviceToDevice, stream) == hipSuccess;
    }
    ok &= hipStreamSynchronize(stream) == hipSuccess;
    return ok ? 1 : 0;
}
// Masters every signal (src -> dst) and leaves mst::kFields doubles per signal in out.  `label(i)` names signal i in errors.
// On any failure once the passes have begun (the ceiling not held, a HIP error, the meter failing) every dst holds its src again.
static int master_signals(hipStream_t stream, uint8_t** d_work, size_t* cap, uint8_t** d_loud, size_t* loud_cap, ProfCtx* prof,
                          const std::vector<mst::Signal>& sig, double T, double C, double lookahead_ms, double release_ms,
                          double* out, std::string (*label)(size_t)) {
    const size_t n = sig.size();
    if (!n) return 1;
    std::vector<double> fin(8 * n), fig(8 * n);
    {
        std::vector<loud::Signal> ms;
        for (const mst::Signal& s : sig) ms.push_back(meter_view(s.src, s));
        if (!measure_loudness(stream, d_loud, loud_cap, prof, ms, fin.data(), nullptr)) return 0;
    }
    for (size_t i = 0; i < n; ++i)
        if (!std::isfinite(fin[8 * i]))
            return fail("master: nothing to master (" + label(i) + "integrated loudness " + std::to_string(fin[8 * i]) +
                        ": silence, fewer than 4 hops or everything gated)");
    // the workspace: descriptors, min-G words, then per signal q, agg, carry
    std::vector<MasterDesc> d(n);
    std::vector<mst::Loop> lp(n);
    const size_t desc_b = align256(n * sizeof(MasterDesc)), gmin_b = align256(n * 4);
    size_t need = desc_b + gmin_b;
    std::vector<size_t> q_off(n), a_off(n), c_off(n);
    uint32_t max_tiles = 0;
    for (size_t i = 0; i < n; ++i) {
        mst::describe(sig[i], mst::window(lookahead_ms, sig[i].sr), mst::release_coef(release_ms, sig[i].sr), d[i]);
        lp[i].start(T, C, fin[8 * i]);
        q_off[i] = need;
        need += align256(sig[i].frames * 4);
        a_off[i] = need;
        need += align256((size_t)d[i].n_tiles * 8);
        c_off[i] = need;
        need += align256((size_t)d[i].n_tiles * 8);
        max_tiles = std::max(max_tiles, d[i].n_tiles);
    }
    if (!grow_device(stream, d_work, cap, need)) return 0;
    uint8_t* w = *d_work;
    uint32_t* d_gmin = (uint32_t*)(w + desc_b);
    for (size_t i = 0; i < n; ++i) {
        d[i].src = sig[i].src;
        d[i].dst = sig[i].dst;
        d[i].q = (float*)(w + q_off[i]);
        d[i].agg = (double*)(w + a_off[i]);
        d[i].carry = (double*)(w + c_off[i]);
        d[i].gmin = d_gmin + i;
        d[i].g = lp[i].g;
        d[i].cp = lp[i].cp;
    }
    ProfCtx none;
    ProfCtx& pc = prof ? *prof : none;
    pc.now = pc.every != 0;   // (every call is timed while profiling is on)
    TD_HIP(hipMemcpyAsync(w, d.data(), n * sizeof(MasterDesc), hipMemcpyHostToDevice, stream));
    {
        Prof pr(pc, F_MASTER_DETECT, stream);
        launch_master_detect((const MasterDesc*)w, (int)n, max_tiles, stream);
    }
    TD_HIP(hipGetLastError());
    std::vector<float> gmin(n, 1.0f);
    bool failed = false;
    auto run_passes = [&]() -> int {
        for (;;) {
            std::vector<size_t> act;
            for (size_t i = 0; i < n; ++i)
                if (!lp[i].done) act.push_back(i);
            if (act.empty()) break;
            std::vector<MasterDesc> ad;
            uint32_t at = 0;
            for (size_t i : act) {
                d[i].g = lp[i].g;
                d[i].cp = lp[i].cp;
                d[i].gmin = d_gmin + ad.size();
                ad.push_back(d[i]);
                at = std::max(at, d[i].n_tiles);
            }
            const int na = (int)ad.size();
            const std::vector<uint32_t> inf(act.size(), 0x7F800000u);
            TD_HIP(hipMemcpyAsync(w, ad.data(), ad.size() * sizeof(MasterDesc), hipMemcpyHostToDevice, stream));
            TD_HIP(hipMemcpyAsync(d_gmin, inf.data(), inf.size() * 4, hipMemcpyHostToDevice, stream));
            pc.now = pc.every != 0;
            { Prof pr(pc, F_MASTER_SCAN, stream); launch_master_scan((const MasterDesc*)w, na, at, stream); }
            { Prof pr(pc, F_MASTER_CARRY, stream); launch_master_carry((const MasterDesc*)w, na, stream); }
            { Prof pr(pc, F_MASTER_APPLY, stream); launch_master_apply((const MasterDesc*)w, na, at, stream); }
            TD_HIP(hipGetLastError());
            std::vector<uint32_t> words(act.size());
            TD_HIP(hipMemcpyAsync(words.data(), d_gmin, words.size() * 4, hipMemcpyDeviceToHost, stream));
            std::vector<loud::Signal> ms;
            for (size_t i : act) ms.push_back(meter_view(sig[i].dst, sig[i]));
            std::vector<double> f(8 * act.size());
            if (!measure_loudness(stream, d_loud, loud_cap, prof, ms, f.data(), nullptr)) return 0;   // (synchronises the stream)
            for (size_t k = 0; k < act.size(); ++k) {
                const size_t i = act[k];
                memcpy(&gmin[i], &words[k], 4);
                std::copy(f.begin() + (long)(8 * k), f.begin() + (long)(8 * k + 8), fig.begin() + (long)(8 * i));
                lp[i].after(f[8 * k], f[8 * k + 4]);
                failed |= lp[i].failed;
            }
        }
        return 1;
    };
    if (!run_passes()) {
        (void)restore_words(sig, stream);
        return 0;
    }
    if (failed) {
        std::string who;
        for (size_t i = 0; i < n && who.empty(); ++i)
            if (lp[i].failed) who = label(i) + "true peak " + std::to_string(fig[8 * i + 4]) + " dBTP";
        const bool back = restore_words(sig, stream);
        return fail("master: the ceiling could not be held (" + who + " after " + std::to_string(mst::kAimedPasses + 1) +
                    " passes): " + (back ? "the rendered words are back" : "HIP error while putting the rendered words back"));
    }
    for (size_t i = 0; i < n; ++i) {
        double* o = out + (size_t)mst::kFields * i;
        std::copy(fig.begin() + (long)(8 * i), fig.begin() + (long)(8 * i + 8), o);
        o[8] = fin[8 * i];
        o[9] = fin[8 * i + 4];
        o[10] = lp[i].g;
        o[11] = lp[i].cp;
        o[12] = (double)gmin[i];
        o[13] = (double)lp[i].passes;
        o[14] = lp[i].met ? 1.0 : 0.0;
    }
    return 1;
}
// The output of g's last whole render as a signal to master from the kept copy (made here when there is none).
static int master_view(td_graph* g, hipStream_t stream, mst::Signal* s) {
    const size_t bytes = g->loud_frames * (g->loud_bits > 16 ? 8 : 4);
    if (!g->master_kept) {
        if (!grow_device(stream, &g->d_master_src, &g->master_src_cap, bytes)) return 0;
        TD_HIP(hipMemcpyAsync(g->d_master_src, g->d_pcm, bytes, hipMemcpyDeviceToDevice, stream));
        g->master_kept = true;
    }
    s->src = g->d_master_src;
    s->dst = g->d_pcm;
    s->kind = g->loud_bits > 16 ? 1u : 0u;
    s->bits = g->loud_bits;
    s->frames = g->loud_frames;
    s->sr = g->loud_sr;
    return 1;
}
int td_graph_master(td_graph* g, double target_lufs, double ceiling_dbtp, double lookahead_ms, double release_ms, double* out) {
    const std::string bad = mst::check(target_lufs, ceiling_dbtp, lookahead_ms, release_ms);
    if (!bad.empty()) return fail(bad);
    if (!g->loud_frames || !g->d_pcm) return fail("master: no whole render to master (td_graph_render_all / _async / _resampled)");
    if (!drain(g)) return 0;   // (the deferred Normalize check and a guarded verdict settle first, as for td_graph_loudness)
    if (!g->loud_frames || !g->d_pcm) return fail("master: no whole render to master");
    if (!have_master_kernels()) return 0;
    if (!out) return fail("master: null report");
    mst::Signal s;
    if (!master_view(g, g->stream, &s)) return 0;
    return master_signals(g->stream, &g->d_master, &g->master_cap, &g->d_loud, &g->loud_cap, &g->prof, {s}, target_lufs,
                          ceiling_dbtp, lookahead_ms, release_ms, out, [](size_t) { return std::string(); });
}
int td_batch_master(td_batch* b, double target_lufs, double ceiling_dbtp, double lookahead_ms, double release_ms, double* out) {
    const std::string bad = mst::check(target_lufs, ceiling_dbtp, lookahead_ms, release_ms);
    if (!bad.empty()) return fail(bad);
    if (b->graphs.empty()) return 1;
    for (size_t i = 0; i < b->graphs.size(); ++i)
        if (!b->graphs[i]->loud_frames || !b->graphs[i]->d_pcm)
            return fail("master: project " + std::to_string(i) + " has no whole render to master");
    if (!ensure_device(b->device)) return 0;
    for (td_graph* g : b->graphs)
        if (!drain(g)) return 0;
    if (!have_master_kernels()) return 0;
    if (!out) return fail("master: null report");
    hipStream_t st = b->stream ? b->stream : b->graphs[0]->stream;
    std::vector<mst::Signal> sig(b->graphs.size());
    for (size_t i = 0; i < b->graphs.size(); ++i)
        if (!master_view(b->graphs[i], st, &sig[i])) return 0;
    return master_signals(st, &b->d_master, &b->master_cap, &b->d_loud, &b->loud_cap, &b->prof, sig, target_lufs, ceiling_dbtp,
                          lookahead_ms, release_ms, out, [](size_t i) { return "project " + std::to_string(i) + ": "; });
}
int td_master_f32(const float* lr, size_t frames, size_t sr, double target_lufs, double ceiling_dbtp, double lookahead_ms,
                  double release_ms, float* out_lr, double* out) {
    const std::string bad = mst::check(target_lufs, ceiling_dbtp, lookahead_ms, release_ms);
    if (!bad.empty()) return fail(bad);
    if (!ensure_device(cur_device())) return 0;
    if (frames && (!lr || !out_lr)) return fail("master_f32: null frames");
    if (!out) return fail("master_f32: null report");
    if (!have_master_kernels()) return 0;
    mst::Signal s;
    s.kind = 2;
    s.frames = frames;
    s.sr = sr;
    void* d_in = nullptr;
    void* d_out = nullptr;
    uint8_t *d_work = nullptr, *d_loud = nullptr;
    size_t cap = 0, loud_cap = 0;
    int ok = hipMalloc(&d_in, frames * 8 + 16) == hipSuccess && hipMalloc(&d_out, frames * 8 + 16) == hipSuccess
                 ? 1 : fail("master_f32: out of device memory");
    if (ok && frames && hipMemcpy(d_in, lr, frames * 8, hipMemcpyHostToDevice) != hipSuccess) ok = fail("HIP error: master_f32 upload");
    s.src = d_in;
    s.dst = d_out;
    if (ok)
        ok = master_signals(nullptr, &d_work, &cap, &d_loud, &loud_cap, nullptr, {s}, target_lufs, ceiling_dbtp, lookahead_ms,
                            release_ms, out, [](size_t) { return std::string(); });
    if (ok && frames && hipMemcpy(out_lr, d_out, frames * 8, hipMemcpyDeviceToHost) != hipSuccess) ok = fail("HIP error: master_f32 download");
    if (d_work) (void)hipFree(d_work);
    if (d_loud) (void)hipFree(d_loud);
    if (d_out) (void)hipFree(d_out);
    if (d_in) (void)hipFree(d_in);
    return ok;
}
const float* td_graph_output_f32_device(const td_graph* g) { return (const float*)g->last_out_f32; }
int td_graph_read_pcm(const td_graph* g, void* out, size_t bytes) {
    if (!g->d_pcm || bytes > g->pcm_bytes) return fail("read_pcm: nothing rendered / size too large");
    if (!drain(const_cast<td_graph*>(g))) return 0;
    if (debug_sync() & 4) fprintf(stderr, "R pcm %zu\n", bytes);
    TD_HIP(hipMemcpy(out, g->d_pcm, bytes, hipMemcpyDeviceToHost));
    if (debug_sync() & 4) fprintf(stderr, "ok\n");
    return 1;
}
int td_graph_read_f32(const td_graph* g, float* out, size_t n_floats) {
    if (!g->last_out_f32 || n_floats > g->last_frames * 2) return fail("read_f32: nothing rendered / size too large");
    if (!drain(const_cast<td_graph*>(g))) return 0;
    if (debug_sync() & 4) fprintf(stderr, "R f32 %zu\n", n_floats);
    TD_HIP(hipMemcpy(out, g->last_out_f32, n_floats * sizeof(float), hipMemcpyDeviceToHost));
    if (debug_sync() & 4) fprintf(stderr, "ok\n");
    return 1;
}
float td_graph_output_peak(const td_graph* gc) {
    td_graph* g = const_cast<td_graph*>(gc);
    if (!g->last_out_f32 || !g->last_frames) return 0.0f;
    if (!drain(g)) return 0.0f;
    launch_absmax((const float*)g->last_out_f32, (uint32_t)std::min<size_t>(g->last_frames * 2, 0xFFFFFFFFu), g->d_scalar,
                  g->stream);
    float v = 0.0f;
    if (hipMemcpyAsync(&v, g->d_scalar, 4, hipMemcpyDeviceToHost, g->stream) != hipSuccess) return 0.0f;
    (void)hipStreamSynchronize(g->stream);
    return v;
}
size_t td_graph_host_times(td_graph* g, double* ms4, int reset) {
    for (int i = 0; i < 4; ++i) ms4[i] = g->host_ms[i];
    const size_t n = g->host_chunks;
    if (reset) { for (double& v : g->host_ms) v = 0.0; g->host_chunks = 0; }
    return n;
}
static void prof_set(ProfCtx& pc, int on) {
    pc.every = on > 0 ? (unsigned)on : 0u;
    pc.count = 0;
    pc.now = false;
    for (auto& e : pc.pending) { pc.free_ev.push_back(e.a); pc.free_ev.push_back(e.b); }
    pc.pending.clear();
    pc.last_times.clear();
}
// (the caller has synchronised the stream the events were recorded on)
static size_t prof_collect(ProfCtx& pc, const char** names, float* ms, size_t* launches, size_t cap) {
    if (pc.last_times.empty()) {
        pc.last_times.resize(F_COUNT);
        for (int f = 0; f < F_COUNT; ++f) pc.last_times[f].name = kFamilyName[f];
    }
    for (auto& e : pc.pending) {
        float t = 0.f;
        if (hipEventElapsedTime(&t, e.a, e.b) == hipSuccess) {
            pc.last_times[e.fam].ms += t;
            pc.last_times[e.fam].launches += 1;
        }
        pc.free_ev.push_back(e.a);
        pc.free_ev.push_back(e.b);
    }
    pc.pending.clear();
    size_t n = 0;
    for (auto& kt : pc.last_times) {
        if (!kt.launches) continue;
        if (n < cap) {
            names[n] = kt.name.c_str();
            ms[n] = kt.ms;
            launches[n] = kt.launches;
        }
        ++n;
    }
    return std::min(n, cap);
}
void td_graph_set_profiling(td_graph* g, int on) { prof_set(g->prof, on); }
size_t td_graph_last_kernel_times(const td_graph* gc, const char** names, float* ms, size_t* launches, size_t cap) {
    td_graph* g = const_cast<td_graph*>(gc);
    if (!(g->stream && hipSetDevice(g->device) == hipSuccess)) return 0;
    (void)hipStreamSynchronize(g->stream);
    return prof_collect(g->prof, names, ms, launches, cap);
}
int td_device_sinf(const float* in, float* out, size_t n, int sine_mode) {   // (diagnostic: the engine's sine over a host array)
    if (!n) return 1;
    if (n > 0x40000000u) return fail("td_device_sinf: at most 2^30 values per call");   // (the kernel strides a 32-bit index)
    if (!ensure_device(cur_device())) return 0;
    float *d_in = nullptr, *d_out = nullptr;
    TD_HIP(hipMalloc(&d_in, n * sizeof(float)));
    if (hipMalloc(&d_out, n * sizeof(float)) != hipSuccess) { (void)hipFree(d_in); return fail("td_device_sinf: out of device memory"); }
    int ok = hipMemcpy(d_in, in, n * sizeof(float), hipMemcpyHostToDevice) == hipSuccess;
    if (ok) {
        launch_sinf(d_in, d_out, (uint32_t)n, sine_mode != 0, nullptr);
        ok = hipDeviceSynchronize() == hipSuccess && hipMemcpy(out, d_out, n * sizeof(float), hipMemcpyDeviceToHost) == hipSuccess;
    }
    (void)hipFree(d_in);
    (void)hipFree(d_out);
    return ok ? 1 : fail("td_device_sinf: HIP error");
}
void td_trim_memory(void) { tde::mem_trim(); }
size_t td_cached_memory_bytes(void) { return tde::mem_cached_bytes(); }
size_t td_graph_device_bytes(const td_graph* g) { return g->device_bytes + g->arena.device_bytes; }

int td_graph_band_guard_stats(const td_graph* g, double out[4]) {
    out[0] = (double)g->guard.audits;
    out[1] = (double)g->guard.redos;
    out[2] = (double)g->guard.last_est;
    out[3] = (double)g->guard.max_est;
    return 1;
}
int td_graph_band_stats(const td_graph* gc, uint32_t out[3]) {
    td_graph* g = const_cast<td_graph*>(gc);
    out[0] = out[1] = out[2] = 0;
    if (g->band_stats_off.empty() || !g->band_stats_base) return 1;
    if (!ensure_device(g->device)) return 0;
    TD_HIP(hipStreamSynchronize(g->stream));
    for (size_t so : g->band_stats_off) {
        uint32_t s[4];
        TD_HIP(hipMemcpy(s, g->band_stats_base + so, 16, hipMemcpyDeviceToHost));
        for (int i = 0; i < 3; ++i) out[i] += s[i];
    }
    return 1;
}

// ---- engine options.  SEVEN supported keys (include/termdaw_amd.h); everything else an engine ever grew a switch for is either gone
// (branch streams, HIP-graph replay, the serial-only band-pass: measured slower) or a TEST HOOK under "debug.<name>":
// value-neutral by construction -- it selects an older or alternative form of a launch, or moves a speculation parameter whose
// outcome is verified on the device -- and each is pinned by the test named in the header.  td_graph_get_option reads any of them.
struct OptionRef { const char* key; int kind; void* p; };   // kind 0 bool, 1 int, 2 unsigned, 3 size_t
static std::vector<OptionRef> option_table(td_graph* g) {
    return {
        {"fuse_sources", 0, &g->fuse_sources}, {"packed_samples", 0, &g->packed_samples}, {"band_mode", 1, &g->band_mode},
        {"band_guard_ppb", 2, &g->band_guard_ppb}, {"sine_mode", 1, &g->sine_mode}, {"output_f32", 0, &g->output_f32},
        {"max_chunk_frames", 3, &g->max_chunk_frames},
        {"debug.norm", 1, &g->norm_debug}, {"debug.sum_groups", 2, &g->sum_groups}, {"debug.band_scan", 1, &g->band_scan_debug}, {"debug.one_grid_sources", 0, &g->one_grid_sources}, {"debug.inline_probe", 0, &g->inline_probe},
        {"debug.inline_adsr", 0, &g->inline_adsr}, {"debug.spec_normalize", 0, &g->spec_normalize},
        {"debug.single_pass_normalize", 0, &g->single_pass_normalize}, {"debug.fuse_normalize", 0, &g->fuse_normalize},
        {"debug.table_cache", 0, &g->table_cache}, {"debug.band_serial", 0, &g->band_serial}, {"debug.band_chain", 0, &g->band_chain}, {"debug.band_scan_nf", 1, &g->band_scan_nf},
        {"debug.delay_tile", 2, &g->delay_tile}, {"debug.sat_tile", 2, &g->sat_tile}, {"debug.chorus_tile", 2, &g->chorus_tile},
        {"debug.reverb_form", 2, &g->reverb_form}, {"debug.reverb_block", 2, &g->reverb_block},
        {"debug.band_quick", 2, &g->band_quick}, {"debug.band_short", 2, &g->band_short}, {"debug.band_medium", 2, &g->band_medium},
        {"debug.band_warmup", 2, &g->band_warmup}, {"debug.band_depth", 2, &g->band_depth},
        {"debug.stem_taps", 2, &g->stem_taps}, {"debug.norm_early_store", 0, &g->norm_early_store},
    };
}
int td_graph_set_option(td_graph* g, const char* key, long value) {
    const std::string k = key ? key : "";
    // (keys with a rule of their own first)
    if (k == "debug.stem_taps") return fail("td_graph_set_option: debug.stem_taps is read-only");
    if (k == "debug.norm_early_store") return fail("td_graph_set_option: debug.norm_early_store is read-only (debug.norm bit 3 selects the other order)");
    if (k == "band_mode") {   // 0: exact (default, the parity mode), 1: blocked affine scan (tolerance class), 2: the scan under the guard
        if (value != 0 && value != 1 && value != 2) return fail("band_mode must be 0 (exact), 1 (scan) or 2 (guarded scan)");
        if (g->guard.armed && !drain(g)) return 0;   // (a verdict still out belongs to the mode it was rendered in)
        g->band_mode = (int)value;
        return 1;
    }
    if (k == "sine_mode") {   // 0: the fast device forms, 1: glibc's sinf operation for operation (kernels.hip sin_glibc), 2: the fast forms under the guard
        if (value != 0 && value != 1 && value != 2) return fail("td_graph_set_option: sine_mode is 0 (fast), 1 (glibc's sinf) or 2 (fast under the guard)");
        if (g->guard.armed && !drain(g)) return 0;   // (a verdict still out belongs to the mode it was rendered in)
        g->sine_mode = (int)value;
        for (auto& v : g->vertices)
            if (v.kind == K_DEBUG_SINE || v.kind == K_SYNTH) v.exact_sin = value == 1;   // (compile_chunk decides per chunk in mode 2)
        return 1;
    }
    if (k == "band_guard_ppb") { g->band_guard_ppb = value > 0 ? (unsigned)std::min<long>(value, 1000000000L) : 0u; return 1; }
    if (k == "max_chunk_frames") {
        if (value < 1) return fail("max_chunk_frames must be >= 1");
        g->max_chunk_frames = (size_t)value;
        return 1;
    }
    if (k == "debug.band_scan_nf") {
        if (value != 8 && value != 16) return fail("debug.band_scan_nf must be 8 or 16");
        g->band_scan_nf = (int)value;
        return 1;
    }
    if (k == "debug.delay_tile") {
        if (value != 8 && value != 16 && value != 32 && value != 64) return fail("debug.delay_tile must be 8, 16, 32 or 64");
        g->delay_tile = (unsigned)value;
        return 1;
    }
    if (k == "debug.sat_tile") {
        if (value != 128 && value != 256 && value != 384) return fail("debug.sat_tile must be 128, 256 or 384");
        g->sat_tile = (unsigned)value;
        return 1;
    }
    if (k == "debug.chorus_tile") {
        if (value != 256 && value != 512 && value != 1024) return fail("debug.chorus_tile must be 256, 512 or 1024");
        g->chorus_tile = (unsigned)value;
        return 1;
    }
    if (k == "debug.reverb_form") {
        if (value != 0 && value != 1) return fail("debug.reverb_form must be 0 (serial) or 1 (scan)");
        g->reverb_form = (unsigned)value;
        return 1;
    }
    if (k == "debug.reverb_block") {
        if (value != 64 && value != 128 && value != 256) return fail("debug.reverb_block must be 64, 128 or 256");
        g->reverb_block = (unsigned)value;
        return 1;
    }
    if (k == "debug.band_live_exp") { g->band_live_thr = value >= 38 ? 0.0f : powf(10.0f, -(float)value); return 1; }
    if (k == "debug.band_short") { g->band_short = value > 0 ? (unsigned)value : 64u; return 1; }
    if (k == "debug.band_medium") { g->band_medium = value > 0 ? (unsigned)value : 30u; return 1; }
    if (k == "debug.band_depth") { g->band_depth = value > 0 ? (unsigned)value : 100u; return 1; }
    if (k == "debug.band_warmup") { g->band_warmup = value > 0 ? (unsigned)value : 150u; return 1; }
    for (const OptionRef& o : option_table(g)) {
        if (k != o.key) continue;
        switch (o.kind) {
            case 0: *(bool*)o.p = value != 0; break;
            case 1: *(int*)o.p = (int)value; break;
            case 2: *(unsigned*)o.p = value > 0 ? (unsigned)value : 0u; break;
            default: *(size_t*)o.p = value > 0 ? (size_t)value : 0; break;
        }
        return 1;
    }
    return fail("unknown option \"" + k + "\"");
}
int td_graph_get_option(const td_graph* g, const char* key, long* value) {
    const std::string k = key ? key : "";
    for (const OptionRef& o : option_table(const_cast<td_graph*>(g))) {
        if (k != o.key) continue;
        switch (o.kind) {
            case 0: *value = *(const bool*)o.p ? 1 : 0; break;
            case 1: *value = *(const int*)o.p; break;
            case 2: *value = (long)*(const unsigned*)o.p; break;
            default: *value = (long)*(const size_t*)o.p; break;
        }
        return 1;
    }
    return fail("unknown option \"" + k + "\"");
}
// (the option keys, for tests that walk them: n-th key or NULL)
const char* td_graph_option_key(size_t n) {
    static td_graph dummy_for_keys;
    static const std::vector<OptionRef> t = option_table(&dummy_for_keys);
    return n < t.size() ? t[n].key : nullptr;
}

// ---- Batch (no reference counterpart: the reference renders one project per process; this is the loop a
// batch driver would run State::render, state.rs:563-575, in for many independent States) ----
td_batch* td_batch_new(void) {
    td_batch* b = new td_batch();
    b->device = t_device;
    return b;
}
void td_batch_free(td_batch* b) {
    if (!b) return;
    const bool dev_ok = hipSetDevice(b->device) == hipSuccess;
    if (b->stream && dev_ok) (void)settle_arena(b->arena, b->stream);   // (the projects' results stay readable through their own handles)
    for (td_graph* g : b->graphs) {   // the projects outlive the batch: give each its own stream back (made on next use)
        // (a member rendered on its own queues on the batch's stream with its own arena: its deferred check, if one is
        // outstanding, must run before that stream goes)
        if (b->stream && dev_ok) (void)settle_arena(g->arena, b->stream);
        drop_pending(g->arena);
        g->batch = nullptr;
        g->stream = nullptr;
        g->owns_stream = true;
        g->band_stats_base = nullptr;   // (it pointed into the batch arena's scratch, freed below)
        g->band_stats_off.clear();
        if (g->pcm_borrowed) { g->d_pcm = nullptr; g->pcm_cap = 0; g->pcm_bytes = 0; g->pcm_borrowed = false; g->loud_frames = 0; g->master_kept = false; }   // (a slice of the batch's PCM arena)
        if (dev_ok && hipStreamCreateWithFlags(&g->stream, hipStreamNonBlocking) != hipSuccess) g->stream = nullptr;
    }
    if (dev_ok) {
        free_arena(b->arena);
        free_prof(b->prof);
        if (b->d_peaks) (void)hipFree(b->d_peaks);
        if (b->d_table) (void)hipFree(b->d_table);
        if (b->h_table) (void)hipHostFree(b->h_table);
        if (b->copy_stream) { (void)hipStreamSynchronize(b->copy_stream); (void)hipStreamDestroy(b->copy_stream); }
        if (b->d_pcm_arena) (void)hipFree(b->d_pcm_arena);
        if (b->d_loud) (void)hipFree(b->d_loud);
        if (b->d_master) (void)hipFree(b->d_master);
        for (hipEvent_t e : b->ev_pool) (void)hipEventDestroy(e);
        for (hipEvent_t e : b->ev_mark) if (e) (void)hipEventDestroy(e);
        if (b->host_pcm) (void)hipHostFree(b->host_pcm);
        if (b->stream) (void)hipStreamDestroy(b->stream);
    }
    drop_pending(b->arena);
    delete b;
}
long td_batch_add(td_batch* b, td_graph* g, const td_samplebank* sb, td_flowwbank* fb) {
    if (!g || !sb || !fb) { fail("td_batch_add: null handle"); return -1; }
    if (g->batch) { fail("td_batch_add: the graph already belongs to a batch"); return -1; }
    if (g->device != b->device || sb->device != b->device) { fail("td_batch_add: project and batch live on different devices"); return -1; }
    if (!ensure_device(b->device)) return -1;
    if (!b->stream && hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking) != hipSuccess) {
        fail("td_batch_add: cannot create a HIP stream");
        return -1;
    }
    // the graph's launches, state copies and memsets move to the batch's stream
    if (g->stream) {
        (void)drain(g);   // (its own arena's deferred check, if any, runs on the stream about to go)
        if (g->owns_stream) (void)hipStreamDestroy(g->stream);
    }
    g->stream = b->stream;
    g->owns_stream = false;
    g->batch = b;
    b->graphs.push_back(g);
    b->sbs.push_back(sb);
    b->fbs.push_back(fb);
    return (long)b->graphs.size() - 1;
}
size_t td_batch_size(const td_batch* b) { return b->graphs.size(); }
/* reset_normalize_vertices (state.rs:467) + FlowwBank::set_time(0) for every project: the state right after refresh */
void td_batch_rewind(td_batch* b) {
    for (size_t i = 0; i < b->graphs.size(); ++i) {
        td_graph_reset_normalize_vertices(b->graphs[i]);
        b->fbs[i]->set_time(0);
    }
}
size_t td_batch_render_all_async(td_batch* b, size_t n_blocks, int bits) {
    if (!batch_render_chunks(b, n_blocks, false, bits, true, true)) return 0;
    for (td_graph* g : b->graphs) {
        if (!graph_set_time_impl(g, 0)) return 0;   // state.rs:575
        }
    return b->graphs.empty() ? 0 : n_blocks * b->graphs[0]->bl;
}
int td_batch_sync(td_batch* b) {
    if (!b->stream) return 1;
    if (!ensure_device(b->device)) return 0;
    if (!settle_arena(b->arena, b->stream)) return 0;
    for (td_graph* g : b->graphs)   // (band_mode 2: a project whose estimate was over the bound renders again, alone, exact)
        if (g->guard.armed && !guard_settle(g)) return 0;
    return 1;
}
size_t td_batch_render_all(td_batch* b, size_t n_blocks, int bits) {
    const size_t n = td_batch_render_all_async(b, n_blocks, bits);
    if (!n) return 0;
    if (!td_batch_sync(b)) return 0;
    return n;
}

// State::render (state.rs:477-577) for every project of the batch, END TO END: render, PCM to the host, the WAV file.
// The projects render in groups of `group` (one submission each, queued back to back on the batch's stream) into ONE device
// arena, project after project; a copy stream takes each group's PCM -- one contiguous transfer -- to page-locked host memory
// as soon as the group has rendered, while the next groups render; `writers` host threads write project i's file -- hound's
// header (wav.cpp) + the PCM words -- as soon as its group's copy has landed.  Returns when every file is written.
// (Measured: one copy per project leaves ~38 us between transfers, 0.84 of the pinned copy rate; two copy streams make the
// runtime copy with shader kernels that take the CUs from the renders: 27 GB/s and renders twice as slow.)
int td_batch_render_to_files(td_batch* b, size_t n_blocks, int bits, size_t render_sr, const char* const* paths, int group,
                             int writers, double* times) {
    const size_t P = b->graphs.size();
    if (times) for (int i = 0; i < 8; ++i) times[i] = 0.0;
    if (!P) return 1;
    if (!ensure_device(b->device)) return 0;
    if (!(bits == 8 || bits == 16 || bits == 24 || bits == 32)) return fail("Bitdepth not supported: choose bitdepth in {8, 16, 24, 32}.");
    for (size_t i = 0; i < P; ++i)
        if (!b->graphs[i]->stems.empty()) return fail("td_batch: project " + std::to_string(i) + " has stems set: batches do not render stems");
    const size_t G = group > 0 ? (size_t)group : 8;
    const size_t n_groups = (P + G - 1) / G;
    const auto w0 = std::chrono::steady_clock::now();
    if (!b->copy_stream) TD_HIP(hipStreamCreateWithFlags(&b->copy_stream, hipStreamNonBlocking));
    // events: [g] render of group g done; a timed pair around every group's copy; two timed ones around the renders
    const size_t n_ev = 3 * n_groups + 2;
    while (b->ev_pool.size() < n_ev) {
        hipEvent_t e = nullptr;
        TD_HIP(hipEventCreate(&e));
        b->ev_pool.push_back(e);
    }
    hipEvent_t* ev_group = b->ev_pool.data();
    hipEvent_t* ev_c0 = ev_group + n_groups;
    hipEvent_t* ev_c1 = ev_c0 + n_groups;
    hipEvent_t ev_r0 = ev_c1[n_groups], ev_r1 = ev_c1[n_groups + 1];
    // one slice per project, the same layout on the device and in page-locked host memory (kept from call to call)
    const size_t word = bits > 16 ? 4 : 2;
    b->host_pcm_off.assign(P, 0);
    b->host_pcm_bytes.assign(P, 0);
    std::vector<size_t> slice(P);
    size_t need = 0;
    for (size_t i = 0; i < P; ++i) {
        b->host_pcm_off[i] = need;
        b->host_pcm_bytes[i] = n_blocks * b->graphs[i]->bl * 2 * word;
        slice[i] = (b->host_pcm_bytes[i] + 64 + 4095) & ~(size_t)4095;   // (+ 64: the engine's own pad behind a PCM buffer)
        need += slice[i];
    }
    if (need > b->host_pcm_cap) {
        if (b->host_pcm) (void)hipHostFree(b->host_pcm);
        b->host_pcm = nullptr;
        b->host_pcm_cap = 0;
        TD_HIP(hipHostMalloc((void**)&b->host_pcm, need, hipHostMallocDefault));
        b->host_pcm_cap = need;
    }
    bool relayout = need > b->d_pcm_arena_cap;
    for (size_t i = 0; i < P && !relayout; ++i)
        relayout = !(b->graphs[i]->pcm_borrowed && b->graphs[i]->d_pcm == b->d_pcm_arena + b->host_pcm_off[i] && b->graphs[i]->pcm_cap >= slice[i]);
    if (relayout) {
        if (!settle_arena(b->arena, b->stream)) return 0;   // (nothing queued may still write an old PCM buffer)
        if (need > b->d_pcm_arena_cap) {
            for (td_graph* g : b->graphs)
                if (g->pcm_borrowed) { g->d_pcm = nullptr; g->pcm_cap = 0; g->pcm_bytes = 0; g->pcm_borrowed = false; g->loud_frames = 0; g->master_kept = false; }
            if (b->d_pcm_arena) (void)hipFree(b->d_pcm_arena);
            b->d_pcm_arena = nullptr;
            b->d_pcm_arena_cap = 0;
            TD_HIP(hipMalloc((void**)&b->d_pcm_arena, need));
            b->d_pcm_arena_cap = need;
        }
        for (size_t i = 0; i < P; ++i) {
            td_graph* g = b->graphs[i];
            if (g->d_pcm && !g->pcm_borrowed) { (void)hipFree(g->d_pcm); g->device_bytes -= g->pcm_cap; }
            g->d_pcm = b->d_pcm_arena + b->host_pcm_off[i];
            g->pcm_cap = slice[i];
            g->pcm_bytes = 0;
            g->pcm_borrowed = true;
        }
    }
    const auto w1 = std::chrono::steady_clock::now();
    // writer threads: project i is theirs once its group's copy has completed
    std::atomic<size_t> next{0};
    std::atomic<int> failed{0};
    const size_t nw = paths ? (size_t)std::max(writers, 1) : 0;   // (files asked for: at least one writer, whatever `writers` says)
    std::vector<std::string> errs(nw);
    std::vector<double> first_write(nw, -1.0), last_write(nw, 0.0);
    std::atomic<size_t> queued{0};   // groups whose copy has been enqueued (their events are recorded)
    std::mutex q_mu;                 // (writers sleep on q_cv until their group is queued: up to 96 of them spinning on `queued` took
    std::condition_variable q_cv;    //  host cores from the thread that enqueues the renders)
    const int dev = b->device;
    // a file is written in `parts` slices by as many threads (pwrite at their own offsets): the last group's files -- nothing
    // renders or copies under them any more -- are then finished by all the writers, not by one thread per file
    const size_t parts = (bits == 16 || bits == 32) ? (size_t)std::max<long>(1, std::min<long>(8, (long)nw * 2 / (long)std::max<size_t>(G, 1))) : 1;
    auto writer = [&](size_t w) {
        (void)hipSetDevice(dev);
        for (;;) {
            const size_t task = next.fetch_add(1);
            if (task >= P * parts) return;
            const size_t i = task / parts, part = task % parts;
            const size_t gi = i / G;
            {
                std::unique_lock<std::mutex> lk(q_mu);
                q_cv.wait(lk, [&] { return queued.load(std::memory_order_acquire) > gi || failed.load() != 0; });
                if (queued.load(std::memory_order_acquire) <= gi) return;   // (failed)
            }
            if (hipEventSynchronize(ev_c1[gi]) != hipSuccess) { failed = 1; errs[w] = "copy event failed"; return; }
            const double t_a = ms_between(w0, std::chrono::steady_clock::now());
            if (first_write[w] < 0) first_write[w] = t_a;
            std::string err;
            const void* words = b->host_pcm + b->host_pcm_off[i];
            const size_t frames = n_blocks * b->graphs[i]->bl;
            const bool ok_w = parts > 1 ? tdw::write_wav_int_part(paths[i], words, frames, 2, render_sr, bits, (int)part, (int)parts, &err)
                                        : tdw::write_wav_int(paths[i], words, frames, 2, render_sr, bits, &err);
            if (!ok_w) {
                failed = 1;
                errs[w] = err;
                return;
            }
            last_write[w] = ms_between(w0, std::chrono::steady_clock::now());
        }
    };
    std::vector<std::thread> pool;
    for (size_t w = 0; w < nw; ++w) pool.emplace_back(writer, w);
    int ok = 1;
    if (hipEventRecord(ev_r0, b->stream) != hipSuccess) ok = fail("HIP error: event");
    for (size_t gi = 0; gi < n_groups && ok; ++gi) {
        const size_t lo = gi * G, hi = std::min(P, lo + G);
        ok = batch_render_range(b, lo, hi, n_blocks, false, bits, true, true, false);
        for (size_t i = lo; i < hi && ok; ++i) {
            ok = graph_set_time_impl(b->graphs[i], 0);   // state.rs:575
        }
        {   // (band_mode 2: a group with guarded projects is settled -- verdicts looked at, a project over the bound done again -- before its PCM leaves)
            bool any_armed = false;
            for (size_t i = lo; i < hi; ++i) any_armed = any_armed || b->graphs[i]->guard.armed;
            if (ok && any_armed) {
                ok = settle_arena(b->arena, b->stream);
                for (size_t i = lo; i < hi && ok; ++i) ok = guard_settle(b->graphs[i]);
            }
        }
        if (!ok) break;
        const size_t bytes = b->host_pcm_off[hi - 1] + b->host_pcm_bytes[hi - 1] - b->host_pcm_off[lo];
        if (hipEventRecord(ev_group[gi], b->stream) != hipSuccess || hipStreamWaitEvent(b->copy_stream, ev_group[gi], 0) != hipSuccess ||
            hipEventRecord(ev_c0[gi], b->copy_stream) != hipSuccess ||
            hipMemcpyAsync(b->host_pcm + b->host_pcm_off[lo], b->d_pcm_arena + b->host_pcm_off[lo], bytes, hipMemcpyDeviceToHost, b->copy_stream) != hipSuccess ||
            hipEventRecord(ev_c1[gi], b->copy_stream) != hipSuccess) { ok = fail("HIP error: PCM copy to the host"); break; }
        {
            std::lock_guard<std::mutex> lk(q_mu);
            queued.store(gi + 1, std::memory_order_release);
        }
        q_cv.notify_all();
    }
    if (ok && hipEventRecord(ev_r1, b->stream) != hipSuccess) ok = fail("HIP error: event");
    if (!ok) {
        std::lock_guard<std::mutex> lk(q_mu);
        failed = 1;
    }
    q_cv.notify_all();
    const auto w2 = std::chrono::steady_clock::now();
    for (auto& t : pool) t.join();
    if (hipStreamSynchronize(b->copy_stream) != hipSuccess || hipStreamSynchronize(b->stream) != hipSuccess) ok = ok && fail("HIP error: stream");
    const auto w3 = std::chrono::steady_clock::now();
    if (ok && failed.load()) {
        std::string e = "td_batch_render_to_files: ";
        for (auto& x : errs) if (!x.empty()) { e += x; break; }
        return fail(e);
    }
    if (!ok) return 0;
    if (times) {
        float ms = 0.f;
        times[0] = ms_between(w0, w3);                         // wall: whole call
        times[1] = ms_between(w0, w1);                         // of which: buffers (first call only) + events
        if (hipEventElapsedTime(&ms, ev_r0, ev_r1) == hipSuccess) times[2] = ms;                    // GPU: first render start -> last render end
        if (hipEventElapsedTime(&ms, ev_c0[0], ev_c1[n_groups - 1]) == hipSuccess) times[3] = ms;   // copy stream: first copy start -> last copy end
        double busy = 0.0, bytes = 0.0;
        for (size_t gi = 0; gi < n_groups; ++gi)
            if (hipEventElapsedTime(&ms, ev_c0[gi], ev_c1[gi]) == hipSuccess) busy += ms;
        for (size_t i = 0; i < P; ++i) bytes += (double)b->host_pcm_bytes[i];
        times[4] = busy;                                       // sum of the copies' own durations
        times[5] = bytes;
        double fw = -1.0, lw = 0.0;
        for (size_t w = 0; w < nw; ++w) {
            if (first_write[w] >= 0 && (fw < 0 || first_write[w] < fw)) fw = first_write[w];
            lw = std::max(lw, last_write[w]);
        }
        times[6] = fw < 0 ? 0.0 : lw - fw;                     // host: first file opened -> last file closed
        times[7] = ms_between(w1, w2);                         // host: time to enqueue everything
    }
    return 1;
}
const void* td_batch_host_pcm(const td_batch* b, size_t i, size_t* bytes) {
    if (bytes) *bytes = 0;
    if (!b->host_pcm || i >= b->host_pcm_off.size()) return nullptr;
    if (bytes) *bytes = b->host_pcm_bytes[i];
    return b->host_pcm + b->host_pcm_off[i];
}
int td_batch_normalize_scan(td_batch* b, size_t chunks) {   // State::scan_exact (state.rs:473-475) for every project
    for (size_t i = 0; i < b->graphs.size(); ++i)
        if (!b->graphs[i]->stems.empty()) return fail("td_batch: project " + std::to_string(i) + " has stems set: batches do not render stems");
    for (size_t i = 0; i < b->graphs.size(); ++i) {
        if (b->graphs[i]->output_vertex < 0) return fail("TermDaw: error: output vertex not found.");
        if (!scan_begin(b->graphs[i], b->fbs[i])) return 0;
    }
    if (!batch_render_chunks(b, chunks, true, 16, false, false)) return 0;
    {
        bool any_armed = false;
        for (td_graph* g : b->graphs) any_armed = any_armed || g->guard.armed;
        if (any_armed && !td_batch_sync(b)) return 0;   // (a dry run over the bound is done again before its peaks are applied)
    }
    for (size_t i = 0; i < b->graphs.size(); ++i)
        if (!scan_end(b->graphs[i], b->fbs[i])) return 0;
    return td_batch_sync(b);
}
// Per-project peak after the last render: the output Normalize vertex' running peak (`max`, extensions.rs:323 --
// the project's pre-normalisation peak), or the absolute peak of the output buffer when the output vertex is no
// Normalize.  Fills a table of n_total floats in DEVICE memory: project i of this batch goes to entry
// first + i * stride, every other entry is written as 0 -- ready for one all-reduce(max) across the ranks.
int td_batch_peak_table_device(td_batch* b, float* d_table, size_t n_total, size_t first, size_t stride) {
    const size_t P = b->graphs.size();
    if (stride == 0 || (P && first + (P - 1) * stride >= n_total)) return fail("td_batch_peak_table_device: table too small");
    if (n_total > 0xFFFFFFFFull) return fail("td_batch_peak_table_device: table too large");
    if (!ensure_device(b->device)) return 0;
    if (!b->stream) TD_HIP(hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking));
    // The table kernel goes out right behind whatever is queued -- no host wait in front of it.  The carried max of a single-pass
    // Normalize is final only once a deferred k_norm_fix has had its chance: with one outstanding the stream is drained
    // afterwards, and in the rare case that the check then redid a vertex the table is made again.
    auto enqueue_table = [&]() -> int {
        if (P > b->peaks_cap) {
            TD_HIP(hipStreamSynchronize(b->stream));
            if (b->d_peaks) (void)hipFree(b->d_peaks);
            b->d_peaks = nullptr;
            b->peaks_cap = 0;
            TD_HIP(hipMalloc(&b->d_peaks, (P + 10) * (sizeof(float) + sizeof(float*))));
            b->peaks_cap = P + 8;
            b->peak_src.clear();   // (the device copy of the pointer table went with the old allocation)
        }
        const float** d_src = reinterpret_cast<const float**>(b->d_peaks + ((b->peaks_cap + 1) & ~(size_t)1));
        std::vector<const float*> src(P);
        for (size_t i = 0; i < P; ++i) {
            td_graph* g = b->graphs[i];
            const Vertex* outv = g->output_vertex >= 0 ? &g->vertices[(size_t)g->output_vertex] : nullptr;
            if (outv && outv->kind == K_NORMALIZE && g->dstate && !outv->has_init_override) {
                src[i] = &g->dstate[outv->state_slot].norm.max;
            } else {
                src[i] = b->d_peaks + i;
                if (g->last_out_f32 && g->last_frames)
                    launch_absmax((const float*)g->last_out_f32, (uint32_t)std::min<size_t>(g->last_frames * 2, 0xFFFFFFFFu), b->d_peaks + i, b->stream);
                else
                    TD_HIP(hipMemsetAsync(b->d_peaks + i, 0, sizeof(float), b->stream));
            }
        }
        // the pointer table rarely changes (carried normalize states keep their addresses from render to render): the
        // device copy is reused, and the exchange then costs one small launch and no synchronisation
        if (src != b->peak_src) {
            b->peak_src = src;
            if (P) TD_HIP(hipMemcpyAsync(d_src, b->peak_src.data(), P * sizeof(float*), hipMemcpyHostToDevice, b->stream));
            TD_HIP(hipStreamSynchronize(b->stream));
        }
        if (n_total) launch_peak_table(d_src, d_table, (uint32_t)n_total, (uint32_t)P, (uint32_t)first, (uint32_t)stride, b->stream);
        TD_HIP(hipGetLastError());
        return 1;
    };
    const bool pending = !b->arena.pending_fix.empty();
    const size_t runs0 = b->arena.fix_runs;
    if (!enqueue_table()) return 0;
    if (pending) {
        if (!settle_arena(b->arena, b->stream)) return 0;
        if (b->arena.fix_runs != runs0 && !enqueue_table()) return 0;
    }
    return 1;
}
int td_batch_peaks(td_batch* b, float* out) {   // host copy of this batch's own entries, in td_batch_add order
    const size_t P = b->graphs.size();
    if (!P) return 1;
    if (!ensure_device(b->device)) return 0;
    float* d_tab = nullptr;
    TD_HIP(hipMalloc(&d_tab, P * sizeof(float)));
    int ok = td_batch_peak_table_device(b, d_tab, P, 0, 1);
    if (ok && (hipMemcpyAsync(out, d_tab, P * sizeof(float), hipMemcpyDeviceToHost, b->stream) != hipSuccess ||
               hipStreamSynchronize(b->stream) != hipSuccess))
        ok = fail("td_batch_peaks: read-back failed");
    (void)hipFree(d_tab);
    return ok;
}
// ---- the job's one collective (comm.h): all-reduce(max) of the per-project peak table across the ranks, behind the C ABI
int td_comm_unique_id(void* out, size_t bytes) {
    if (!out || bytes < 128) return fail("td_comm_unique_id: the id takes 128 bytes");
    return rccl_unique_id(out);
}
td_comm* td_comm_init(const void* unique_id, size_t bytes, int rank, int world) {
    if (!unique_id || bytes < 128) { fail("td_comm_init: the id takes 128 bytes"); return nullptr; }
    if (world < 1 || rank < 0 || rank >= world) { fail("td_comm_init: rank outside the job"); return nullptr; }
    if (!ensure_device(t_device)) return nullptr;
    td_comm* c = new td_comm();
    c->rank = rank; c->world = world; c->device = t_device; c->kind = 0;
    if (!rccl_init(c, unique_id, rank, world)) { delete c; return nullptr; }
    return c;
}
td_comm* td_comm_init_host(td_allreduce_max_fn allreduce_max, void* ctx, int rank, int world) {
    if (world < 1 || rank < 0 || rank >= world) { fail("td_comm_init_host: rank outside the job"); return nullptr; }
    if (!allreduce_max && world > 1) { fail("td_comm_init_host: no all-reduce given"); return nullptr; }
    td_comm* c = new td_comm();
    c->rank = rank; c->world = world; c->device = t_device; c->kind = 1;
    c->host_allreduce_max = allreduce_max;
    c->host_ctx = ctx;
    return c;
}
void td_comm_free(td_comm* c) {
    if (!c) return;
    if (c->kind == 0 && hipSetDevice(c->device) == hipSuccess) rccl_destroy(c);
    delete c;
}
const char* td_comm_backend(const td_comm* c) { return !c ? "none" : c->kind == 0 ? "rccl-native" : "host-callback"; }
const char* td_comm_library(void) { return rccl_library_path(); }
// The peak table of the whole job, per_rank x world floats: this rank's project i at entry rank + i * world, then ONE
// all-reduce(max) -- on the batch's stream right behind the renders and the table kernel, no host synchronisation in between
// (RCCL kind), or through the host's own all-reduce on the page-locked mirror (host kind).  c NULL: a job of one rank.
int td_batch_exchange_peaks(td_batch* b, td_comm* c, size_t per_rank) {
    const int rank = c ? c->rank : 0, world = c ? c->world : 1;
    if (b->graphs.size() > per_rank) return fail("td_batch_exchange_peaks: the batch holds more projects than per_rank");
    if (c && c->kind == 0 && c->device != b->device) return fail("td_batch_exchange_peaks: the communicator belongs to another device");
    const size_t n = per_rank * (size_t)world;
    if (!ensure_device(b->device)) return 0;
    if (!b->stream) TD_HIP(hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking));
    {   // (a guarded render whose verdict is still out may be done again: its peak is final only then)
        bool any_armed = false;
        for (td_graph* g : b->graphs) any_armed = any_armed || g->guard.armed;
        if (any_armed && !td_batch_sync(b)) return 0;
    }
    if (n > b->table_cap) {
        TD_HIP(hipStreamSynchronize(b->stream));
        if (b->d_table) (void)hipFree(b->d_table);
        if (b->h_table) (void)hipHostFree(b->h_table);
        b->d_table = b->h_table = nullptr;
        b->table_cap = 0;
        TD_HIP(hipMalloc((void**)&b->d_table, (n + 16) * sizeof(float)));
        TD_HIP(hipHostMalloc((void**)&b->h_table, (n + 16) * sizeof(float), hipHostMallocDefault));
        b->table_cap = n + 16;
    }
    b->table_n = n;
    if (!n) return 1;
    if (!td_batch_peak_table_device(b, b->d_table, n, (size_t)rank, (size_t)world)) return 0;
    if (!c) return 1;
    if (c->kind == 0) return rccl_allreduce_max_f32(c, b->d_table, n, b->stream);   // (a job of one rank too: the same call)
    if (world == 1 && !c->host_allreduce_max) return 1;
    TD_HIP(hipMemcpyAsync(b->h_table, b->d_table, n * sizeof(float), hipMemcpyDeviceToHost, b->stream));
    TD_HIP(hipStreamSynchronize(b->stream));
    if (!c->host_allreduce_max(c->host_ctx, b->h_table, n)) return fail("td_batch_exchange_peaks: the host's all-reduce failed");
    TD_HIP(hipMemcpyAsync(b->d_table, b->h_table, n * sizeof(float), hipMemcpyHostToDevice, b->stream));
    return 1;
}
const float* td_batch_peak_table(const td_batch* b, size_t* n) {
    if (n) *n = b->table_n;
    return b->d_table;
}
int td_batch_read_peak_table(td_batch* b, float* out, size_t n) {
    if (n > b->table_n) return fail("td_batch_read_peak_table: the table is shorter");
    if (!n) return 1;
    if (!ensure_device(b->device)) return 0;
    TD_HIP(hipMemcpyAsync(b->h_table, b->d_table, n * sizeof(float), hipMemcpyDeviceToHost, b->stream));
    TD_HIP(hipStreamSynchronize(b->stream));
    memcpy(out, b->h_table, n * sizeof(float));
    return 1;
}
void td_batch_set_profiling(td_batch* b, int on) { prof_set(b->prof, on); }
int td_batch_mark(td_batch* b, int which) {
    if (which < 0 || which > 1) return fail("td_batch_mark: which is 0 or 1");
    if (!ensure_device(b->device)) return 0;
    if (!b->stream) TD_HIP(hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking));
    if (!b->ev_mark[which]) TD_HIP(hipEventCreate(&b->ev_mark[which]));
    TD_HIP(hipEventRecord(b->ev_mark[which], b->stream));
    b->mark_set[which] = true;
    if (which == 0) b->mark_set[1] = false;
    return 1;
}
double td_batch_marked_ms(td_batch* b) {
    if (!(b->mark_set[0] && b->mark_set[1]) || hipSetDevice(b->device) != hipSuccess) return -1.0;
    float ms = -1.0f;
    if (hipEventSynchronize(b->ev_mark[1]) != hipSuccess || hipEventElapsedTime(&ms, b->ev_mark[0], b->ev_mark[1]) != hipSuccess) return -1.0;
    return (double)ms;
}
size_t td_batch_last_kernel_times(td_batch* b, const char** names, float* ms, size_t* launches, size_t cap) {
    if (!(b->stream && hipSetDevice(b->device) == hipSuccess)) return 0;
    (void)hipStreamSynchronize(b->stream);
    return prof_collect(b->prof, names, ms, launches, cap);
}
size_t td_batch_host_times(td_batch* b, double* ms4, int reset) {
    for (int i = 0; i < 4; ++i) ms4[i] = b->host_ms[i];
    const size_t n = b->host_steps;
    if (reset) { for (double& v : b->host_ms) v = 0.0; b->host_steps = 0; }
    return n;
}

}  // extern "C"
