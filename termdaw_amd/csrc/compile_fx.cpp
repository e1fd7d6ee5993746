// compile_fx.cpp -- the effect kinds of the host compiler (compile.h FxKind / FxLevel): compressor, EQ, delay, saturator,
// chorus, reverb, gate, phaser, vocoder, filter, limiter, multiband, convolution.  One table row per kind -- its chunk limit, the family its launches start at, the factor the guard
// carries an estimate through it at, the state slots it carries and their state at time 0, whether it takes a key, whether its
// kernels are linked; and the kind as the front ends see it: its script line, the schema of its parameters (fx_params.h), their
// check, how much of the check the script line is held to and what adding a vertex does beyond storing the block -- one function per
// kind that lowers a level's vertices of that kind to descriptors and launches, and right
// behind it the one that decodes such a launch and calls the kernels' entry points (kernels.h launch_*: the only calls out of the
// host compiler; no HIP call of its own, like compile.cpp).  compile_chunk, engine.cpp and project.cpp enumerate the kinds through
// the table only.  Not an object of its own: compile.cpp includes this file at its end, so no build list changes with it.
#include "chorus_math.h"
#include "comp_math.h"
#include "compile.h"
#include "conv_math.h"
#include "delay_math.h"
#include "eq_math.h"
#include "filter_math.h"
#include "gate_math.h"
#include "limiter_math.h"
#include "multiband_math.h"
#include "phaser_math.h"
#include "reverb_math.h"
#include "sat_math.h"
#include "vocoder_math.h"

#include <math.h>

#include <algorithm>

using namespace tdk;

namespace tde {

float2* FxLevel::tmp_buffer() {
    float2* b = take_buffer(g);
    if (!b) { fail("termdaw_amd: out of device memory for edge buffers"); return nullptr; }
    level_tmp.push_back(b);
    return b;
}

namespace fxk {   // (compile.cpp includes this file: what is only used here keeps a scope of its own)

// A delay, saturator, chorus, reverb, vocoder, limiter, multiband or convolution vertex enters a chunk of M frames: a set_time since the vertex last ran is consumed here
// (the block restarts from zero, like an EQ's state), the books move on behind the chunk -- `alternates`: the launch writes the other
// half of the line, which the next one reads.  Returns the frames run up to the chunk (Vertex::Line::total as the chunk finds it).
static uint64_t enter_chunk(Vertex& v, size_t M, bool alternates) {
    if (v.first_pending) v.line.total = 0;
    v.first_pending = false;
    const uint64_t total = v.line.total;
    v.line.total += M;
    if (alternates) v.line.parity ^= 1u;
    return total;
}

// ---- compressor: five launches (kernels.h CompDesc) ----
static int lower_comp(FxLevel& L, std::vector<size_t>& vs) {
    td_graph* g = L.g;
    const size_t M = L.M, sr = L.sr;
    const uint32_t n_tiles = (uint32_t)((M + kCompTile - 1) / kCompTile), chunk = (n_tiles + kThreads - 1) / kThreads;
    std::vector<CompDesc> d;
    std::vector<MasterDesc> c1, c2;
    const size_t n_plain = L.keyed_last(vs);   // (the keyed vertices behind the others: k_comp_detect<true> runs over those)
    for (size_t vi : vs) {
        Vertex& v = g->vertices[vi];
        CompDesc x{};
        x.x = L.tmp_buffer();
        x.dy = reinterpret_cast<double*>(L.tmp_buffer());   // (an edge buffer holds one double per frame)
        if (!x.x || !x.dy) return 0;
        L.head(x, vi);
        if (L.key_off.count(vi)) L.key_fields(x, vi);
        x.state = &g->dstate[v.state_slot].comp;
        x.n_tiles = n_tiles;
        x.thr = (double)v.fx.comp.threshold_db;
        x.slope = 1.0 - 1.0 / (double)v.fx.comp.ratio;
        x.knee = (double)v.fx.comp.knee_db;
        x.makeup = (double)v.fx.comp.makeup_db;
        x.aR = exp(-1.0 / ((double)v.fx.comp.release_ms * (double)sr / 1000.0));
        x.aA = v.fx.comp.attack_ms > 0.0f ? exp(-1.0 / ((double)v.fx.comp.attack_ms * (double)sr / 1000.0)) : 0.0;
        x.oA = 1.0 - x.aA;
        MasterDesc y1{}, yl{};
        y1.n_tiles = yl.n_tiles = n_tiles;
        y1.chunk = yl.chunk = chunk;
        yl.op = 1u;
        for (int j = 0; j < 8; ++j) {
            const double e = (double)(1u << j);
            x.pwR[j] = pow(x.aR, (double)kCompRun * e);
            x.pwA[j] = pow(x.aA, (double)kCompRun * e);
            y1.pwc[j] = pow(x.aR, (double)kCompTile * (double)chunk * e);
            yl.pwc[j] = pow(x.aA, (double)kCompTile * (double)chunk * e);
        }
        y1.a_tile = pow(x.aR, (double)kCompTile);
        yl.a_tile = pow(x.aA, (double)kCompTile);
        // (a set_time since the vertex last ran: the state restarts from (0, 0) -- consumed here, like a band-pass vertex' first_override)
        if (!v.first_pending) {
            y1.init = &g->dstate[v.state_slot].comp.y1;
            yl.init = &g->dstate[v.state_slot].comp.yL;
        }
        v.first_pending = false;
        d.push_back(x);
        c1.push_back(y1);
        c2.push_back(yl);
    }
    const size_t off = L.put(d, vs);
    const size_t o1 = L.cb.st->put(c1), o2 = L.cb.st->put(c2);
    for (size_t i = 0; i < vs.size(); ++i) {
        const size_t o = off + i * sizeof(CompDesc), tb = (size_t)n_tiles * sizeof(double);
        const size_t a1 = L.cb.scratch(tb), k1 = L.cb.scratch(tb), a2 = L.cb.scratch(tb), k2 = L.cb.scratch(tb);
        L.cb.scratch_field(o, offsetof(CompDesc, agg1), a1);
        L.cb.scratch_field(o, offsetof(CompDesc, carry1), k1);
        L.cb.scratch_field(o, offsetof(CompDesc, agg2), a2);
        L.cb.scratch_field(o, offsetof(CompDesc, carry2), k2);
        L.cb.scratch_field(o1 + i * sizeof(MasterDesc), offsetof(MasterDesc, agg), a1);
        L.cb.scratch_field(o1 + i * sizeof(MasterDesc), offsetof(MasterDesc, carry), k1);
        L.cb.scratch_field(o2 + i * sizeof(MasterDesc), offsetof(MasterDesc, agg), a2);
        L.cb.scratch_field(o2 + i * sizeof(MasterDesc), offsetof(MasterDesc, carry), k2);
        if (i >= n_plain) L.cb.ptr_field(o, offsetof(CompDesc, key_ins), L.key_off[vs[i]]);
    }
    if (n_plain) L.add_launch(F_COMP_DETECT, off, (int)n_plain, n_tiles);
    if (n_plain < vs.size()) L.add_launch(F_COMP_DETECT, off + n_plain * sizeof(CompDesc), (int)(vs.size() - n_plain), n_tiles | kKeyedBit);
    L.add_launch(F_COMP_CARRY1, o1, (int)vs.size(), 0u);
    L.add_launch(F_COMP_ENV, off, (int)vs.size(), n_tiles);
    L.add_launch(F_COMP_CARRY2, o2, (int)vs.size(), 0u);
    L.add_launch(F_COMP_APPLY, off, (int)vs.size(), n_tiles);
    return 1;
}
// (a keyed form: prepare_render has checked it exists where a key edge asks for it -- here and in the kinds below)
static void launch_comp(const Launch& L, const void* d, hipStream_t s) {
    switch (L.fam) {
        case F_COMP_DETECT: (L.aux & kKeyedBit ? launch_comp_detect_keyed : launch_comp_detect)((const CompDesc*)d, L.n, L.aux & ~kKeyedBit, s); break;
        case F_COMP_CARRY1:
        case F_COMP_CARRY2: launch_master_carry((const MasterDesc*)d, L.n, s); break;
        case F_COMP_ENV: launch_comp_env((const CompDesc*)d, L.n, L.aux, s); break;
        case F_COMP_APPLY: launch_comp_apply((const CompDesc*)d, L.n, L.aux, s); break;
    }
}

// ---- EQ: three launches (kernels.h EqDesc) ----
static int lower_eq(FxLevel& L, std::vector<size_t>& vs) {
    td_graph* g = L.g;
    const uint32_t n_tiles = (uint32_t)((L.M + kEqTile - 1) / kEqTile), chunk = (n_tiles + kThreads - 1) / kThreads;
    std::vector<EqDesc> d;
    for (size_t vi : vs) {
        Vertex& v = g->vertices[vi];
        EqDesc x{};
        x.x = L.tmp_buffer();
        if (!x.x) return 0;
        L.head(x, vi);
        x.state = &g->dstate[v.state_slot].eq;
        // (a set_time since the vertex last ran: the state restarts from zero -- consumed here, like a compressor's)
        x.init = v.first_pending ? nullptr : x.state;
        v.first_pending = false;
        x.n_tiles = n_tiles;
        x.chunk = chunk;
        double c[5];
        eq::coefficients(v.fx.eq.kind, L.sr, v.fx.eq.freq_hz, v.fx.eq.q, v.fx.eq.gain_db, c);
        x.b0 = c[0]; x.b1 = c[1]; x.b2 = c[2]; x.a1 = c[3]; x.a2 = c[4];
        x.c0 = x.b1 - x.a1 * x.b0;
        x.c1 = x.b2 - x.a2 * x.b0;
        eq::powers(x.a1, x.a2, kEqRun, chunk, x.pw, x.a_tile, x.pwc);
        d.push_back(x);
    }
    const size_t off = L.put(d, vs);
    for (size_t i = 0; i < vs.size(); ++i) {
        const size_t o = off + i * sizeof(EqDesc), tb = (size_t)n_tiles * 4 * sizeof(double);
        L.cb.scratch_field(o, offsetof(EqDesc, agg), L.cb.scratch(tb));
        L.cb.scratch_field(o, offsetof(EqDesc, carry), L.cb.scratch(tb));
    }
    L.add_launch(F_EQ_LOCAL, off, (int)vs.size(), n_tiles);
    L.add_launch(F_EQ_CARRY, off, (int)vs.size(), 0u);
    L.add_launch(F_EQ_APPLY, off, (int)vs.size(), n_tiles);
    return 1;
}
static void launch_eq(const Launch& L, const void* d, hipStream_t s) {
    switch (L.fam) {
        case F_EQ_LOCAL: launch_eq_local((const EqDesc*)d, L.n, L.aux, s); break;
        case F_EQ_CARRY: launch_eq_carry((const EqDesc*)d, L.n, s); break;
        case F_EQ_APPLY: launch_eq_apply((const EqDesc*)d, L.n, L.aux, s); break;
    }
}

// ---- delay (kernels.h DelayDesc) ----
static int lower_delay(FxLevel& L, std::vector<size_t>& vs) {
    td_graph* g = L.g;
    const size_t M = L.M;
    const uint32_t T = g->delay_tile;
    struct Plan { size_t vi; uint32_t D; delay::Tiling t; double c[4]; };
    std::vector<Plan> plans;
    for (size_t vi : vs) {
        const Vertex& v = g->vertices[vi];
        Plan p{};
        p.vi = vi;
        delay::params(L.sr, v.fx.delay.time_ms, v.fx.delay.feedback, v.fx.delay.cross, p.c);
        p.D = (uint32_t)p.c[0];
        p.t = delay::tiling(M, p.D, T);
        if ((uint64_t)M + (uint64_t)(T + 4u) * p.D > 0xFFFF0000ull) return fail("delay: chunk too long");
        plans.push_back(p);
    }
    // the vertices whose chunk takes more than one tile first: k_delay_local and k_delay_carry run over those only
    std::stable_sort(plans.begin(), plans.end(), [](const Plan& a, const Plan& b) { return (a.t.n_tiles > 1u) > (b.t.n_tiles > 1u); });
    std::vector<DelayDesc> d;
    std::vector<size_t> ord;
    int n_multi = 0;
    uint32_t g_local = 0, g_carry = 0, g_apply = 0, g_single = 0;
    for (const Plan& p : plans) {
        Vertex& v = g->vertices[p.vi];
        const bool multi = p.t.n_tiles > 1u;
        DelayDesc x{};
        if (multi && !(x.x = L.tmp_buffer())) return 0;
        L.head(x, p.vi);
        x.line = (double*)take_line(g, v, (size_t)p.D * 2 * sizeof(double));
        if (!x.line) return fail("termdaw_amd: out of device memory for a delay line");
        const uint64_t total = enter_chunk(v, M, false);
        x.D = p.D;
        x.lanes = p.t.lanes;
        x.T = T;
        x.n_tiles = p.t.n_tiles;
        x.pos = (uint32_t)(total % p.D);
        x.filled = (uint32_t)std::min<uint64_t>(total, p.D);
        x.seg = p.t.seg;
        x.chunk = p.t.chunk;
        x.gs = p.c[1];
        x.gc = p.c[2];
        delay::powers(x.gs, x.gc, T, x.chunk, x.g_tile, x.pwc);
        const uint32_t groups = (uint32_t)(((uint64_t)x.n_tiles * x.lanes + kThreads - 1) / kThreads);
        (multi ? g_apply : g_single) = std::max(multi ? g_apply : g_single, groups);
        if (multi) {
            ++n_multi;
            g_local = std::max(g_local, groups);
            const uint32_t lw = (uint32_t)kThreads / x.seg;
            g_carry = std::max(g_carry, (x.lanes + lw - 1) / lw);
        }
        d.push_back(x);
        ord.push_back(p.vi);
    }
    const size_t off = L.put(d, ord);
    for (size_t i = 0; i < plans.size(); ++i) {
        if (plans[i].t.n_tiles <= 1u) continue;
        const size_t o = off + i * sizeof(DelayDesc), tb = (size_t)plans[i].t.n_tiles * plans[i].t.lanes * 2 * sizeof(double);
        L.cb.scratch_field(o, offsetof(DelayDesc, agg), L.cb.scratch(tb));
        L.cb.scratch_field(o, offsetof(DelayDesc, carry), L.cb.scratch(tb));
    }
    if (n_multi) {
        L.add_launch(F_DELAY_LOCAL, off, n_multi, g_local);
        L.add_launch(F_DELAY_CARRY, off, n_multi, g_carry);
    }
    // (k_delay_apply's two instantiations: the multi-tile vertices stream their scratch buffer, the others run the term loop)
    if (n_multi) L.add_launch(F_DELAY_APPLY, off, n_multi, g_apply);
    if ((size_t)n_multi < plans.size())
        L.add_launch(F_DELAY_APPLY, off + (size_t)n_multi * sizeof(DelayDesc), (int)plans.size() - n_multi, g_single | kDelaySingleBit);
    return 1;
}
static void launch_delay(const Launch& L, const void* d, hipStream_t s) {
    switch (L.fam) {
        case F_DELAY_LOCAL: launch_delay_local((const DelayDesc*)d, L.n, L.aux, s); break;
        case F_DELAY_CARRY: launch_delay_carry((const DelayDesc*)d, L.n, L.aux, s); break;
        case F_DELAY_APPLY: launch_delay_apply((const DelayDesc*)d, L.n, L.aux & ~kDelaySingleBit, (L.aux & kDelaySingleBit) != 0u, s); break;
    }
}

// ---- saturator (kernels.h SatDesc): the vertices with R > 1 (L.fam == F_SAT_SUM) or those with R = 1 (F_SAT1) ----
static int lower_sat(FxLevel& L, std::vector<size_t>& vs) {
    td_graph* g = L.g;
    const size_t M = L.M;
    const uint32_t F = g->sat_tile, n_tiles = (uint32_t)((M + F - 1) / F);
    const bool filtered = L.fam != F_SAT1, multi = filtered && M > (size_t)kSatInlineFrames;   // (multi: k_sat_sum first)
    std::vector<size_t> ord(vs.begin(), vs.end());   // one k_sat launch per oversampling factor
    std::stable_sort(ord.begin(), ord.end(), [&](size_t a, size_t b) { return g->vertices[a].fx.sat.oversample < g->vertices[b].fx.sat.oversample; });
    std::vector<SatDesc> d;
    std::map<int, size_t> taps_off;
    for (size_t vi : ord) {
        Vertex& v = g->vertices[vi];
        double c[6];
        sat::params(v.fx.sat.kind, v.fx.sat.oversample, v.fx.sat.drive_db, v.fx.sat.bias, v.fx.sat.out_db, c);
        SatDesc x{};
        if (multi && !(x.x = L.tmp_buffer())) return 0;
        L.head(x, vi);
        if (filtered) {
            x.line = (float2*)take_line(g, v, 2 * sat::kLine * sizeof(float2));
            if (!x.line) return fail("termdaw_amd: out of device memory for a saturator line");
            x.parity = v.line.parity;
            x.filled = (uint32_t)std::min<uint64_t>(enter_chunk(v, M, true), sat::kLine);
            if (!taps_off.count(v.fx.sat.oversample)) taps_off[v.fx.sat.oversample] = L.cb.st->put(sat::taps(v.fx.sat.oversample));
        }
        v.first_pending = false;   // (R = 1 has no line: the set_time is consumed all the same)
        x.F = F;
        x.n_tiles = n_tiles;
        x.kind = (uint32_t)v.fx.sat.kind;
        x.g_in = c[0];
        x.g_out = c[1];
        x.bias = (double)v.fx.sat.bias;
        x.fb = c[2];
        d.push_back(x);
    }
    const size_t off = L.put(d, ord);
    if (!filtered) {
        L.add_launch(F_SAT1, off, (int)ord.size(), 0);
        return 1;
    }
    for (size_t i = 0; i < ord.size(); ++i)
        L.cb.ptr_field(off + i * sizeof(SatDesc), offsetof(SatDesc, taps), taps_off[g->vertices[ord[i]].fx.sat.oversample]);
    if (multi) L.add_launch(F_SAT_SUM, off, (int)ord.size(), 0);
    for (size_t i = 0; i < ord.size();) {
        const int R = g->vertices[ord[i]].fx.sat.oversample;
        size_t j = i;
        while (j < ord.size() && g->vertices[ord[j]].fx.sat.oversample == R) ++j;
        L.add_launch(F_SAT, off + i * sizeof(SatDesc), (int)(j - i), sat_aux(n_tiles, F, (uint32_t)R, !multi));
        i = j;
    }
    return 1;
}
static void launch_sat_kind(const Launch& L, const void* d, hipStream_t s) {
    switch (L.fam) {
        case F_SAT_SUM: launch_sat_sum((const SatDesc*)d, L.n, L.M, s); break;
        case F_SAT: launch_sat((const SatDesc*)d, L.n, (L.aux >> 24) & 15u, L.aux & 0xFFFFFu, ((L.aux >> 20) & 15u) * 128u, (L.aux & kSatTermsBit) != 0u, s); break;
        case F_SAT1: launch_sat1((const SatDesc*)d, L.n, L.M, s); break;
    }
}

// ---- chorus (kernels.h ChorusDesc) ----
static int lower_chorus(FxLevel& L, std::vector<size_t>& vs) {
    td_graph* g = L.g;
    const size_t M = L.M;
    const uint32_t F = g->chorus_tile, n_tiles = (uint32_t)((M + F - 1) / F);
    const bool multi = M > (size_t)kSatInlineFrames;   // (multi: k_chorus_sum first)
    std::vector<ChorusDesc> d;
    for (size_t vi : vs) {
        Vertex& v = g->vertices[vi];
        double c[6];
        chorus::params(L.sr, v.fx.chorus.voices, v.fx.chorus.delay_ms, v.fx.chorus.depth_ms, v.fx.chorus.rate_hz, v.fx.chorus.stereo, v.fx.chorus.shape, c);
        ChorusDesc x{};
        if (multi && !(x.x = L.tmp_buffer())) return 0;
        L.head(x, vi);
        x.H = (uint32_t)c[3];
        x.line = (float2*)take_line(g, v, 2 * (size_t)x.H * sizeof(float2));
        if (!x.line) return fail("termdaw_amd: out of device memory for a chorus line");
        x.parity = v.line.parity;
        x.filled = (uint32_t)std::min<uint64_t>(enter_chunk(v, M, true), x.H);
        x.t0 = L.t0;
        x.F = F;
        x.n_tiles = n_tiles;
        x.voices = (uint32_t)v.fx.chorus.voices;
        x.shape = (uint32_t)v.fx.chorus.shape;
        x.D0 = c[0];
        x.A = c[1];
        x.f = c[2];
        x.stereo = (double)v.fx.chorus.stereo;
        x.inv_v = 1.0 / (double)v.fx.chorus.voices;
        d.push_back(x);
    }
    const size_t off = L.put(d, vs);
    if (multi) L.add_launch(F_CHORUS_SUM, off, (int)vs.size(), 0);
    L.add_launch(F_CHORUS, off, (int)vs.size(), chorus_aux(n_tiles, !multi));
    return 1;
}
static void launch_chorus_kind(const Launch& L, const void* d, hipStream_t s) {
    if (L.fam == F_CHORUS_SUM) launch_chorus_sum((const ChorusDesc*)d, L.n, L.M, s);
    else launch_chorus((const ChorusDesc*)d, L.n, L.aux & 0xFFFFFu, L.M, (L.aux & kChorusTermsBit) != 0u, s);
}

// ---- reverb (kernels.h ReverbDesc) ----
static int lower_reverb(FxLevel& L, std::vector<size_t>& vs) {
    td_graph* g = L.g;
    std::vector<ReverbDesc> d;
    for (size_t vi : vs) {
        Vertex& v = g->vertices[vi];
        double c[reverb::kParams];
        reverb::params(L.sr, v.fx.reverb.room, v.fx.reverb.damp, v.fx.reverb.width, v.fx.reverb.size, c);
        ReverbDesc x{};
        x.x = L.tmp_buffer();
        if (!x.x) return 0;
        L.head(x, vi);
        uint32_t at = 16, shortest = 0xFFFFFFFFu;
        for (int i = 0; i < reverb::kLines; ++i) {
            x.len[i] = (uint32_t)c[7 + i];
            x.off[i] = at;
            at += x.len[i];
            shortest = std::min(shortest, x.len[i]);
        }
        x.state = (double*)take_line(g, v, at * sizeof(double));
        if (!x.state) return fail("termdaw_amd: out of device memory for a reverb vertex' lines");
        const uint64_t total = enter_chunk(v, L.M, false);
        for (int i = 0; i < reverb::kLines; ++i) {
            const uint32_t D = x.len[i];
            x.pos[i] = (uint32_t)(total % D);
            x.skip[i] = total < D ? (uint32_t)(D - total) : 0u;
        }
        x.fresh = total == 0 ? 1u : 0u;
        x.B = reverb::window(shortest, g->reverb_block);
        x.g = c[0];
        x.d1 = c[1];
        x.d2 = c[2];
        x.w1 = c[3];
        x.w2 = c[4];
        reverb::powers(x.d1, x.B / 64u, x.pw);
        d.push_back(x);
    }
    const size_t off = L.put(d, vs);
    L.add_launch(F_REVERB_SUM, off, (int)vs.size(), 0);
    L.add_launch(F_REVERB, off, (int)vs.size(), g->reverb_form);
    return 1;
}
static void launch_reverb_kind(const Launch& L, const void* d, hipStream_t s) {
    if (L.fam == F_REVERB_SUM) launch_reverb_sum((const ReverbDesc*)d, L.n, L.M, s);
    else launch_reverb((const ReverbDesc*)d, L.n, L.aux, s);
}

// ---- gate: five launches (kernels.h GateDesc) ----
static int lower_gate(FxLevel& L, std::vector<size_t>& vs) {
    td_graph* g = L.g;
    const uint32_t n_tiles = (uint32_t)((L.M + kGateTile - 1) / kGateTile), chunk = (n_tiles + kThreads - 1) / kThreads;
    std::vector<GateDesc> d;
    const size_t n_plain = L.keyed_last(vs);   // (the keyed vertices behind the others: k_gate_detect<true> / k_gate_env<true> run over those)
    for (size_t vi : vs) {
        Vertex& v = g->vertices[vi];
        GateDesc x{};
        x.x = L.tmp_buffer();
        if (!x.x) return 0;
        L.head(x, vi);
        if (L.key_off.count(vi)) L.key_fields(x, vi);
        x.state = &g->dstate[v.state_slot].gate;
        // (a set_time since the vertex last ran: the state restarts closed -- consumed here, like a compressor's)
        x.init = v.first_pending ? nullptr : x.state;
        v.first_pending = false;
        x.n_tiles = n_tiles;
        x.chunk = chunk;
        double c[6];
        gate::params(L.sr, v.fx.gate.threshold_db, v.fx.gate.hysteresis_db, v.fx.gate.hold_ms, v.fx.gate.attack_ms, v.fx.gate.release_ms, v.fx.gate.range_db, c);
        if (!(c[2] <= gate::kMaxHold)) return fail("gate: hold_ms is too many frames at this sample rate");
        x.To = c[0];
        x.Tc = c[1];
        x.cap = (uint32_t)c[2] + 1u;
        x.aA = c[3];
        x.aR = c[4];
        x.oA = 1.0 - x.aA;
        x.oR = 1.0 - x.aR;
        x.F = c[5];
        x.oF = 1.0 - x.F;
        d.push_back(x);
    }
    const size_t off = L.put(d, vs);
    for (size_t i = 0; i < vs.size(); ++i) {
        const size_t o = off + i * sizeof(GateDesc), tb = (size_t)n_tiles * sizeof(double);
        L.cb.scratch_field(o, offsetof(GateDesc, map), L.cb.scratch(tb));
        L.cb.scratch_field(o, offsetof(GateDesc, carry_hc), L.cb.scratch((size_t)n_tiles * sizeof(uint32_t)));
        L.cb.scratch_field(o, offsetof(GateDesc, tbits), L.cb.scratch((size_t)n_tiles * kThreads));
        L.cb.scratch_field(o, offsetof(GateDesc, aggA), L.cb.scratch(tb));
        L.cb.scratch_field(o, offsetof(GateDesc, aggB), L.cb.scratch(tb));
        L.cb.scratch_field(o, offsetof(GateDesc, carry_env), L.cb.scratch(tb));
        if (i >= n_plain) {   // a keyed vertex: its key terms, and the lanes' class words between detect and env
            L.cb.ptr_field(o, offsetof(GateDesc, key_ins), L.key_off[vs[i]]);
            L.cb.scratch_field(o, offsetof(GateDesc, cls), L.cb.scratch((size_t)n_tiles * kThreads * sizeof(uint16_t)));
        }
    }
    const size_t off_k = off + n_plain * sizeof(GateDesc);
    const int n_keyed = (int)(vs.size() - n_plain);
    if (n_plain) L.add_launch(F_GATE_DETECT, off, (int)n_plain, n_tiles);
    if (n_keyed) L.add_launch(F_GATE_DETECT, off_k, n_keyed, n_tiles | kKeyedBit);
    L.add_launch(F_GATE_CARRY_H, off, (int)vs.size(), 0u);
    if (n_plain) L.add_launch(F_GATE_ENV, off, (int)n_plain, n_tiles);
    if (n_keyed) L.add_launch(F_GATE_ENV, off_k, n_keyed, n_tiles | kKeyedBit);
    L.add_launch(F_GATE_CARRY_ENV, off, (int)vs.size(), 0u);
    L.add_launch(F_GATE_APPLY, off, (int)vs.size(), n_tiles);
    return 1;
}
static void launch_gate(const Launch& L, const void* d, hipStream_t s) {
    switch (L.fam) {
        case F_GATE_DETECT: (L.aux & kKeyedBit ? launch_gate_detect_keyed : launch_gate_detect)((const GateDesc*)d, L.n, L.aux & ~kKeyedBit, s); break;
        case F_GATE_CARRY_H: launch_gate_carry((const GateDesc*)d, L.n, false, s); break;
        case F_GATE_ENV: (L.aux & kKeyedBit ? launch_gate_env_keyed : launch_gate_env)((const GateDesc*)d, L.n, L.aux & ~kKeyedBit, s); break;
        case F_GATE_CARRY_ENV: launch_gate_carry((const GateDesc*)d, L.n, true, s); break;
        case F_GATE_APPLY: launch_gate_apply((const GateDesc*)d, L.n, L.aux, s); break;
    }
}
// A gate vertex' state at time 0: closed, the hold run out -- (env, h, c) = (0, 0, H + 1)
static void rest_gate(const td_graph* g, const Vertex& v, StateSlot* run) {
    double c[6];
    gate::params(g->sr, v.fx.gate.threshold_db, v.fx.gate.hysteresis_db, v.fx.gate.hold_ms, v.fx.gate.attack_ms, v.fx.gate.release_ms, v.fx.gate.range_db, c);
    run->gate = {0.0, 0u, (uint32_t)std::min(c[2] + 1.0, gate::kMaxHold + 1.0), {0, 0, 0, 0}};
}

// ---- phaser: three launches per stage count, or one (kernels.h PhaserDesc) ----
static int lower_phaser(FxLevel& L, std::vector<size_t>& vs) {
    td_graph* g = L.g;
    const uint32_t n_tiles = (uint32_t)((L.M + kPhaserTile - 1) / kPhaserTile);
    const bool multi = n_tiles > 1u;   // (multi: k_phaser_local and k_phaser_carry first)
    std::vector<size_t> ord(vs.begin(), vs.end());   // one launch per stage count: the kernels are templates on it
    std::stable_sort(ord.begin(), ord.end(), [&](size_t a, size_t b) { return g->vertices[a].fx.phaser.stages < g->vertices[b].fx.phaser.stages; });
    std::vector<PhaserDesc> d;
    for (size_t vi : ord) {
        Vertex& v = g->vertices[vi];
        PhaserDesc x{};
        if (multi && !(x.x = L.tmp_buffer())) return 0;
        L.head(x, vi);
        x.state = reinterpret_cast<PhaserState*>(&g->dstate[v.state_slot]);
        // (a set_time since the vertex last ran: the state restarts from zero -- consumed here, like an EQ's)
        x.init = v.first_pending ? nullptr : x.state;
        v.first_pending = false;
        x.t0 = L.t0;
        x.n_tiles = n_tiles;
        double c[phaser::kParams];
        phaser::params(L.sr, v.fx.phaser.stages, v.fx.phaser.lo_hz, v.fx.phaser.hi_hz, v.fx.phaser.rate_hz, v.fx.phaser.feedback, v.fx.phaser.stereo, v.fx.phaser.shape, c);
        x.stages = (uint32_t)v.fx.phaser.stages;
        x.shape = (uint32_t)v.fx.phaser.shape;
        x.am = c[3];
        x.ad = c[4];
        x.f = c[5];
        x.fb = c[6];
        x.stereo = (double)v.fx.phaser.stereo;
        d.push_back(x);
    }
    const size_t off = L.put(d, ord);
    for (size_t i = 0; multi && i < ord.size(); ++i) {
        const size_t o = off + i * sizeof(PhaserDesc), D = (size_t)d[i].stages + 1;
        L.cb.scratch_field(o, offsetof(PhaserDesc, agg), L.cb.scratch((size_t)n_tiles * 2 * D * (D + 1) * sizeof(double)));
        L.cb.scratch_field(o, offsetof(PhaserDesc, carry), L.cb.scratch((size_t)n_tiles * 2 * D * sizeof(double)));
    }
    for (size_t i = 0; i < ord.size();) {
        const uint32_t N = d[i].stages;
        size_t j = i;
        while (j < ord.size() && d[j].stages == N) ++j;
        const size_t o = off + i * sizeof(PhaserDesc);
        if (multi) {
            L.add_launch(F_PHASER_LOCAL, o, (int)(j - i), phaser_aux(n_tiles, N, false));
            L.add_launch(F_PHASER_CARRY, o, (int)(j - i), phaser_aux(0u, N, false));
        }
        L.add_launch(F_PHASER_APPLY, o, (int)(j - i), phaser_aux(n_tiles, N, !multi));
        i = j;
    }
    return 1;
}
static void launch_phaser(const Launch& L, const void* d, hipStream_t s) {
    const uint32_t N = (L.aux >> 24) & 15u, n_tiles = L.aux & 0xFFFFFFu;
    switch (L.fam) {
        case F_PHASER_LOCAL: launch_phaser_local((const PhaserDesc*)d, L.n, N, n_tiles, s); break;
        case F_PHASER_CARRY: launch_phaser_carry((const PhaserDesc*)d, L.n, N, s); break;
        case F_PHASER_APPLY: launch_phaser_apply((const PhaserDesc*)d, L.n, N, n_tiles, (L.aux & kPhaserSingleBit) != 0u, s); break;
    }
}

// ---- vocoder: five launches per band count and key form, or one (kernels.h VocDesc) ----
static int lower_vocoder(FxLevel& L, std::vector<size_t>& vs) {
    td_graph* g = L.g;
    const uint32_t n_tiles = (uint32_t)((L.M + kVocTile - 1) / kVocTile), chunk = (n_tiles + kThreads - 1) / kThreads;
    const bool multi = n_tiles > 1u;   // (multi: the four launches in front of k_voc_apply)
    // the keyed vertices behind the others (FxLevel::keyed_last), each group by band count: the kernels are templates on it
    std::vector<size_t> ord(vs.begin(), vs.end());
    const size_t n_plain = L.keyed_last(ord);
    auto by_bands = [&](size_t a, size_t b) { return g->vertices[a].fx.vocoder.bands < g->vertices[b].fx.vocoder.bands; };
    std::stable_sort(ord.begin(), ord.begin() + (long)n_plain, by_bands);
    std::stable_sort(ord.begin() + (long)n_plain, ord.end(), by_bands);
    std::vector<VocDesc> d;
    std::vector<size_t> band_off;
    for (size_t i = 0; i < ord.size(); ++i) {
        const size_t vi = ord[i];
        Vertex& v = g->vertices[vi];
        const bool keyed = i >= n_plain;
        const int B = v.fx.vocoder.bands;
        VocDesc x{};
        if (multi) {
            if (!(x.x = L.tmp_buffer())) return 0;
            x.kx = x.x;   // (an unkeyed vertex listens to itself)
            if (keyed && !(x.kx = L.tmp_buffer())) return 0;
        }
        L.head(x, vi);
        if (keyed) L.key_fields(x, vi);
        x.line = (double*)take_line(g, v, (size_t)B * kVocState * sizeof(double));
        if (!x.line) return fail("termdaw_amd: out of device memory for a vocoder vertex' state");
        x.init = enter_chunk(v, L.M, false) ? x.line : nullptr;   // (afresh: the state is zero, the line is not read)
        x.n_tiles = n_tiles;
        x.chunk = chunk;
        x.bands = (uint32_t)B;
        double c[vocoder::kMaxParams];
        vocoder::params(L.sr, B, v.fx.vocoder.lo_hz, v.fx.vocoder.hi_hz, v.fx.vocoder.q, v.fx.vocoder.response_ms, v.fx.vocoder.out_db, c);
        std::vector<VocBand> bands((size_t)B);
        for (int b = 0; b < B; ++b) {
            VocBand& y = bands[(size_t)b];
            const double* cb = c + vocoder::kBandParams * b + 1;
            y.b0 = cb[0]; y.b1 = cb[1]; y.b2 = cb[2]; y.a1 = cb[3]; y.a2 = cb[4];
            y.c0 = y.b1 - y.a1 * y.b0;
            y.c1 = y.b2 - y.a2 * y.b0;
            y.pad = 0.0;
            eq::powers(y.a1, y.a2, kVocRun, chunk, y.pw, y.a_tile, y.pwc);
        }
        band_off.push_back(L.cb.st->put(bands));
        x.a = c[vocoder::kBandParams * B];
        x.oa = 1.0 - x.a;
        x.g = c[vocoder::kBandParams * B + 1];
        // the follower's powers, in long double like the matrices', each rounded once
        long double p = powl((long double)x.a, (long double)kVocRun);
        for (int k = 0; k < 8; ++k) { x.pwa[k] = (double)p; p *= p; }
        x.a_tile = (double)p;
        p = powl(p, (long double)chunk);
        for (int k = 0; k < 8; ++k) { x.pwac[k] = (double)p; p *= p; }
        d.push_back(x);
    }
    const size_t off = L.put(d, ord);
    for (size_t i = 0; i < ord.size(); ++i) {
        const size_t o = off + i * sizeof(VocDesc), B = d[i].bands;
        L.cb.ptr_field(o, offsetof(VocDesc, band), band_off[i]);
        if (i >= n_plain) L.cb.ptr_field(o, offsetof(VocDesc, key_ins), L.key_off[ord[i]]);
        if (!multi) continue;
        L.cb.scratch_field(o, offsetof(VocDesc, agg), L.cb.scratch((size_t)n_tiles * B * 6 * sizeof(double)));
        L.cb.scratch_field(o, offsetof(VocDesc, carry), L.cb.scratch((size_t)n_tiles * B * 6 * sizeof(double)));
        L.cb.scratch_field(o, offsetof(VocDesc, agge), L.cb.scratch((size_t)n_tiles * B * sizeof(double)));
        L.cb.scratch_field(o, offsetof(VocDesc, carrye), L.cb.scratch((size_t)n_tiles * B * sizeof(double)));
    }
    for (size_t i = 0; i < ord.size();) {
        const uint32_t B = d[i].bands;
        const bool keyed = i >= n_plain;
        size_t j = i;
        while (j < ord.size() && d[j].bands == B && (j >= n_plain) == keyed) ++j;
        const size_t o = off + i * sizeof(VocDesc);
        const int n = (int)(j - i);
        if (multi) {   // (only k_voc_local has a keyed form here: the later launches read x and kx)
            L.add_launch(F_VOC_LOCAL, o, n, voc_aux(n_tiles, B, false, keyed));
            L.add_launch(F_VOC_CARRY, o, n, voc_aux(0u, B, false, false));
            L.add_launch(F_VOC_ENV, o, n, voc_aux(n_tiles, B, false, false));
            L.add_launch(F_VOC_CARRY_ENV, o, n, voc_aux(0u, B, false, false));
            L.add_launch(F_VOC_APPLY, o, n, voc_aux(n_tiles, B, false, false));
        } else {
            L.add_launch(F_VOC_APPLY, o, n, voc_aux(n_tiles, B, true, keyed));
        }
        i = j;
    }
    return 1;
}
static void launch_vocoder(const Launch& L, const void* d, hipStream_t s) {
    const uint32_t B = voc_aux_bands(L.aux), n_tiles = voc_aux_tiles(L.aux);
    switch (L.fam) {
        case F_VOC_LOCAL: (L.aux & kKeyedBit ? launch_voc_local_keyed : launch_voc_local)((const VocDesc*)d, L.n, B, n_tiles, s); break;
        case F_VOC_CARRY: launch_voc_carry((const VocDesc*)d, L.n, B, false, s); break;
        case F_VOC_ENV: launch_voc_env((const VocDesc*)d, L.n, B, n_tiles, s); break;
        case F_VOC_CARRY_ENV: launch_voc_carry((const VocDesc*)d, L.n, B, true, s); break;
        case F_VOC_APPLY:
            if (L.aux & kKeyedBit) launch_voc_apply_keyed((const VocDesc*)d, L.n, B, n_tiles, s);
            else launch_voc_apply((const VocDesc*)d, L.n, B, n_tiles, (L.aux & kVocSingleBit) != 0u, s);
            break;
    }
}

// ---- filter: the follower's four launches, then three, or one (kernels.h FiltDesc) ----
static int lower_filter(FxLevel& L, std::vector<size_t>& vs) {
    td_graph* g = L.g;
    const uint32_t n_tiles = (uint32_t)((L.M + kFiltTile - 1) / kFiltTile), chunk = (n_tiles + kThreads - 1) / kThreads;
    const bool multi = n_tiles > 1u;   // (multi: the six launches in front of k_filt_apply)
    // the vertices whose follower does not run first, then those that listen to themselves, the keyed ones last (a vertex with
    // env_oct == 0 has no entry in key_off: Vertex::reads_key)
    std::vector<size_t> ord;
    for (size_t vi : vs)
        if (!g->vertices[vi].filt_follows()) ord.push_back(vi);
    const size_t n_still = ord.size();
    for (size_t vi : vs)
        if (g->vertices[vi].filt_follows() && !L.key_off.count(vi)) ord.push_back(vi);
    const size_t n_plain = ord.size();
    for (size_t vi : vs)
        if (g->vertices[vi].filt_follows() && L.key_off.count(vi)) ord.push_back(vi);
    const size_t n_all = ord.size(), n_env = n_all - n_still;
    std::vector<FiltDesc> d;
    std::vector<MasterDesc> c1, c2;
    for (size_t i = 0; i < n_all; ++i) {
        const size_t vi = ord[i];
        Vertex& v = g->vertices[vi];
        FiltDesc x{};
        if (multi) {
            if (!(x.x = L.tmp_buffer())) return 0;
            if (i >= n_still && !(x.lv = reinterpret_cast<double*>(L.tmp_buffer()))) return 0;   // (an edge buffer holds one double per frame)
        }
        L.head(x, vi);
        if (i >= n_plain) L.key_fields(x, vi);
        x.state = reinterpret_cast<FiltState*>(&g->dstate[v.state_slot]);
        // (a set_time since the vertex last ran: the state restarts from zero -- consumed here, like an EQ's)
        x.init = v.first_pending ? nullptr : x.state;
        v.first_pending = false;
        x.t0 = L.t0;
        x.n_tiles = n_tiles;
        double c[filter::kParams];
        filter::params(L.sr, v.fx.filter.kind, v.fx.filter.freq_hz, v.fx.filter.q, v.fx.filter.lfo_oct, v.fx.filter.rate_hz, v.fx.filter.stereo, v.fx.filter.shape,
                       v.fx.filter.env_oct, v.fx.filter.sens_db, v.fx.filter.attack_ms, v.fx.filter.release_ms, c);
        x.kind = (uint32_t)v.fx.filter.kind;
        x.shape = (uint32_t)v.fx.filter.shape;
        x.env = i >= n_still ? 1u : 0u;
        x.g0 = c[0]; x.kq = c[1]; x.gmin = c[2]; x.gmax = c[3]; x.cl = c[4]; x.ce = c[5]; x.f = c[6];
        x.stereo = (double)v.fx.filter.stereo;
        x.S = c[7]; x.aA = c[8]; x.oA = c[9]; x.aR = c[10];
        for (int j = 0; j < 8; ++j) {
            const double e = (double)(1u << j);
            x.pwR[j] = pow(x.aR, (double)kFiltRun * e);
            x.pwA[j] = pow(x.aA, (double)kFiltRun * e);
        }
        d.push_back(x);
        if (!multi || i < n_still) continue;
        MasterDesc y1{}, ye{};
        y1.n_tiles = ye.n_tiles = n_tiles;
        y1.chunk = ye.chunk = chunk;
        ye.op = 1u;
        for (int j = 0; j < 8; ++j) {
            const double e = (double)(1u << j);
            y1.pwc[j] = pow(x.aR, (double)kFiltTile * (double)chunk * e);
            ye.pwc[j] = pow(x.aA, (double)kFiltTile * (double)chunk * e);
        }
        y1.a_tile = pow(x.aR, (double)kFiltTile);
        ye.a_tile = pow(x.aA, (double)kFiltTile);
        if (x.init) {
            y1.init = &x.state->y1;
            ye.init = &x.state->e;
        }
        c1.push_back(y1);
        c2.push_back(ye);
    }
    const size_t off = L.put(d, ord);
    for (size_t i = n_plain; i < n_all; ++i) L.cb.ptr_field(off + i * sizeof(FiltDesc), offsetof(FiltDesc, key_ins), L.key_off[ord[i]]);
    const size_t off_e = off + n_still * sizeof(FiltDesc), off_k = off + n_plain * sizeof(FiltDesc);
    const int n_keyed = (int)(n_all - n_plain), n_self = (int)(n_plain - n_still);
    if (!multi) {
        if (n_plain) L.add_launch(F_FILT_APPLY, off, (int)n_plain, filt_aux(n_tiles, true, false));
        if (n_keyed) L.add_launch(F_FILT_APPLY, off_k, n_keyed, filt_aux(n_tiles, true, true));
        return 1;
    }
    const size_t o1 = n_env ? L.cb.st->put(c1) : 0, o2 = n_env ? L.cb.st->put(c2) : 0;
    for (size_t i = 0; i < n_all; ++i) {
        const size_t o = off + i * sizeof(FiltDesc), tb = (size_t)n_tiles * sizeof(double);
        L.cb.scratch_field(o, offsetof(FiltDesc, agg), L.cb.scratch(12 * tb));
        L.cb.scratch_field(o, offsetof(FiltDesc, carry), L.cb.scratch(4 * tb));
        if (i < n_still) continue;
        const size_t m1 = o1 + (i - n_still) * sizeof(MasterDesc), m2 = o2 + (i - n_still) * sizeof(MasterDesc);
        const size_t a1 = L.cb.scratch(tb), k1 = L.cb.scratch(tb), a2 = L.cb.scratch(tb), k2 = L.cb.scratch(tb);
        L.cb.scratch_field(o, offsetof(FiltDesc, agg1), a1);
        L.cb.scratch_field(o, offsetof(FiltDesc, carry1), k1);
        L.cb.scratch_field(o, offsetof(FiltDesc, agg2), a2);
        L.cb.scratch_field(o, offsetof(FiltDesc, carry2), k2);
        L.cb.scratch_field(m1, offsetof(MasterDesc, agg), a1);
        L.cb.scratch_field(m1, offsetof(MasterDesc, carry), k1);
        L.cb.scratch_field(m2, offsetof(MasterDesc, agg), a2);
        L.cb.scratch_field(m2, offsetof(MasterDesc, carry), k2);
    }
    if (n_self) L.add_launch(F_FILT_DETECT, off_e, n_self, filt_aux(n_tiles, false, false));
    if (n_keyed) L.add_launch(F_FILT_DETECT, off_k, n_keyed, filt_aux(n_tiles, false, true));
    if (n_env) {
        L.add_launch(F_FILT_CARRY1, o1, (int)n_env, 0u);
        L.add_launch(F_FILT_ENV, off_e, (int)n_env, filt_aux(n_tiles, false, false));
        L.add_launch(F_FILT_CARRY2, o2, (int)n_env, 0u);
    }
    L.add_launch(F_FILT_LOCAL, off, (int)n_all, filt_aux(n_tiles, false, false));
    L.add_launch(F_FILT_CARRY, off, (int)n_all, 0u);
    L.add_launch(F_FILT_APPLY, off, (int)n_all, filt_aux(n_tiles, false, false));
    return 1;
}
static void launch_filter(const Launch& L, const void* d, hipStream_t s) {
    const uint32_t n_tiles = filt_aux_tiles(L.aux);
    const bool keyed = (L.aux & kKeyedBit) != 0u;
    switch (L.fam) {
        case F_FILT_DETECT: launch_filt_detect((const FiltDesc*)d, L.n, n_tiles, keyed, s); break;
        case F_FILT_CARRY1:
        case F_FILT_CARRY2: launch_master_carry((const MasterDesc*)d, L.n, s); break;
        case F_FILT_ENV: launch_filt_env((const FiltDesc*)d, L.n, n_tiles, s); break;
        case F_FILT_LOCAL: launch_filt_local((const FiltDesc*)d, L.n, n_tiles, s); break;
        case F_FILT_CARRY: launch_filt_carry((const FiltDesc*)d, L.n, s); break;
        case F_FILT_APPLY: launch_filt_apply((const FiltDesc*)d, L.n, n_tiles, (L.aux & kFiltSingleBit) != 0u, keyed, s); break;
    }
}

// ---- limiter: three launches, or one (kernels.h LimDesc) ----
static int lower_limiter(FxLevel& L, std::vector<size_t>& vs) {
    td_graph* g = L.g;
    const uint32_t n_tiles = (uint32_t)((L.M + kLimTile - 1) / kLimTile), chunk = (n_tiles + kThreads - 1) / kThreads;
    const bool multi = n_tiles > 1u;   // (multi: k_lim_detect and k_master_carry first)
    std::vector<LimDesc> d;
    std::vector<MasterDesc> c1;
    for (size_t vi : vs) {
        Vertex& v = g->vertices[vi];
        double c[limiter::kParams];
        limiter::params(L.sr, v.fx.limiter.ceiling_db, v.fx.limiter.lookahead_ms, v.fx.limiter.release_ms, v.fx.limiter.drive_db, c);
        if (!(c[2] <= limiter::kMaxL)) return fail("limiter: lookahead_ms is too many frames at this sample rate");
        LimDesc x{};
        if (multi) {
            if (!(x.x = L.tmp_buffer())) return 0;
            if (!(x.q = reinterpret_cast<float*>(L.tmp_buffer()))) return 0;   // (an edge buffer holds two floats per frame)
        }
        L.head(x, vi);
        x.L = (uint32_t)c[2];
        x.line = (double*)take_line(g, v, (size_t)4 * x.L * sizeof(double));
        if (!x.line) return fail("termdaw_amd: out of device memory for a limiter vertex' line");
        x.parity = v.line.parity;
        x.fresh = enter_chunk(v, L.M, true) ? 0u : 1u;   // (afresh: the state is that of time 0, the half is not read)
        x.n_tiles = n_tiles;
        x.c = c[0];
        x.gin = c[1];
        x.a = c[3];
        for (int j = 0; j < 8; ++j) x.pw[j] = pow(x.a, (double)kLimRun * (double)(1u << j));
        d.push_back(x);
        if (!multi) continue;
        MasterDesc y{};
        y.n_tiles = n_tiles;
        y.chunk = chunk;
        for (int j = 0; j < 8; ++j) y.pwc[j] = pow(x.a, (double)kLimTile * (double)chunk * (double)(1u << j));
        y.a_tile = pow(x.a, (double)kLimTile);
        if (!x.fresh) y.init = x.line + (size_t)x.parity * 2u * x.L;   // (word 0 of the half this chunk reads: u)
        c1.push_back(y);
    }
    const size_t off = L.put(d, vs);
    if (!multi) {
        L.add_launch(F_LIM_APPLY, off, (int)vs.size(), lim_aux(n_tiles, true));
        return 1;
    }
    const size_t o1 = L.cb.st->put(c1);
    for (size_t i = 0; i < vs.size(); ++i) {
        const size_t o = off + i * sizeof(LimDesc), m = o1 + i * sizeof(MasterDesc), tb = (size_t)n_tiles * sizeof(double);
        const size_t a1 = L.cb.scratch(tb), k1 = L.cb.scratch(tb);
        L.cb.scratch_field(o, offsetof(LimDesc, agg), a1);
        L.cb.scratch_field(o, offsetof(LimDesc, carry), k1);
        L.cb.scratch_field(m, offsetof(MasterDesc, agg), a1);
        L.cb.scratch_field(m, offsetof(MasterDesc, carry), k1);
    }
    L.add_launch(F_LIM_DETECT, off, (int)vs.size(), lim_aux(n_tiles, false));
    L.add_launch(F_LIM_CARRY, o1, (int)vs.size(), 0u);
    L.add_launch(F_LIM_APPLY, off, (int)vs.size(), lim_aux(n_tiles, false));
    return 1;
}
static void launch_limiter(const Launch& L, const void* d, hipStream_t s) {
    switch (L.fam) {
        case F_LIM_DETECT: launch_lim_detect((const LimDesc*)d, L.n, lim_aux_tiles(L.aux), s); break;
        case F_LIM_CARRY: launch_master_carry((const MasterDesc*)d, L.n, s); break;
        case F_LIM_APPLY: launch_lim_apply((const LimDesc*)d, L.n, lim_aux_tiles(L.aux), (L.aux & kLimSingleBit) != 0u, s); break;
    }
}

// ---- multiband: seven launches, or one (kernels.h MbDesc) ----
static int lower_multiband(FxLevel& L, std::vector<size_t>& vs) {
    td_graph* g = L.g;
    const uint32_t n_tiles = (uint32_t)((L.M + kMbTile - 1) / kMbTile), chunk = (n_tiles + kThreads - 1) / kThreads;
    const bool multi = n_tiles > 1u;   // (multi: the six launches in front of k_mb_apply)
    static_assert(kMbWords == (uint32_t)multiband::kWords && kMbBlocks == (uint32_t)multiband::kBlocks, "the crossover's operator: one shape on both sides");
    std::vector<MbDesc> d;
    std::vector<CompDesc> bands;
    std::vector<MasterDesc> c1, c2;
    std::vector<size_t> pow_off;
    for (size_t vi : vs) {
        Vertex& v = g->vertices[vi];
        MbDesc x{};
        if (!(x.x = L.tmp_buffer())) return 0;
        for (int b = 0; b < 3; ++b)
            if (!(x.dy[b] = reinterpret_cast<double*>(L.tmp_buffer()))) return 0;   // (an edge buffer holds one double per frame)
        L.head(x, vi);
        x.line = (double*)take_line(g, v, (size_t)kMbState * sizeof(double));
        if (!x.line) return fail("termdaw_amd: out of device memory for a multiband vertex' state");
        x.init = enter_chunk(v, L.M, false) ? x.line : nullptr;   // (afresh: the state is zero, the line is not read)
        x.n_tiles = n_tiles;
        x.chunk = chunk;
        double c[multiband::kParams];
        multiband::params(L.sr, v.fx.mb.lo_hz, v.fx.mb.hi_hz, v.fx.mb.attack_ms, v.fx.mb.release_ms, c);
        for (int s = 0; s < 5; ++s)
            for (int i = 0; i < 5; ++i) x.co[s][i] = c[5 * s + i];
        std::vector<MbPowers> pw(1);
        multiband::powers(c, kMbRun, chunk, pw[0].pw, pw[0].a_tile, pw[0].pwc);
        pow_off.push_back(L.cb.st->put(pw));
        x.aA = c[25];
        x.aR = c[26];
        x.oA = 1.0 - x.aA;
        x.knee = (double)v.fx.mb.knee_db;
        for (int b = 0; b < 3; ++b) {
            x.thr[b] = (double)v.fx.mb.threshold_db[b];
            x.slope[b] = 1.0 - 1.0 / (double)v.fx.mb.ratio[b];
            x.makeup[b] = (double)v.fx.mb.makeup_db[b];
        }
        for (int j = 0; j < 8; ++j) {   // (the compressor's powers: k_comp_env runs over the bands)
            const double e = (double)(1u << j);
            x.pwR[j] = pow(x.aR, (double)kMbRun * e);
            x.pwA[j] = pow(x.aA, (double)kMbRun * e);
        }
        if (multi) {
            for (int b = 0; b < 3; ++b) {
                CompDesc y{};   // what k_comp_env reads of a compressor's descriptor, for band b
                y.dy = x.dy[b];
                y.state = reinterpret_cast<CompState*>(x.line + 2u * kMbWords + 2u * b);   // (k_comp_env stores y1 only: the pair's first word)
                y.frames = x.frames;
                y.n_tiles = n_tiles;
                y.aR = x.aR; y.aA = x.aA; y.oA = x.oA;
                for (int j = 0; j < 8; ++j) { y.pwR[j] = x.pwR[j]; y.pwA[j] = x.pwA[j]; }
                bands.push_back(y);
                MasterDesc y1{}, yl{};
                y1.n_tiles = yl.n_tiles = n_tiles;
                y1.chunk = yl.chunk = chunk;
                yl.op = 1u;
                for (int j = 0; j < 8; ++j) {
                    const double e = (double)(1u << j);
                    y1.pwc[j] = pow(x.aR, (double)kMbTile * (double)chunk * e);
                    yl.pwc[j] = pow(x.aA, (double)kMbTile * (double)chunk * e);
                }
                y1.a_tile = pow(x.aR, (double)kMbTile);
                yl.a_tile = pow(x.aA, (double)kMbTile);
                if (x.init) {
                    y1.init = x.line + 2u * kMbWords + 2u * b;
                    yl.init = x.line + 2u * kMbWords + 2u * b + 1u;
                }
                c1.push_back(y1);
                c2.push_back(yl);
            }
        }
        d.push_back(x);
    }
    const size_t off = L.put(d, vs);
    for (size_t i = 0; i < vs.size(); ++i) L.cb.ptr_field(off + i * sizeof(MbDesc), offsetof(MbDesc, pow), pow_off[i]);
    if (!multi) {
        L.add_launch(F_MB_APPLY, off, (int)vs.size(), mb_aux(n_tiles, true));
        return 1;
    }
    const size_t ob = L.cb.st->put(bands), o1 = L.cb.st->put(c1), o2 = L.cb.st->put(c2);
    for (size_t i = 0; i < vs.size(); ++i) {
        const size_t o = off + i * sizeof(MbDesc), zb = (size_t)n_tiles * 2u * kMbWords * sizeof(double), tb = (size_t)n_tiles * sizeof(double);
        L.cb.scratch_field(o, offsetof(MbDesc, agg), L.cb.scratch(zb));
        L.cb.scratch_field(o, offsetof(MbDesc, carry), L.cb.scratch(zb));
        for (size_t b = 0; b < 3; ++b) {
            const size_t a1 = L.cb.scratch(tb), k1 = L.cb.scratch(tb), a2 = L.cb.scratch(tb), k2 = L.cb.scratch(tb);
            const size_t q = 3 * i + b, oc = ob + q * sizeof(CompDesc), m1 = o1 + q * sizeof(MasterDesc), m2 = o2 + q * sizeof(MasterDesc);
            L.cb.scratch_field(o, offsetof(MbDesc, agg1) + b * sizeof(double*), a1);
            L.cb.scratch_field(o, offsetof(MbDesc, carry2) + b * sizeof(double*), k2);
            L.cb.scratch_field(oc, offsetof(CompDesc, agg1), a1);
            L.cb.scratch_field(oc, offsetof(CompDesc, carry1), k1);
            L.cb.scratch_field(oc, offsetof(CompDesc, agg2), a2);
            L.cb.scratch_field(oc, offsetof(CompDesc, carry2), k2);
            L.cb.scratch_field(m1, offsetof(MasterDesc, agg), a1);
            L.cb.scratch_field(m1, offsetof(MasterDesc, carry), k1);
            L.cb.scratch_field(m2, offsetof(MasterDesc, agg), a2);
            L.cb.scratch_field(m2, offsetof(MasterDesc, carry), k2);
        }
    }
    const int n = (int)vs.size();
    L.add_launch(F_MB_LOCAL, off, n, mb_aux(n_tiles, false));
    L.add_launch(F_MB_CARRY, off, n, 0u);
    L.add_launch(F_MB_DETECT, off, n, mb_aux(n_tiles, false));
    L.add_launch(F_MB_CARRY1, o1, 3 * n, 0u);
    L.add_launch(F_MB_ENV, ob, 3 * n, n_tiles);
    L.add_launch(F_MB_CARRY2, o2, 3 * n, 0u);
    L.add_launch(F_MB_APPLY, off, n, mb_aux(n_tiles, false));
    return 1;
}
static void launch_multiband(const Launch& L, const void* d, hipStream_t s) {
    switch (L.fam) {
        case F_MB_LOCAL: launch_mb_local((const MbDesc*)d, L.n, mb_aux_tiles(L.aux), s); break;
        case F_MB_CARRY: launch_mb_carry((const MbDesc*)d, L.n, s); break;
        case F_MB_DETECT: launch_mb_detect((const MbDesc*)d, L.n, mb_aux_tiles(L.aux), s); break;
        case F_MB_CARRY1:
        case F_MB_CARRY2: launch_master_carry((const MasterDesc*)d, L.n, s); break;
        case F_MB_ENV: launch_comp_env((const CompDesc*)d, L.n, L.aux, s); break;
        case F_MB_APPLY: launch_mb_apply((const MbDesc*)d, L.n, mb_aux_tiles(L.aux), (L.aux & kMbSingleBit) != 0u, s); break;
    }
}

// ---- convolution: three launches, four when spectra have to be built (kernels.h ConvDesc) ----
static int lower_convolution(FxLevel& L, std::vector<size_t>& vs) {
    td_graph* g = L.g;
    const uint32_t n_tiles = (uint32_t)((L.M + kConvB - 1) / kConvB);
    static_assert(kConvB == (uint32_t)conv::kB && kConvN == (uint32_t)conv::kN, "the partition: one size on both sides");
    std::vector<ConvDesc> d, ir;
    uint32_t g_ir = 0, g_fwd = 0, g_inv = 0;
    for (size_t vi : vs) {
        Vertex& v = g->vertices[vi];
        if (!L.sb || v.sample_index >= L.sb->samples.size()) return fail("convolution: sample index out of range");
        const SampleEntry& smp = L.sb->samples[v.sample_index];
        if (const char* why = conv::check_len(L.sr, smp.len, v.fx.conv.length_ms)) return fail(std::string("convolution: ") + why);
        double c[conv::kParams];
        conv::params(L.sr, smp.len, v.fx.conv.length_ms, v.fx.conv.predelay_ms, v.fx.conv.out_db, c);
        ConvDesc x{};
        if (!(x.x = L.tmp_buffer())) return 0;
        L.head(x, vi);
        x.Lh = (uint32_t)c[0];
        x.D = (uint32_t)c[1];
        x.g = c[2];
        x.P = (uint32_t)c[3];
        x.hist = (uint32_t)c[4];
        x.n_tiles = n_tiles;
        x.norm = (uint32_t)v.fx.conv.norm;
        x.ir = smp.d;
        if (!(x.tw = take_twiddles(g))) return fail("termdaw_amd: out of device memory for the convolution vertices' twiddle table");
        const size_t line_bytes = std::max<size_t>(16, 2 * (size_t)x.hist * sizeof(float2));
        bool build = false;
        x.spec = (double*)take_spectra(g, v, (kConvHead + (size_t)x.P * kConvBins * 4u) * sizeof(double), smp.d, smp.len, line_bytes, &build);
        if (!x.spec) return fail("termdaw_amd: out of device memory for a convolution vertex' spectra");
        x.line = (float2*)take_line(g, v, line_bytes);
        if (!x.line) return fail("termdaw_amd: out of device memory for a convolution vertex' line");
        x.parity = v.line.parity;
        x.fresh = enter_chunk(v, L.M, true) ? 0u : 1u;   // (afresh: the frames in front of the chunk are 0, the half is not read)
        x.hist_groups = std::min<uint32_t>(kConvHistGroups, (x.hist + kConvHistFrames - 1u) / kConvHistFrames);
        g_fwd = std::max(g_fwd, n_tiles + x.P - 1u);
        g_inv = std::max(g_inv, n_tiles + x.hist_groups);
        if (build) {
            ir.push_back(x);
            g_ir = std::max(g_ir, x.P);
            if (x.norm) g->conv_checks.push_back(vi);
        }
        d.push_back(x);
    }
    const size_t off = L.put(d, vs);
    for (size_t i = 0; i < vs.size(); ++i) {
        const size_t o = off + i * sizeof(ConvDesc), wb = (size_t)kConvN * 2u * sizeof(double);
        L.cb.scratch_field(o, offsetof(ConvDesc, xs), L.cb.scratch((size_t)(n_tiles + d[i].P - 1u) * wb));
        L.cb.scratch_field(o, offsetof(ConvDesc, ys), L.cb.scratch((size_t)n_tiles * wb));
    }
    if (!ir.empty()) L.add_launch(F_CONV_IR, L.cb.st->put(ir), (int)ir.size(), g_ir);
    L.add_launch(F_CONV_FWD, off, (int)vs.size(), g_fwd);
    L.add_launch(F_CONV_MAC, off, (int)vs.size(), ((n_tiles + kConvTT - 1u) / kConvTT) * kConvMacGroups);
    L.add_launch(F_CONV_INV, off, (int)vs.size(), g_inv);
    return 1;
}
static void launch_convolution(const Launch& L, const void* d, hipStream_t s) {
    switch (L.fam) {
        case F_CONV_IR: launch_conv_ir((const ConvDesc*)d, L.n, L.aux, s); break;
        case F_CONV_FWD: launch_conv_fwd((const ConvDesc*)d, L.n, L.aux, s); break;
        case F_CONV_MAC: launch_conv_mac((const ConvDesc*)d, L.n, L.aux, s); break;
        case F_CONV_INV: launch_conv_inv((const ConvDesc*)d, L.n, L.aux, s); break;
    }
}

// ---- the table ----
// fits: the largest chunk the kind's kernels index (32-bit frames; the line kinds keep room for their look-back, the tiled
// ones for the tile count packed into a launch's aux)
static bool fits_scan(const td_graph*, const Vertex&, size_t M) { return M <= 0xFFFF0000ull; }
static bool fits_line(const td_graph*, const Vertex&, size_t M) { return M <= 0xF0000000ull; }
static bool fits_sat(const td_graph* g, const Vertex&, size_t M) { return M <= 0xF0000000ull && (M + g->sat_tile - 1) / g->sat_tile < 0x100000ull; }
static bool fits_chorus(const td_graph* g, const Vertex&, size_t M) { return M <= 0xF0000000ull && (M + g->chorus_tile - 1) / g->chorus_tile < 0x100000ull; }

static bool fits_voc(const td_graph*, const Vertex&, size_t M) { return M <= 0xFFFF0000ull && (M + kVocTile - 1) / kVocTile < 0x1000000ull; }

static bool fits_mb(const td_graph*, const Vertex&, size_t M) { return M <= 0xFFFF0000ull && (M + kMbTile - 1) / kMbTile < 0x1000000ull; }

// the windows of a chunk and the partitions in front of them stay a 32-bit grid, the frames a 32-bit index
static bool fits_conv(const td_graph*, const Vertex&, size_t M) { return M <= 0xF0000000ull; }

static int family_sat(const Vertex& v) { return v.fx.sat.oversample == 1 ? F_SAT1 : F_SAT_SUM; }

// through: a dry vertex is the Sum it compiles to (factor 1); `lerp`: the estimate goes through (1 - wet) x + wet f(x) at
// (1 - wet) + wet H, H the L2 gain (or Lipschitz bound) of f
static bool dry(const Vertex& v) { return v.wet < 0.0001f; }
static double lerp_gain(const Vertex& v, double H) { return (1.0 - (double)v.wet) + (double)v.wet * H; }
// a compressor is no static gain: no estimate is carried through it -- everything upstream takes the exact forms, as upstream
// of a stem
static double through_comp(const Vertex&, size_t) { return kNoStaticGain; }
// ... and so is a gate, unless it is dry
static double through_gate(const Vertex& v, size_t) { return dry(v) ? 1.0 : kNoStaticGain; }
// a phaser is linear, but time-varying with feedback, and no L2 bound of it is proven: none is guessed
static double through_phaser(const Vertex& v, size_t) { return dry(v) ? 1.0 : kNoStaticGain; }
// a vocoder's gain on its carrier is the modulator's envelope: no static gain -- like a compressor's, unless it is dry
static double through_vocoder(const Vertex& v, size_t) { return dry(v) ? 1.0 : kNoStaticGain; }
// a filter's resonance gain depends on the signal through e[n], and on the time: no static bound of it is proven
static double through_filter(const Vertex& v, size_t) { return dry(v) ? 1.0 : kNoStaticGain; }
// a limiter's gain follows the signal's peaks: no static gain -- the compressor's case, unless it is dry
static double through_limiter(const Vertex& v, size_t) { return dry(v) ? 1.0 : kNoStaticGain; }
// a multiband's three gains follow the bands' levels: no static gain -- the compressor's case, unless it is dry
static double through_multiband(const Vertex& v, size_t) { return dry(v) ? 1.0 : kNoStaticGain; }
// a convolution is linear and time-invariant, but its L2 gain is the peak of the response's spectrum, which lives in the bank
// on the device: no static gain is carried through it unless it is dry
static double through_convolution(const Vertex& v, size_t) { return dry(v) ? 1.0 : kNoStaticGain; }
// an EQ is linear and time-invariant: Hmax of its biquad
static double through_eq(const Vertex& v, size_t sr) {
    if (dry(v)) return 1.0;
    double c[5];
    eq::coefficients(v.fx.eq.kind, sr, v.fx.eq.freq_hz, v.fx.eq.q, v.fx.eq.gain_db, c);
    return lerp_gain(v, eq::hmax(c));
}
// a delay too: out = x + wet (echoes), the echo path's L2 gain is Hecho = 1 / (1 - feedback)
static double through_delay(const Vertex& v, size_t sr) {
    if (dry(v)) return 1.0;
    double c[4];
    delay::params(sr, v.fx.delay.time_ms, v.fx.delay.feedback, v.fx.delay.cross, c);
    return 1.0 + (double)v.wet * c[3];
}
// a saturator's shaper is Lipschitz: Hsat = g_out Hdown Lf g_in Hup
static double through_sat(const Vertex& v, size_t) {
    if (dry(v)) return 1.0;
    double c[6];
    sat::params(v.fx.sat.kind, v.fx.sat.oversample, v.fx.sat.drive_db, v.fx.sat.bias, v.fx.sat.out_db, c);
    return lerp_gain(v, c[5]);
}
// a chorus is linear (and time-varying): Hch, an L2 bound of the modulated four-point read
static double through_chorus(const Vertex& v, size_t) { return dry(v) ? 1.0 : lerp_gain(v, chorus::kHch); }
// a reverb is linear and time-invariant: Hrev, the product of its stages' largest gains
static double through_reverb(const Vertex& v, size_t sr) {
    if (dry(v)) return 1.0;
    double c[reverb::kParams];
    reverb::params(sr, v.fx.reverb.room, v.fx.reverb.damp, v.fx.reverb.width, v.fx.reverb.size, c);
    return lerp_gain(v, c[5]);
}

// check: the kind's block handed to its ranges (<kind>_math.h), field by field
static const char* check_comp(size_t, const FxParams& p, bool) {
    return comp::check(p.comp.threshold_db, p.comp.ratio, p.comp.attack_ms, p.comp.release_ms, p.comp.knee_db, p.comp.makeup_db);
}
static const char* check_eq(size_t sr, const FxParams& p, bool rate_free) { return eq::check(sr, p.eq.kind, p.eq.freq_hz, p.eq.q, p.eq.gain_db, rate_free); }
static const char* check_delay(size_t sr, const FxParams& p, bool rate_free) { return delay::check(sr, p.delay.time_ms, p.delay.feedback, p.delay.cross, rate_free); }
static const char* check_sat(size_t, const FxParams& p, bool) { return sat::check(p.sat.kind, p.sat.oversample, p.sat.drive_db, p.sat.bias, p.sat.out_db); }
static const char* check_chorus(size_t sr, const FxParams& p, bool) {
    return chorus::check(sr, p.chorus.voices, p.chorus.delay_ms, p.chorus.depth_ms, p.chorus.rate_hz, p.chorus.stereo, p.chorus.shape);
}
static const char* check_reverb(size_t sr, const FxParams& p, bool) { return reverb::check(sr, p.reverb.room, p.reverb.damp, p.reverb.width, p.reverb.size); }
static const char* check_gate(size_t, const FxParams& p, bool) {
    return gate::check(p.gate.threshold_db, p.gate.hysteresis_db, p.gate.hold_ms, p.gate.attack_ms, p.gate.release_ms, p.gate.range_db);
}
static const char* check_phaser(size_t sr, const FxParams& p, bool) {
    return phaser::check(sr, p.phaser.stages, p.phaser.lo_hz, p.phaser.hi_hz, p.phaser.rate_hz, p.phaser.feedback, p.phaser.stereo, p.phaser.shape);
}
static const char* check_vocoder(size_t sr, const FxParams& p, bool) {
    return vocoder::check(sr, p.vocoder.bands, p.vocoder.lo_hz, p.vocoder.hi_hz, p.vocoder.q, p.vocoder.response_ms, p.vocoder.out_db);
}
static const char* check_filter(size_t sr, const FxParams& p, bool) {
    const FilterParams& f = p.filter;
    return filter::check(sr, f.kind, f.freq_hz, f.q, f.lfo_oct, f.rate_hz, f.stereo, f.shape, f.env_oct, f.sens_db, f.attack_ms, f.release_ms);
}
static const char* check_limiter(size_t sr, const FxParams& p, bool) {
    return limiter::check(sr, p.limiter.ceiling_db, p.limiter.lookahead_ms, p.limiter.release_ms, p.limiter.drive_db);
}
static const char* check_multiband(size_t sr, const FxParams& p, bool) {
    return multiband::check(sr, p.mb.lo_hz, p.mb.hi_hz, p.mb.threshold_db, p.mb.ratio, p.mb.attack_ms, p.mb.release_ms, p.mb.knee_db, p.mb.makeup_db);
}
static const char* check_convolution(size_t sr, const FxParams& p, bool) { return conv::check(sr, p.conv.length_ms, p.conv.predelay_ms, p.conv.out_db, p.conv.norm); }
// settle: an EQ kind without gain keeps none
static void settle_eq(FxParams& p) {
    if (!eq::kind_has_gain(p.eq.kind)) p.eq.gain_db = 0.0f;
}

// state_slots: a phaser vertex' 2 x (N + 1) doubles and a filter vertex' six take a run of slots
constexpr int kPhaserSlots = (int)(sizeof(PhaserState) / sizeof(StateSlot)), kFiltSlots = (int)(sizeof(FiltState) / sizeof(StateSlot));
static_assert(sizeof(PhaserState) == kPhaserSlots * sizeof(StateSlot) && sizeof(FiltState) == kFiltSlots * sizeof(StateSlot), "a phaser's and a filter's state: whole slots");

// (a function's static: these sources also go through the HIP compiler, whose device pass would want a copy of a namespace-scope
// constant -- and of the host functions it points to.)  A row's family count is the distance to the next row's first family, so
// the rows cover the effect families of `Family` without gap or overlap as long as they stand in its order.  built / keyed_built:
// the entry points the kind's `launch` calls are linked (kernels.h declares them weak); the filter's keyed forms are instantiations
// behind the entry points of its unkeyed ones.
constexpr int kFxKinds = 13;
static_assert(F_COMP_DETECT < F_EQ_LOCAL && F_EQ_LOCAL < F_DELAY_LOCAL && F_DELAY_LOCAL < F_SAT_SUM && F_SAT_SUM < F_CHORUS_SUM &&
              F_CHORUS_SUM < F_REVERB_SUM && F_REVERB_SUM < F_GATE_DETECT && F_GATE_DETECT < F_PHASER_LOCAL && F_PHASER_LOCAL < F_VOC_LOCAL &&
              F_VOC_LOCAL < F_FILT_DETECT && F_FILT_DETECT < F_LIM_DETECT && F_LIM_DETECT < F_MB_LOCAL && F_MB_LOCAL < F_CONV_IR && F_CONV_IR < F_COUNT,
              "the rows of the effect kinds' table stand in the order of their families");
static const FxKind* table() {
    // the kinds' script lines behind (name, gain, angle, wet): the fields of their blocks in the order of the line
    static const FxParam p_comp[] = {FX_F32(CompParams, threshold_db), FX_F32(CompParams, ratio), FX_F32(CompParams, attack_ms),
                                     FX_F32(CompParams, release_ms), FX_F32(CompParams, knee_db), FX_F32(CompParams, makeup_db)};
    static const FxParam p_eq[] = {FX_PARAM(EqParams, kind, NAME, eq::kind_names(), eq::kKinds, 0, nullptr), FX_F32(EqParams, freq_hz), FX_F32(EqParams, q),
                                   FX_F32(EqParams, gain_db)};
    static const FxParam p_delay[] = {FX_F32(DelayParams, time_ms), FX_F32(DelayParams, feedback), FX_F32(DelayParams, cross)};
    static const FxParam p_sat[] = {FX_PARAM(SatParams, kind, NAME, sat::kind_names(), 3, 0, nullptr), FX_F32(SatParams, drive_db), FX_F32(SatParams, bias),
                                    FX_F32(SatParams, out_db), FX_PARAM(SatParams, oversample, INT, nullptr, 0, 1u << 1 | 1u << 2 | 1u << 4 | 1u << 8, "1, 2, 4 or 8")};
    static const FxParam p_chorus[] = {FX_PARAM(ChorusParams, voices, INT, nullptr, 0, 1u << 1 | 1u << 2 | 1u << 3 | 1u << 4, "1 .. 4"), FX_F32(ChorusParams, delay_ms),
                                       FX_F32(ChorusParams, depth_ms), FX_F32(ChorusParams, rate_hz), FX_F32(ChorusParams, stereo),
                                       FX_PARAM(ChorusParams, shape, NAME, chorus::shape_names(), 2, 0, nullptr)};
    static const FxParam p_reverb[] = {FX_F32(ReverbParams, room), FX_F32(ReverbParams, damp), FX_F32(ReverbParams, width), FX_F32(ReverbParams, size)};
    static const FxParam p_gate[] = {FX_F32(GateParams, threshold_db), FX_F32(GateParams, hysteresis_db), FX_F32(GateParams, hold_ms),
                                     FX_F32(GateParams, attack_ms), FX_F32(GateParams, release_ms), FX_F32(GateParams, range_db)};
    static const FxParam p_phaser[] = {FX_PARAM(PhaserParams, stages, INT, nullptr, 0, 1u << 2 | 1u << 4 | 1u << 6 | 1u << 8, "2, 4, 6 or 8"), FX_F32(PhaserParams, lo_hz),
                                       FX_F32(PhaserParams, hi_hz), FX_F32(PhaserParams, rate_hz), FX_F32(PhaserParams, feedback), FX_F32(PhaserParams, stereo),
                                       FX_PARAM(PhaserParams, shape, NAME, chorus::shape_names(), 2, 0, nullptr)};
    static const FxParam p_vocoder[] = {FX_PARAM(VocoderParams, bands, INT, nullptr, 0, 1u << 4 | 1u << 8 | 1u << 16, "4, 8 or 16"), FX_F32(VocoderParams, lo_hz),
                                        FX_F32(VocoderParams, hi_hz), FX_F32(VocoderParams, q), FX_F32(VocoderParams, response_ms), FX_F32(VocoderParams, out_db)};
    static const FxParam p_filter[] = {FX_PARAM(FilterParams, kind, NAME, filter::kind_names(), 4, 0, nullptr), FX_F32(FilterParams, freq_hz), FX_F32(FilterParams, q),
                                       FX_F32(FilterParams, lfo_oct), FX_F32(FilterParams, rate_hz), FX_F32(FilterParams, stereo),
                                       FX_PARAM(FilterParams, shape, NAME, chorus::shape_names(), 2, 0, nullptr), FX_F32(FilterParams, env_oct),
                                       FX_F32(FilterParams, sens_db), FX_F32(FilterParams, attack_ms), FX_F32(FilterParams, release_ms)};
    static const FxParam p_limiter[] = {FX_F32(LimiterParams, ceiling_db), FX_F32(LimiterParams, lookahead_ms), FX_F32(LimiterParams, release_ms),
                                        FX_F32(LimiterParams, drive_db)};
    // (the per-band triples: the line is flat, the bands in the order low, mid, high)
    static const FxParam p_mb[] = {FX_F32(MbParams, lo_hz), FX_F32(MbParams, hi_hz), FX_F32(MbParams, threshold_db[0]), FX_F32(MbParams, threshold_db[1]),
                                   FX_F32(MbParams, threshold_db[2]), FX_F32(MbParams, ratio[0]), FX_F32(MbParams, ratio[1]), FX_F32(MbParams, ratio[2]),
                                   FX_F32(MbParams, attack_ms), FX_F32(MbParams, release_ms), FX_F32(MbParams, knee_db), FX_F32(MbParams, makeup_db[0]),
                                   FX_F32(MbParams, makeup_db[1]), FX_F32(MbParams, makeup_db[2])};
    // (the response stands in front of the block's fields)
    static const FxParam p_conv[] = {{"sample", FxParam::SAMPLE, 0, nullptr, 0, 0, nullptr}, FX_F32(ConvParams, length_ms), FX_F32(ConvParams, predelay_ms),
                                     FX_F32(ConvParams, out_db), FX_PARAM(ConvParams, norm, INT, nullptr, 0, 1u << 0 | 1u << 1, "0 or 1")};
    static const FxKind rows[kFxKinds] = {
        {K_COMPRESSOR, "compressor", "comp", F_COMP_DETECT, F_EQ_LOCAL - F_COMP_DETECT, sizeof(CompDesc), 1, true, fits_scan, nullptr, through_comp, lower_comp, launch_comp, launch_comp_detect && launch_comp_env && launch_comp_apply && launch_master_carry, launch_comp_detect_keyed != nullptr, "compressor / gate", nullptr,
         "add_compressor", "add_compressor: ", FX_SCHEMA(p_comp), check_comp, FxKind::LINE_NONE, false, nullptr},
        {K_EQ, "eq", "eq", F_EQ_LOCAL, F_DELAY_LOCAL - F_EQ_LOCAL, sizeof(EqDesc), 1, false, fits_scan, nullptr, through_eq, lower_eq, launch_eq, launch_eq_local && launch_eq_carry && launch_eq_apply, true, nullptr, nullptr,
         "add_eq", "add_eq: ", FX_SCHEMA(p_eq), check_eq, FxKind::LINE_RATE_FREE, false, settle_eq},
        {K_DELAY, "delay", "delay", F_DELAY_LOCAL, F_SAT_SUM - F_DELAY_LOCAL, sizeof(DelayDesc), 0, false, fits_line, nullptr, through_delay, lower_delay, launch_delay, launch_delay_local && launch_delay_carry && launch_delay_apply, true, nullptr, nullptr,
         "add_delay", "add_delay: ", FX_SCHEMA(p_delay), check_delay, FxKind::LINE_RATE_FREE, true, nullptr},
        {K_SATURATOR, "saturator", "sat", F_SAT_SUM, F_CHORUS_SUM - F_SAT_SUM, sizeof(SatDesc), 0, false, fits_sat, family_sat, through_sat, lower_sat, launch_sat_kind, launch_sat_sum && launch_sat && launch_sat1, true, nullptr, nullptr,
         "add_saturator", "add_saturator: ", FX_SCHEMA(p_sat), check_sat, FxKind::LINE_FULL, true, nullptr},
        {K_CHORUS, "chorus", "chorus", F_CHORUS_SUM, F_REVERB_SUM - F_CHORUS_SUM, sizeof(ChorusDesc), 0, false, fits_chorus, nullptr, through_chorus, lower_chorus, launch_chorus_kind, launch_chorus_sum && launch_chorus, true, nullptr, nullptr,
         "add_chorus", "add_chorus: ", FX_SCHEMA(p_chorus), check_chorus, FxKind::LINE_FULL, true, nullptr},
        {K_REVERB, "reverb", "reverb", F_REVERB_SUM, F_GATE_DETECT - F_REVERB_SUM, sizeof(ReverbDesc), 0, false, fits_line, nullptr, through_reverb, lower_reverb, launch_reverb_kind, launch_reverb_sum && launch_reverb, true, nullptr, nullptr,
         "add_reverb", "add_reverb: ", FX_SCHEMA(p_reverb), check_reverb, FxKind::LINE_FULL, true, nullptr},
        {K_GATE, "gate", "gate", F_GATE_DETECT, F_PHASER_LOCAL - F_GATE_DETECT, sizeof(GateDesc), 1, true, fits_scan, nullptr, through_gate, lower_gate, launch_gate, launch_gate_detect && launch_gate_carry && launch_gate_env && launch_gate_apply, launch_gate_detect_keyed && launch_gate_env_keyed, "compressor / gate", rest_gate,
         "add_gate", "add_gate: ", FX_SCHEMA(p_gate), check_gate, FxKind::LINE_FULL, false, nullptr},
        {K_PHASER, "phaser", "phaser", F_PHASER_LOCAL, F_VOC_LOCAL - F_PHASER_LOCAL, sizeof(PhaserDesc), kPhaserSlots, false, fits_scan, nullptr, through_phaser, lower_phaser, launch_phaser, launch_phaser_local && launch_phaser_carry && launch_phaser_apply, true, nullptr, nullptr,
         "add_phaser", "add_phaser: ", FX_SCHEMA(p_phaser), check_phaser, FxKind::LINE_FULL, false, nullptr},
        {K_VOCODER, "vocoder", "voc", F_VOC_LOCAL, F_FILT_DETECT - F_VOC_LOCAL, sizeof(VocDesc), 0, true, fits_voc, nullptr, through_vocoder, lower_vocoder, launch_vocoder, launch_voc_local && launch_voc_carry && launch_voc_env && launch_voc_apply, launch_voc_local_keyed && launch_voc_apply_keyed, "vocoder", nullptr,
         "add_vocoder", "add_vocoder: ", FX_SCHEMA(p_vocoder), check_vocoder, FxKind::LINE_FULL, false, nullptr},
        {K_FILTER, "filter", "filt", F_FILT_DETECT, F_LIM_DETECT - F_FILT_DETECT, sizeof(FiltDesc), kFiltSlots, true, fits_scan, nullptr, through_filter, lower_filter, launch_filter, launch_filt_detect && launch_filt_env && launch_filt_local && launch_filt_carry && launch_filt_apply && launch_master_carry, true, nullptr, nullptr,
         "add_filter", "add_filter: ", FX_SCHEMA(p_filter), check_filter, FxKind::LINE_FULL, false, nullptr},
        {K_LIMITER, "limiter", "lim", F_LIM_DETECT, F_MB_LOCAL - F_LIM_DETECT, sizeof(LimDesc), 0, false, fits_scan, nullptr, through_limiter, lower_limiter, launch_limiter, launch_lim_detect && launch_lim_apply && launch_master_carry, true, nullptr, nullptr,
         "add_limiter", "add_limiter: ", FX_SCHEMA(p_limiter), check_limiter, FxKind::LINE_FULL, false, nullptr},
        {K_MULTIBAND, "multiband", "mb", F_MB_LOCAL, F_CONV_IR - F_MB_LOCAL, sizeof(MbDesc), 0, false, fits_mb, nullptr, through_multiband, lower_multiband, launch_multiband, launch_mb_local && launch_mb_carry && launch_mb_detect && launch_mb_apply && launch_comp_env && launch_master_carry, true, nullptr, nullptr,
         "add_multiband", "add_multiband: multiband: ", FX_SCHEMA(p_mb), check_multiband, FxKind::LINE_FULL, false, nullptr},
        {K_CONVOLUTION, "convolution", "conv", F_CONV_IR, F_COUNT - F_CONV_IR, sizeof(ConvDesc), 0, false, fits_conv, nullptr, through_convolution, lower_convolution, launch_convolution, launch_conv_ir && launch_conv_fwd && launch_conv_mac && launch_conv_inv, true, nullptr, nullptr,
         "add_convolution", "add_convolution: convolution: ", FX_SCHEMA(p_conv), check_convolution, FxKind::LINE_FULL, false, nullptr},
    };
    return rows;
}

}  // namespace fxk

const FxKind* fx_kind(Kind k) {
    const FxKind* rows = fxk::table();
    for (int i = 0; i < fxk::kFxKinds; ++i)
        if (rows[i].kind == k) return &rows[i];
    return nullptr;
}
const FxKind* fx_of_family(int fam) {
    static const FxKind* const* const by = [] {   // the row of every family, filled once
        static const FxKind* row[F_COUNT] = {};
        const FxKind* rows = fxk::table();
        for (int i = 0; i < fxk::kFxKinds; ++i)
            for (int f = rows[i].first_family; f < rows[i].first_family + rows[i].n_families; ++f) row[f] = &rows[i];
        return row;
    }();
    return fam >= 0 && fam < F_COUNT ? by[fam] : nullptr;
}

}  // namespace tde
