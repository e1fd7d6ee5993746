"""The limiter vertex on the device (td_graph_add_limiter) against its float64 twin (tests/np_limiter.py, the
serial restatement of the definition in include/termdaw_amd.h), run on the engine's own constants (td_limiter_params).

The input of the vertex under test always comes from the engine itself: a second render of the same graph with set_output on
the vertex in front, read as f32 -- the oracle-verified part of the graph is not restated here.

Bounds.  wet = 1, gain = 1, angle = 0, per value:  |p' - p| <= 2^-23 |p| + E max|p| on the limited signal p, carried through the
definition's f32 lerp against the DELAYED input xd to the vertex' output (test_gpu_eq.assert_close says why it is not asserted on
the output as it stands).  The first term is the one f32 rounding of the chain, which may flip; E covers the float64 order of the
release scan and of the prefix sums behind G: 8 x what the numpy emulation of the kernels' order shows over this file's own grid
and inputs (tests/limiter_projects.py E, derived and re-checked on the CPU by tests/test_limiter_host.py; E = 3.2e-10, under the
cap 2^-28).  Q is exact on both sides.  The ceiling is asserted on the device's own output, through the same lerp: no wet-path
value above c (1 + 2^-22).
With wet in (0, 1), pan and gain: 4 x 2^-23 x max(|dry|, |p|) x |amplitude| absolute, as for the EQ.  PCM cases: within one word
of the twin's quantised value.

Every case prints its worst error over the bound; DESIGN.md §3x records how many cases came out bit-identical."""
import os
import subprocess
import sys
import wave

import numpy as np
import pytest

from termdaw_amd import workloads as W

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import limiter_projects as LP  # noqa: E402
import np_limiter as NL  # noqa: E402
from test_gpu_compressor import MIX, _quantise16  # noqa: E402
from test_gpu_eq import REL, F32_TINY, _f32_down, _pull_all, assert_close, build, mix_bound, render_f32  # noqa: E402
from test_gpu_stems import _write_project  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIM_LAUNCHES = ["k_lim_detect", "k_lim_carry", "k_lim_apply"]
CASE = (-6.0, 10.0, 50.0, 12.0)   # ceiling, lookahead (480 frames at 48 kHz), release, drive


def twin(api, sr, case, x, state=None):
    """(p float32, xd, G, end state) of the serial twin on the engine's constants."""
    return NL.serial(x, api.limiter_params(sr, *case), state)[:4]


def close(y, xd, p, what):
    return assert_close(y, xd, p, what, LP.E)


def under_the_ceiling(y, xd, c, what):
    """Some wet-path value p' with |p'| <= c (1 + 2^-22) gives y = xd + 1 (p' - xd): the lerp is monotone in p'."""
    one = np.float32(1.0)
    top = _f32_down(np.full(xd.shape, c * (1.0 + 2.0 ** -22)))
    lo, hi = xd + one * (-top - xd), xd + one * (top - xd)
    bad = ~((lo <= y) & (y <= hi))
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:4].tolist(), y[bad][:4], c)


# ---- the grid ----
@pytest.mark.parametrize("sr", LP.RATES)
@pytest.mark.parametrize("kind", LP.INPUTS)
def test_grid_matches_the_twin(gpu_api, sr, kind):
    cases = LP.grid_cases(sr)
    assert len(cases) == 45
    p = LP.base_project(kind, sr=sr)
    for i, (c, _) in enumerate(cases):
        LP.add_limiter(p, "m%d" % i, "bus", c)
    built = build(gpu_api, p)
    x = render_f32(gpu_api, built, "bus", p.cs)
    n = p.cs * p.bl
    assert np.abs(x).max() > 0.05 and n > 5 * 2048
    marks = np.arange(2048, n, 2048)
    worst, exact, deep = 0.0, 0, 0
    seen = {"release": 0, "ramp": 0}
    for i, (c, Lw) in enumerate(cases):
        k = gpu_api.limiter_params(sr, *c)
        assert k[2] == Lw and k[4] == Lw - 1
        pw, xd, G, end = twin(gpu_api, sr, c, x)
        omh, u, _ = NL.trace(x, k)
        # the case is not vacuous, and tile boundaries fall inside the stretches no single tile can decide on its own
        deep += int(G.min() < 0.5)
        seen["release"] += int(np.any((u[marks] > omh[marks]) & (u[marks] > 1e-3)))        # u still decaying from a peak in the tile before
        seen["ramp"] += int(Lw > 1 and np.any(G[marks] < G[marks - 1] - 1e-9))             # G on its way down to a peak the window has just met
        y = render_f32(gpu_api, built, "m%d" % i, p.cs)
        worst = max(worst, close(y, xd, pw, "%s %d %s" % (kind, sr, c)))
        under_the_ceiling(y, xd, k[0], (kind, sr, c))
        want = xd + np.float32(1.0) * (pw - xd)
        exact += int(np.array_equal(y.view(np.uint32), want.view(np.uint32)))
    print("grid %s %d: %d cases, worst |y - want| %.3g x the plain bound, %d bit-identical to the twin; smallest G under 0.5 in %d cases; "
          "tile boundaries inside a release tail / a lookahead ramp in %d / %d cases" % (kind, sr, len(cases), worst, exact, deep, seen["release"], seen["ramp"]))
    assert 3 * deep >= len(cases), deep
    assert seen["release"] >= 1 and seen["ramp"] >= 1, seen
    assert np.array_equal(render_f32(gpu_api, built, "bus", p.cs), x)   # (and every render above saw this input)


# ---- chunks, pulls, restarts ----
@pytest.mark.parametrize("bl", [1024, 64])
def test_chunked_and_pulled_renders_match_the_twin(gpu_api, bl):
    """0.5 s of `gated` at L = 480: whole, in 4 096-frame chunks, and by block pulls of `bl` frames (64: shorter than the
    lookahead) -- each inside the bound, and each restarted render bitwise the first."""
    p = LP.base_project("gated", bl=bl, seconds=0.5)
    LP.add_limiter(p, "m", "bus", CASE)
    built = build(gpu_api, p)
    n = p.cs * bl
    x = render_f32(gpu_api, built, "bus", p.cs)
    assert gpu_api.limiter_params(48000, *CASE)[2] == 480
    pw, xd, G, end = twin(gpu_api, 48000, CASE, x)
    assert G.min() < 0.6
    forms = {}
    forms["whole"] = [render_f32(gpu_api, built, "m", p.cs) for _ in range(2)]
    forms["chunks"] = [render_f32(gpu_api, built, "m", p.cs, max_chunk_frames=4096) for _ in range(2)]
    assert n / 4096 > 5
    built[2].set_option("max_chunk_frames", 1 << 24)
    forms["pulls"] = [_pull_all(gpu_api, built, "m", p.cs) for _ in range(2)]
    for name, (a, b) in forms.items():
        assert a.shape == pw.shape
        close(a, xd, pw, "%s bl %d" % (name, bl))
        under_the_ceiling(a, xd, 10.0 ** (-6.0 / 20.0), name)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), name
    # the state really crosses the cuts: restarted from zero state, chunk 1 would be far outside the bound
    restart = twin(gpu_api, 48000, CASE, x[4096:8192])[0]
    assert np.abs(restart.astype(np.float64) - pw[4096:8192]).max() > 1e-3
    # a set_time in the middle of pulling restarts the limiter from silence: two pulls, a jump, one pull
    at = (4000 // bl) * bl
    got = []
    for out in ("m", "bus"):
        sb, fb, g = p.build(gpu_api)
        assert g.set_output(out)
        for _ in range(2):
            g.render(sb, fb)
            fb.set_time_to_next_block()
        fb.set_time(at)
        g.set_time(at)
        got.append(np.stack(g.render(sb, fb), axis=1))
    assert np.abs(got[1]).max() > 0.01
    after, xda, _, _ = twin(gpu_api, 48000, CASE, got[1])
    assert not xda[:min(bl, 479)].any() and xd[at:at + bl].any()   # (silence in front after the jump, where the running render has signal)
    close(got[0], xda, after, "pull after set_time")


@pytest.mark.parametrize("L", [1, 2048])
def test_an_idle_input_comes_out_driven_and_delayed_bit_for_bit(gpu_api, L):
    case = (-0.1, LP.lookahead_ms(48000, L), 50.0, -6.0)
    p = LP.base_project("gated", seconds=0.5)
    LP.add_limiter(p, "m", "bus", case)
    built = build(gpu_api, p)
    x = render_f32(gpu_api, built, "bus", p.cs)
    k = gpu_api.limiter_params(48000, *case)
    assert k[2] == L and np.abs(x).max() * k[1] < k[0] and np.abs(x).max() > 0.05
    xd = np.concatenate([np.zeros((L - 1, 2), np.float32), x])[:len(x)]
    pw = (xd.astype(np.float64) * k[1]).astype(np.float32)
    want = xd + np.float32(1.0) * (pw - xd)
    for opts in ({}, {"max_chunk_frames": 4096}):
        y = render_f32(gpu_api, built, "m", p.cs, **opts)
        assert np.array_equal(y.view(np.uint32), want.view(np.uint32)), (L, opts, np.argwhere(y != want)[:4].tolist())
    built[2].set_option("max_chunk_frames", 1 << 24)
    y = _pull_all(gpu_api, built, "m", p.cs)
    assert np.array_equal(y.view(np.uint32), want.view(np.uint32)), (L, "pulls")


def test_more_than_256_tiles(gpu_api):
    """12 s at 48 kHz of the looped `gated` input: 576 512 frames, 282 tiles -- the carry's lanes fold two tiles each."""
    p = LP.base_project("gated", seconds=12.0)
    LP.add_limiter(p, "m", "bus", CASE)
    built = build(gpu_api, p)
    n = p.cs * p.bl
    assert n == 576512 and (n + 2047) // 2048 == 282
    x = render_f32(gpu_api, built, "bus", p.cs)
    pw, xd, G, end = twin(gpu_api, 48000, CASE, x)
    assert G.min() < 0.6
    y = render_f32(gpu_api, built, "m", p.cs)
    close(y, xd, pw, "282 tiles")
    under_the_ceiling(y, xd, 10.0 ** (-6.0 / 20.0), "282 tiles")


# ---- the mix ----
@pytest.mark.parametrize("wet,gain,angle", MIX)
def test_wet_pan_and_gain(gpu_api, wet, gain, angle):
    p = LP.base_project("drums", seconds=0.5)
    LP.add_limiter(p, "m", "bus", CASE, wet=wet, gain=gain, angle=angle)
    built = build(gpu_api, p)
    x = render_f32(gpu_api, built, "bus", p.cs)
    y = render_f32(gpu_api, built, "m", p.cs)
    c = gpu_api.limiter_params(48000, *CASE)
    want, _ = NL.process(x, c, wet=wet, gain=gain, angle=angle)
    proc, xd = NL.serial(x, c)[:2]
    lim = mix_bound(xd, proc, gain, angle)
    err = np.abs(y.astype(np.float64) - want.astype(np.float64))
    print("wet %g gain %g angle %g: worst error / bound %.3g" % (wet, gain, angle, float(np.max(err / lim))))
    assert (err <= lim).all(), (float(np.max(err / lim)), np.argwhere(err > lim)[:4].tolist())
    assert np.abs(proc - xd).max() > 1e-3   # (the vertex does something)


def test_dry_passes_the_input_through_undelayed(gpu_api):
    p = LP.base_project("drums", seconds=0.5)
    LP.add_limiter(p, "dry", "bus", CASE, wet=0.0)
    LP.add_limiter(p, "almost", "bus", CASE, wet=0.00009)
    LP.add_limiter(p, "wet", "bus", CASE)
    built = build(gpu_api, p)
    x = render_f32(gpu_api, built, "bus", p.cs)
    for name in ("dry", "almost"):
        y = render_f32(gpu_api, built, name, p.cs)
        assert np.array_equal(y, x), (name, np.argwhere(y != x)[:4].tolist())
    g = built[2]
    g.set_profiling(1)
    render_f32(gpu_api, built, "dry", p.cs)
    names = list(g.kernel_times())
    assert not any(n.startswith("k_lim") for n in names) and "k_sum" in names, names   # wet < 0.0001: a plain sum launch
    render_f32(gpu_api, built, "wet", p.cs)
    assert [n for n in g.kernel_times() if n.startswith("k_lim")] == LIM_LAUNCHES


# ---- placement ----
def test_in_front_of_a_normalize_output(gpu_api):
    p = LP.base_project("drums", seconds=1.0)
    LP.add_limiter(p, "m", "bus", CASE)
    p.add_normalize("out", 1.0, 0.0)
    p.connect("m", "out")
    built = build(gpu_api, p)
    x = render_f32(gpu_api, built, "bus", p.cs)
    c = render_f32(gpu_api, built, "m", p.cs)
    pw, xd, _, _ = twin(gpu_api, 48000, CASE, x)
    close(c, xd, pw, "in front of Normalize")
    # normalize_gen (extensions.rs:321-329) on what the limiter really handed on: the running block peak from 1e-6, f32
    pk = np.abs(c).reshape(-1, p.bl * 2).max(axis=1)
    run = np.maximum.accumulate(np.concatenate([[np.float32(0.000001)], pk]).astype(np.float32))[1:]
    want = c * np.repeat(np.float32(1.0) / run, p.bl)[:, None]
    sb, fb, g = built
    g.set_output("out")
    fb.set_time(0)
    g.set_time(0)
    g.reset_normalize_vertices()
    pcm, f = g.render_all(sb, fb, p.cs, 16)
    assert (np.abs(f.astype(np.float64) - want) <= 2.0 * REL * np.abs(want) + F32_TINY).all()
    assert np.abs(pcm.astype(np.int64) - _quantise16(want)).max() <= 1


def test_as_a_stem_and_two_in_series(gpu_api):
    c2 = (-12.0, 0.0, 5.0, 0.0)
    p = LP.base_project("drums", seconds=1.0)
    LP.add_limiter(p, "m1", "bus", CASE)
    LP.add_limiter(p, "m2", "m1", c2, gain=0.8, angle=-20.0)
    p.add_sum("post", 0.5, 10.0)
    p.connect("m2", "post")
    built = build(gpu_api, p)
    x = render_f32(gpu_api, built, "bus", p.cs)
    y1 = render_f32(gpu_api, built, "m1", p.cs)
    pw, xd, _, _ = twin(gpu_api, 48000, CASE, x)
    close(y1, xd, pw, "first of two")
    # the second one against the twin on what the first one really handed it
    y2 = render_f32(gpu_api, built, "m2", p.cs)
    k2 = gpu_api.limiter_params(48000, *c2)
    w2, _ = NL.process(y1, k2, gain=0.8, angle=-20.0)
    proc, xd2 = NL.serial(y1, k2)[:2]
    assert np.abs(proc - xd2).max() > 1e-3
    assert (np.abs(y2.astype(np.float64) - w2) <= mix_bound(xd2, proc, 0.8, -20.0)).all()
    # both as stems of a render whose output sits downstream
    sb, fb, g = built
    g.set_output("post")
    g.set_stems(["m2", "m1"])
    fb.set_time(0)
    g.set_time(0)
    g.render_all(sb, fb, p.cs, 16)
    assert np.abs(g.read_stem_pcm(0).astype(np.int64) - _quantise16(y2)).max() == 0
    assert np.abs(g.read_stem_pcm(1).astype(np.int64) - _quantise16(y1)).max() == 0
    g.set_stems([])


def test_fed_by_an_inlined_loop_source_and_a_gain_stage(gpu_api):
    import gate_projects as GP
    case = (-12.0, 2.0, 30.0, 6.0)
    p = W.ProjectScript(48000, 1024)
    p.set_length(0.5)
    p.assets["a0"] = W.Asset(GP.gated_int16(3))
    p.assets["a1"] = W.Asset(W.noise_int16(51, 9001))
    p.load_sample("a0", "a0", "")
    p.load_sample("a1", "a1", "normalize-seperate")
    p.add_sampleloop("l0", 0.7, 30.0, "a0")     # read by the limiter itself (term kinds 1 / 3)
    p.add_sampleloop("l1", 0.02, 0.0, "a1")
    p.add_sum("stage", 0.5, -45.0)              # one input: a gain / pan stage, read through (term kind 4)
    p.connect("l1", "stage")
    LP.add_limiter(p, "m", "l0", case)
    p.connect("stage", "m")
    p.set_output("m")
    built = p.build(gpu_api)
    a = render_f32(gpu_api, built, "l0", p.cs)
    b = render_f32(gpu_api, built, "stage", p.cs)
    x = (np.float32(0.0) + a) + b               # sum_inputs (extensions.rs:310-319), f32, in connect() order
    pw, xd, G, _ = twin(gpu_api, 48000, case, x)
    assert G.min() < 0.7 and G.max() - G.min() > 0.2   # (the limiter works, and its gain moves)
    for packed in (1, 0):
        y = render_f32(gpu_api, built, "m", p.cs, packed_samples=packed)
        close(y, xd, pw, "inlined terms, packed_samples %d" % packed)


def test_batch_members_are_bitwise_their_own_renders(gpu_api):
    projects = []   # (`noise` has a source called m: the limiters are lm)
    cases = [c for c, _ in LP.grid_cases(48000)]
    for i in range(8):
        p = LP.base_project(LP.INPUTS[i % 3], seconds=1.0, seed=i)
        c = cases[(13 * i + 5) % len(cases)]
        LP.add_limiter(p, "lm", "bus", c, wet=[1.0, 0.6][i % 2], gain=[1.0, 0.7][(i // 4) % 2])
        if i % 4 == 1:     # a second one in series, as the output
            LP.add_limiter(p, "lm2", "lm", cases[(29 * i + 1) % len(cases)])
            p.set_output("lm2")
        elif i % 4 == 2:   # in front of a Normalize output
            p.add_normalize("out", 1.0, 0.0)
            p.connect("lm", "out")
            p.set_output("out")
        else:
            p.set_output("lm")
        projects.append(p)
    cs = projects[0].cs
    own = []   # per project: its first and its second render (the second starts with the voices the first left sounding)
    for p in projects:
        sb, fb, g = p.build(gpu_api)
        first = g.render_all(sb, fb, cs, 16, want_f32=False)[0]
        g.reset_normalize_vertices()
        fb.set_time(0)
        g.set_time(0)
        own.append((first, g.render_all(sb, fb, cs, 16, want_f32=False)[0]))
    assert len({o[0].tobytes() for o in own}) == 8
    batch = gpu_api.Batch()
    for p in projects:
        batch.add(*p.build(gpu_api))
    for rep in range(2):
        batch.rewind()
        assert batch.render_all(cs, 16) == cs * 1024
        for i in range(8):
            assert np.array_equal(batch.read_pcm(i, cs), own[i][rep]), (rep, i)


def test_projects_without_a_limiter_launch_no_limiter_kernel(gpu_api):
    for p in (W.drum_project(seconds=1.0), W.config2(seconds=1.0, n_src=8)):
        sb, fb, g = p.build(gpu_api)
        g.set_profiling(1)
        g.render_all(sb, fb, p.cs, 16, want_f32=False)
        names = list(g.kernel_times())
        assert names and not any(n.startswith("k_lim") for n in names), names
    p = LP.base_project("drums")
    LP.add_limiter(p, "m", "bus", CASE)
    p.set_output("m")
    sb, fb, g = p.build(gpu_api)
    g.set_profiling(1)
    g.render_all(sb, fb, p.cs, 16, want_f32=False)
    assert [n for n in g.kernel_times() if n.startswith("k_lim")] == LIM_LAUNCHES
    # a render of one tile (2 048 frames) is k_lim_apply alone, as every block pull is
    g.set_time(0)
    fb.set_time(0)
    g.set_profiling(1)   # (the times add up over renders until profiling is set again)
    g.render_all(sb, fb, 2, 16, want_f32=False)
    assert [n for n in g.kernel_times() if n.startswith("k_lim")] == ["k_lim_apply"]


# ---- the guard modes ----
def _guard_project(limiter_first):
    p = W.ProjectScript(48000, 1024)
    p.set_length(1.0)
    p.assets["a"] = W.Asset(W.noise_int16(7, 9000))
    p.load_sample("a", "a", "")
    p.event_files["f"] = np.array([(0.01, 60.0, 0.8), (0.4, 60.0, 0.0), (0.5, 64.0, 0.6), (0.9, 64.0, 0.0)], np.float32)
    p.load_midi_floww("f", "f")
    p.add_sampleloop("s", 0.5, 0.0, "a")
    p.add_bandpass("b1", 1.0, 0.0, 1.0, 300.0, 5000.0, True)
    p.add_bandpass("b2", 1.0, 10.0, 1.0, 200.0, 8000.0, True)
    p.add_synth("y", 0.5, 0.0, "f", 0.4, 0.3, W.HIT_ADSR, 1.0, 0.8, W.NOTE_ADSR, 0.5, W.STD_ADSR)
    p.add_sum("bus", 1.0, 0.0)
    p.add_limiter("m", 1.0, 0.0, 1.0, -12.0, 5.0, 80.0, 6.0)
    if limiter_first:   # loop -> limiter -> band-pass chain; the synth joins behind the limiter
        p.connect("s", "m"); p.connect("m", "b1"); p.connect("b1", "b2"); p.connect("b2", "bus"); p.connect("y", "bus")
        p.set_output("bus")
    else:               # band-pass chain and synth -> bus -> limiter
        p.connect("s", "b1"); p.connect("b1", "b2"); p.connect("b2", "bus"); p.connect("y", "bus"); p.connect("bus", "m")
        p.set_output("m")
    return p


def _guard_renders(gpu_api, p):
    outs, names = {}, {}
    for mode, (bm, sm) in (("guard", (2, 2)), ("exact", (0, 1))):
        sb, fb, g = p.build(gpu_api)
        g.set_option("band_mode", bm)
        g.set_option("sine_mode", sm)
        g.set_profiling(1)
        outs[mode] = g.render_all(sb, fb, p.cs, 16, want_pcm=False)[1]
        names[mode] = list(g.kernel_times())
    return outs, names


def test_guard_keeps_the_scan_and_fast_sines_downstream_of_a_limiter(gpu_api):
    outs, names = _guard_renders(gpu_api, _guard_project(True))
    rms = float(np.sqrt(np.mean((outs["guard"].astype(np.float64) - outs["exact"].astype(np.float64)) ** 2)))
    print("guarded scan + fast sines downstream of a limiter: rms %.3g against the exact forms" % rms)
    assert rms <= 1e-6 and np.abs(outs["exact"]).max() > 0.05
    assert "k_band_scan" in names["guard"] and "k_sine_probe" in names["guard"], names["guard"]
    assert not any(n in names["guard"] for n in ("k_band_pass", "k_band_spec")), names["guard"]
    assert [n for n in names["guard"] if n.startswith("k_lim")] == LIM_LAUNCHES


def test_guard_renders_the_exact_forms_upstream_of_a_limiter(gpu_api):
    outs, names = _guard_renders(gpu_api, _guard_project(False))
    assert np.array_equal(outs["guard"].view(np.uint32), outs["exact"].view(np.uint32)) and np.abs(outs["exact"]).max() > 0.05
    assert "k_band_scan" not in names["guard"] and "k_sine_probe" not in names["guard"], names["guard"]
    assert any(n in names["guard"] for n in ("k_band_pass", "k_band_spec")), names["guard"]


# ---- the front end ----
def test_front_end_renders_a_limited_drum_bus(gpu_api, tmp_path):
    p = W.limiter_project(seconds=1.0)
    d = str(tmp_path / "proj")
    _write_project(p, d)
    out = str(tmp_path / "m.wav")
    r = subprocess.run([sys.executable, "-m", "termdaw_amd", d, "-o", out], env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    st = gpu_api.State(open_dir=d)
    assert st.refresh(), gpu_api.last_error()
    assert 'add_limiter("lim",' in st.dump_calls()
    mem = st.render_to_memory()
    with wave.open(out, "rb") as w:
        words = np.frombuffer(w.readframes(w.getnframes()), np.int16).reshape(-1, 2)
    assert words.shape == mem.shape and np.array_equal(words, mem) and np.abs(mem).max() > 1000
    # the ceiling holds on the words: -1 dB of full scale
    assert np.abs(mem.astype(np.int64)).max() <= int(10.0 ** (-1.0 / 20.0) * 32767.0) + 1
    # ... and the limiter is really in the path: with it dry the words differ
    q = W.limiter_project(seconds=1.0, wet=0.0)
    d2 = str(tmp_path / "plain")
    _write_project(q, d2)
    st2 = gpu_api.State(open_dir=d2)
    assert st2.refresh()
    assert not np.array_equal(st2.render_to_memory(), mem)
