"""The filter vertex on the device (td_graph_add_filter) against its float64 twin (tests/np_filter.py, the serial
restatement of the definition in include/termdaw_amd.h), run on the engine's own constants (td_filter_params).

The input of the vertex under test -- and its key -- always come from the engine itself: further renders of the same graph with
set_output on the vertex in front, read as f32 -- the oracle-verified part of the graph is not restated here.

Bounds.  wet = 1, gain = 1, angle = 0, per value:  |p' - p| <= 2^-23 |p| + E max|p| on the filter's output p, carried through the
definition's f32 lerp to the vertex' output (test_gpu_eq.assert_close says why it is not asserted on the output as it stands).
The first term is the one f32 rounding of p, which may flip; E covers the float64 re-association of the scans, the follower's
included: 8 x what the numpy emulation of the tiled scans shows over this file's own grid and inputs (tests/filter_projects.py E,
derived and re-checked on the CPU by tests/test_filter_host.py; far under the cap 2^-28).  g[n] is the same bits on both sides
where e[n] is: IEEE add, multiply, floor, fabs, min and max on the same constants, and one correctly rounded division.
With wet in (0, 1), pan and gain: 4 x 2^-23 x max(|dry|, |p|) x |amplitude| absolute, as for the EQ.

Every case prints its worst error over the bound; DESIGN.md §3w records how many cases came out bit-identical."""
import os
import subprocess
import sys
import wave

import numpy as np
import pytest

from termdaw_amd import workloads as W

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import filter_projects as FP  # noqa: E402
import key_projects as KP  # noqa: E402
import np_filter as NF  # noqa: E402
from test_gpu_compressor import MIX, _quantise16  # noqa: E402
from test_gpu_eq import REL, F32_TINY, _pull_all, assert_close, build, mix_bound, render_f32  # noqa: E402
from test_gpu_stems import _write_project  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FOLLOWER = ["k_filt_detect", "k_filt_carry_y1", "k_filt_env", "k_filt_carry_e"]
FILTER = ["k_filt_local", "k_filt_carry", "k_filt_apply"]
# kind, freq, q, lfo_oct, rate, stereo, shape, env_oct, sens_db, attack_ms, release_ms
CASE = ("lowpass", 400.0, 4.0, 2.0, 3.0, 0.25, "sine", 4.0, 18.0, 2.0, 80.0)       # an auto-wah with a slow sweep on top
STILL = ("bandpass", 900.0, 8.0, 3.0, 7.0, 0.5, "triangle", 0.0, 0.0, 0.0, 1.0)    # the LFO alone: no follower
CASE_HP = ("highpass", 2500.0, 12.0, 1.0, 0.5, 0.0, "sine", -6.0, 30.0, 0.0, 20.0)


def _bits(a):
    return a.view(np.uint32)


def twin(api, sr, case, x, state=None, t0=0, key=None):
    """(p float32, end state) of the serial twin on the engine's constants."""
    v, end = NF.serial(x, FP.spec(api, sr, case), state, t0, key)
    return v.astype(np.float32), end


def close(y, x, p, what):
    return assert_close(y, x, p, what, FP.E)


# ---- the grid ----
@pytest.mark.parametrize("sr", FP.RATES)
@pytest.mark.parametrize("kind", FP.INPUTS)
def test_grid_matches_the_twin(gpu_api, sr, kind):
    cases = FP.grid_cases(sr)
    assert len(cases) == 108
    p = FP.base_project(kind, sr=sr)
    for i, c in enumerate(cases):
        FP.add_filter(p, "f%d" % i, "bus", c)
    built = build(gpu_api, p)
    x = render_f32(gpu_api, built, "bus", p.cs)
    n = p.cs * p.bl
    assert np.abs(x).max() > 0.05 and n > 5 * NF.TILE
    worst, exact, acts = 0.0, 0, 0
    vs, _ = NF.serial(x, [FP.spec(gpu_api, sr, c) for c in cases])   # (the cases side by side)
    for i, v in enumerate(vs):
        pw = v.astype(np.float32)
        y = render_f32(gpu_api, built, "f%d" % i, p.cs)
        worst = max(worst, close(y, x, pw, "%s %d %s" % (kind, sr, cases[i])))
        want = x + np.float32(1.0) * (pw - x)
        exact += int(np.array_equal(_bits(y), _bits(want)))
        acts += int(np.abs(want.astype(np.float64) - x).max() > 64.0 * (REL + FP.E) * np.abs(x).max())
    print("grid %s %d: %d cases, worst |y - want| %.3g x the plain bound, %d bit-identical to the twin" % (kind, sr, len(cases), worst, exact))
    assert acts == len(cases), acts   # (every case moves the signal)
    assert np.array_equal(render_f32(gpu_api, built, "bus", p.cs), x)   # (and every render above saw this input)


# ---- chunks, pulls, restarts ----
@pytest.mark.parametrize("case", [CASE, STILL], ids=["follower", "lfo-only"])
@pytest.mark.parametrize("bl", [1024, 64])
def test_chunked_and_pulled_renders_match_the_twin(gpu_api, bl, case):
    """0.5 s of noise: whole, in 4 096-frame chunks, and by block pulls of `bl` frames -- each inside the bound, and each
    restarted render bitwise the first."""
    p = FP.base_project("noise", bl=bl)
    FP.add_filter(p, "fl", "bus", case)
    built = build(gpu_api, p)
    n = p.cs * bl
    x = render_f32(gpu_api, built, "bus", p.cs)
    pw, end = twin(gpu_api, 48000, case, x)
    forms = {}
    forms["whole"] = [render_f32(gpu_api, built, "fl", p.cs) for _ in range(2)]
    forms["chunks"] = [render_f32(gpu_api, built, "fl", p.cs, max_chunk_frames=4096) for _ in range(2)]
    assert n / 4096 > 5
    built[2].set_option("max_chunk_frames", 1 << 24)
    forms["pulls"] = [_pull_all(gpu_api, built, "fl", p.cs) for _ in range(2)]
    for name, (a, b) in forms.items():
        assert a.shape == pw.shape
        close(a, x, pw, "%s bl %d" % (name, bl))
        assert np.array_equal(_bits(a), _bits(b)), name
    # the state really crosses the cuts: chunk 1 restarted from zero (at its own place on the LFO) is far outside the bound
    restart = twin(gpu_api, 48000, case, x[4096:8192], t0=4096)[0]
    assert np.abs(restart.astype(np.float64) - pw[4096:8192]).max() > 1e-3
    # a set_time in the middle of pulling restarts the state but NOT the LFO: two pulls, a jump, one pull -- the twin started
    # from zero at that absolute frame
    at = (4000 // bl) * bl
    got = []
    for out in ("fl", "bus"):
        sb, fb, g = p.build(gpu_api)
        assert g.set_output(out)
        for _ in range(2):
            g.render(sb, fb)
            fb.set_time_to_next_block()
        fb.set_time(at)
        g.set_time(at)
        got.append(np.stack(g.render(sb, fb), axis=1))
    assert np.abs(got[1]).max() > 0.01
    after = twin(gpu_api, 48000, case, got[1], t0=at)[0]
    close(got[0], got[1], after, "pull after set_time")
    # (the LFO restarted with the state would be another signal)
    assert np.abs(twin(gpu_api, 48000, case, got[1], t0=0)[0].astype(np.float64) - after).max() > 1e-4


@pytest.mark.parametrize("bl", [1, 7, 8, 9, NF.TILE - 1, NF.TILE, NF.TILE + 1, 3 * NF.TILE + 1])
def test_chunk_lengths_around_the_lane_and_the_tile(gpu_api, bl):
    """Three blocks of `bl` frames, rendered as one chunk and as three: one frame, a lane's run -1 / 0 / +1, a tile -1 / 0 / +1,
    three tiles and a frame."""
    p = FP.base_project("noise", bl=bl, seconds=(3.0 * bl - 0.5) / 48000.0)
    FP.add_filter(p, "fl", "bus", CASE)
    built = build(gpu_api, p)
    assert p.cs == 3
    x = render_f32(gpu_api, built, "bus", p.cs)
    pw, _ = twin(gpu_api, 48000, CASE, x)
    close(render_f32(gpu_api, built, "fl", p.cs), x, pw, "one chunk of 3 x %d" % bl)
    close(render_f32(gpu_api, built, "fl", p.cs, max_chunk_frames=bl), x, pw, "three chunks of %d" % bl)


def test_more_than_256_tiles(gpu_api):
    """12 s at 48 kHz of the looped noise: 576 512 frames, 282 tiles -- the follower's carries fold two tiles per lane, the
    filter's carry walks five batches."""
    p = FP.base_project("noise", seconds=12.0)
    FP.add_filter(p, "fl", "bus", CASE)
    built = build(gpu_api, p)
    n = p.cs * p.bl
    assert n == 576512 and (n + NF.TILE - 1) // NF.TILE == 282
    x = render_f32(gpu_api, built, "bus", p.cs)
    pw, _ = twin(gpu_api, 48000, CASE, x)
    close(render_f32(gpu_api, built, "fl", p.cs), x, pw, "282 tiles")


# ---- the key ----
def _keyed(api, bl=1024, case=CASE):
    p, key = KP.ducking_project("keybus", bl=bl)
    FP.add_filter(p, "self", "bus", case, key="bus")
    FP.add_filter(p, "plain", "bus", case)
    FP.add_filter(p, "keyed", "bus", case, key=key)
    return p, key, build(api, p)


@pytest.mark.parametrize("bl", [1024, 64])
def test_a_key_equal_to_the_input_is_the_unkeyed_vertex_bitwise(gpu_api, bl):
    p, _, built = _keyed(gpu_api, bl)
    for form in ("whole", "pulls"):
        a, b = ((render_f32(gpu_api, built, v, p.cs) if form == "whole" else _pull_all(gpu_api, built, v, p.cs)) for v in ("self", "plain"))
        assert np.array_equal(_bits(a), _bits(b)), form
    x = render_f32(gpu_api, built, "bus", p.cs)
    assert np.abs(render_f32(gpu_api, built, "plain", p.cs) - x).max() > 1e-3


@pytest.mark.parametrize("bl", [1024, 64])
def test_a_different_key_matches_the_twin_fed_that_key(gpu_api, bl):
    p, key, built = _keyed(gpu_api, bl)
    x, k = render_f32(gpu_api, built, "bus", p.cs), render_f32(gpu_api, built, key, p.cs)
    assert np.abs(k).max() > 0.05 and not np.array_equal(k, x)
    pw, _ = twin(gpu_api, 48000, CASE, x, key=k)
    forms = {"whole": render_f32(gpu_api, built, "keyed", p.cs), "chunks": render_f32(gpu_api, built, "keyed", p.cs, max_chunk_frames=4096)}
    built[2].set_option("max_chunk_frames", 1 << 24)
    forms["pulls"] = _pull_all(gpu_api, built, "keyed", p.cs)
    for name, y in forms.items():
        close(y, x, pw, "keyed, %s bl %d" % (name, bl))
    # (the key is really what the follower hears: the self-keyed twin is another signal)
    assert np.abs(twin(gpu_api, 48000, CASE, x)[0].astype(np.float64) - pw).max() > 1e-3


def test_env_oct_zero_ignores_the_key_bitwise(gpu_api):
    p, key = KP.ducking_project("keybus")
    FP.add_filter(p, "plain", "bus", STILL)
    FP.add_filter(p, "keyed", "bus", STILL, key=key)
    built = build(gpu_api, p)
    for opts in ({}, {"max_chunk_frames": 4096}):
        a, b = (render_f32(gpu_api, built, v, p.cs, **opts) for v in ("plain", "keyed"))
        assert np.array_equal(_bits(a), _bits(b)), opts
    g = built[2]
    g.set_option("max_chunk_frames", 1 << 24)
    g.set_profiling(1)
    render_f32(gpu_api, built, "keyed", p.cs)
    assert [n for n in g.kernel_times() if n.startswith("k_filt")] == FILTER   # (no follower launches)


def test_a_key_with_non_finite_frames_and_a_key_only_source(gpu_api):
    """The key is a loop that only the key edge reaches, with an infinity and a NaN in it: those frames enter the level as 0."""
    bl, cs = 1024, 12
    raw = W.noise_int16(9, 30011).astype(np.float32).reshape(-1).copy()   # interleaved 16-bit words as floats
    raw[2 * 5000] = np.inf
    raw[2 * 7000 + 1] = np.nan
    sb = gpu_api.SampleBank(48000)
    sb.add_decoded("a", raw, 2, 48000, 16, "")
    sb.add_decoded("b", W.noise_int16(11, 20011).astype(np.float32).reshape(-1), 2, 48000, 16, "")
    fb = gpu_api.FlowwBank(48000, bl)
    g = gpu_api.Graph(bl, 48000)
    g.add_sampleloop("k", 0.5, 0.0, sb.get_index("a"))
    g.add_sampleloop("l", 0.4, 0.0, sb.get_index("b"))
    g.add_sum("bus", 1.0, 0.0)
    g.add_filter("fl", 1.0, 0.0, 1.0, *CASE)
    assert g.connect("l", "bus") and g.connect("bus", "fl") and g.connect_key("k", "fl")
    built = (sb, fb, g)
    x, k = render_f32(gpu_api, built, "bus", cs), render_f32(gpu_api, built, "k", cs)
    assert (~np.isfinite(k)).sum() == 2 and np.isfinite(x).all()
    y = render_f32(gpu_api, built, "fl", cs)
    assert np.isfinite(y).all()
    close(y, x, twin(gpu_api, 48000, CASE, x, key=k)[0], "non-finite key frames")


def test_a_non_finite_input_frame_is_non_finite_at_that_frame_only(gpu_api):
    bl, cs = 1024, 12
    raw = W.noise_int16(9, 30011).astype(np.float32).reshape(-1).copy()
    raw[2 * 5000] = np.inf          # frame 5 000, left
    raw[2 * 7000 + 1] = np.nan      # frame 7 000, right
    sb = gpu_api.SampleBank(48000)
    sb.add_decoded("a", raw, 2, 48000, 16, "")
    fb = gpu_api.FlowwBank(48000, bl)
    g = gpu_api.Graph(bl, 48000)
    g.add_sampleloop("l", 0.5, 0.0, sb.get_index("a"))
    g.add_sum("bus", 1.0, 0.0)
    g.add_filter("fl", 1.0, 0.0, 1.0, *CASE)
    assert g.connect("l", "bus") and g.connect("bus", "fl")
    built = (sb, fb, g)
    x = render_f32(gpu_api, built, "bus", cs)
    assert (~np.isfinite(x)).sum() == 2 and not np.isfinite(x[5000, 0]) and not np.isfinite(x[7000, 1])
    y = render_f32(gpu_api, built, "fl", cs)
    assert (np.isfinite(y) == np.isfinite(x)).all()   # only the input's own non-finite samples
    pw, end = twin(gpu_api, 48000, CASE, x)
    ok = np.isfinite(x).all(axis=1)
    close(y[ok], x[ok], pw[ok], "around non-finite frames")
    assert np.isfinite(end).all()


# ---- the mix ----
@pytest.mark.parametrize("wet,gain,angle", MIX)
def test_wet_pan_and_gain(gpu_api, wet, gain, angle):
    p = FP.base_project("drums")
    FP.add_filter(p, "fl", "bus", CASE, wet=wet, gain=gain, angle=angle)
    built = build(gpu_api, p)
    x = render_f32(gpu_api, built, "bus", p.cs)
    y = render_f32(gpu_api, built, "fl", p.cs)
    sp = FP.spec(gpu_api, 48000, CASE)
    want, _ = NF.process(x, sp, wet=wet, gain=gain, angle=angle)
    proc, _ = NF.process(x, sp, processed=True)
    lim = mix_bound(x, proc, gain, angle)
    err = np.abs(y.astype(np.float64) - want.astype(np.float64))
    print("wet %g gain %g angle %g: worst error / bound %.3g" % (wet, gain, angle, float(np.max(err / lim))))
    assert (err <= lim).all(), (float(np.max(err / lim)), np.argwhere(err > lim)[:4].tolist())
    assert np.abs(want - x).max() > 1e-3 * wet   # (the vertex does something, in proportion to the mix)


def test_dry_passes_the_input_through_as_a_sum_launch(gpu_api):
    p, key = KP.ducking_project("keybus")
    FP.add_filter(p, "dry", "bus", CASE, wet=0.0, key=key)
    FP.add_filter(p, "almost", "bus", CASE, wet=0.00009)
    FP.add_filter(p, "wet", "bus", CASE)
    built = build(gpu_api, p)
    x = render_f32(gpu_api, built, "bus", p.cs)
    for name in ("dry", "almost"):
        y = render_f32(gpu_api, built, name, p.cs)
        assert np.array_equal(y, x), (name, np.argwhere(y != x)[:4].tolist())
    g = built[2]
    g.set_profiling(1)
    render_f32(gpu_api, built, "dry", p.cs)
    names = list(g.kernel_times())
    assert not any(n.startswith("k_filt") for n in names) and "k_sum" in names, names   # wet < 0.0001: a plain sum launch
    render_f32(gpu_api, built, "wet", p.cs)
    assert [n for n in g.kernel_times() if n.startswith("k_filt")] == FOLLOWER + FILTER
    # a chunk of one tile is k_filt_apply alone
    q = FP.base_project("drums", seconds=0.04)
    FP.add_filter(q, "wet", "bus", CASE)
    q.set_output("wet")
    assert q.cs * q.bl == NF.TILE
    sb, fb, g = q.build(gpu_api)
    g.set_profiling(1)
    g.render_all(sb, fb, q.cs, 16, want_f32=False)
    assert [n for n in g.kernel_times() if n.startswith("k_filt")] == ["k_filt_apply"]


# ---- placement ----
def test_in_front_of_a_normalize_output(gpu_api):
    p = FP.base_project("drums", seconds=1.0)
    FP.add_filter(p, "fl", "bus", CASE)
    p.add_normalize("out", 1.0, 0.0)
    p.connect("fl", "out")
    built = build(gpu_api, p)
    x = render_f32(gpu_api, built, "bus", p.cs)
    c = render_f32(gpu_api, built, "fl", p.cs)
    close(c, x, twin(gpu_api, 48000, CASE, x)[0], "in front of Normalize")
    # normalize_gen (extensions.rs:321-329) on what the filter really handed on: the running block peak from 1e-6, f32
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
    p = FP.base_project("drums", seconds=1.0)
    FP.add_filter(p, "f1", "bus", CASE)
    FP.add_filter(p, "f2", "f1", CASE_HP, gain=0.8, angle=-20.0)
    p.add_sum("post", 0.5, 10.0)
    p.connect("f2", "post")
    built = build(gpu_api, p)
    x = render_f32(gpu_api, built, "bus", p.cs)
    y1 = render_f32(gpu_api, built, "f1", p.cs)
    close(y1, x, twin(gpu_api, 48000, CASE, x)[0], "first of two")
    # the second one against the twin on what the first one really handed it
    y2 = render_f32(gpu_api, built, "f2", p.cs)
    s2 = FP.spec(gpu_api, 48000, CASE_HP)
    w2, _ = NF.process(y1, s2, gain=0.8, angle=-20.0)
    proc, _ = NF.process(y1, s2, processed=True)
    assert (np.abs(y2.astype(np.float64) - w2) <= mix_bound(y1, proc, 0.8, -20.0)).all()
    # both as stems of a render whose output sits downstream
    sb, fb, g = built
    g.set_output("post")
    g.set_stems(["f2", "f1"])
    fb.set_time(0)
    g.set_time(0)
    g.render_all(sb, fb, p.cs, 16)
    assert np.abs(g.read_stem_pcm(0).astype(np.int64) - _quantise16(y2)).max() == 0
    assert np.abs(g.read_stem_pcm(1).astype(np.int64) - _quantise16(y1)).max() == 0
    g.set_stems([])


def test_fed_by_an_inlined_loop_source_and_a_gain_stage(gpu_api):
    p = W.ProjectScript(48000, 1024)
    p.set_length(0.5)
    p.assets["a0"] = W.Asset(W.noise_int16(50, 20011))
    p.assets["a1"] = W.Asset(W.noise_int16(51, 9001))
    p.load_sample("a0", "a0", "")
    p.load_sample("a1", "a1", "normalize-seperate")
    p.add_sampleloop("l0", 0.7, 30.0, "a0")     # read by the filter itself (term kinds 1 / 3)
    p.add_sampleloop("l1", 0.02, 0.0, "a1")
    p.add_sum("stage", 0.5, -45.0)              # one input: a gain / pan stage, read through (term kind 4)
    p.connect("l1", "stage")
    FP.add_filter(p, "fl", "l0", CASE)
    p.connect("stage", "fl")
    p.set_output("fl")
    built = p.build(gpu_api)
    a = render_f32(gpu_api, built, "l0", p.cs)
    b = render_f32(gpu_api, built, "stage", p.cs)
    x = (np.float32(0.0) + a) + b               # sum_inputs (extensions.rs:310-319), f32, in connect() order
    pw, _ = twin(gpu_api, 48000, CASE, x)
    for packed in (1, 0):
        y = render_f32(gpu_api, built, "fl", p.cs, packed_samples=packed)
        close(y, x, pw, "inlined terms, packed_samples %d" % packed)


def test_batch_members_are_bitwise_their_own_renders(gpu_api):
    projects = []
    cases = FP.grid_cases(48000)
    for i in range(8):
        p, key = KP.ducking_project("keybus", seconds=1.0) if i % 2 else (FP.base_project(FP.INPUTS[i % 3], seconds=1.0, seed=i), None)
        c = cases[(13 * i + 5) % len(cases)]
        FP.add_filter(p, "fl", "bus", c, wet=[1.0, 0.6][(i // 2) % 2], gain=[1.0, 0.7][(i // 4) % 2], key=key)
        if i % 4 == 1:     # a second one in series, as the output
            FP.add_filter(p, "fl2", "fl", cases[(29 * i + 1) % len(cases)])
            p.set_output("fl2")
        elif i % 4 == 2:   # in front of a Normalize output
            p.add_normalize("out", 1.0, 0.0)
            p.connect("fl", "out")
            p.set_output("out")
        else:
            p.set_output("fl")
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
    batch = gpu_api.Batch()
    for p in projects:
        batch.add(*p.build(gpu_api))
    for rep in range(2):
        batch.rewind()
        assert batch.render_all(cs, 16) == cs * 1024
        for i in range(8):
            assert np.array_equal(batch.read_pcm(i, cs), own[i][rep]), (rep, i)


def test_projects_without_a_filter_launch_no_filter_kernel(gpu_api):
    for p in (W.drum_project(seconds=1.0), W.config2(seconds=1.0, n_src=8)):
        sb, fb, g = p.build(gpu_api)
        g.set_profiling(1)
        g.render_all(sb, fb, p.cs, 16, want_f32=False)
        names = list(g.kernel_times())
        assert names and not any(n.startswith("k_filt") for n in names), names


# ---- the guard modes ----
def _guard_project(shape):
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
    p.add_filter("fl", 1.0, 0.0, 1.0, *(STILL if shape == "key_unheard" else CASE))
    if shape == "down":   # loop -> filter -> band-pass chain; the synth joins behind the filter
        p.connect("s", "fl"); p.connect("fl", "b1"); p.connect("b1", "b2"); p.connect("b2", "bus"); p.connect("y", "bus")
        p.set_output("bus")
    elif shape == "up":   # band-pass chain and synth -> bus -> filter
        p.connect("s", "b1"); p.connect("b1", "b2"); p.connect("b2", "bus"); p.connect("y", "bus"); p.connect("bus", "fl")
        p.set_output("fl")
    else:                 # the band-pass chain and the synth are the KEY of a filter on the loop; the output hears them too
        p.add_sampleloop("s2", 0.3, 0.0, "a")
        p.add_sum("out", 1.0, 0.0)
        p.connect("s", "b1"); p.connect("b1", "b2"); p.connect("b2", "bus"); p.connect("y", "bus")
        p.connect("s2", "fl"); p.connect_key("bus", "fl"); p.connect("fl", "out"); p.connect("bus", "out")
        p.set_output("out")
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


def test_guard_keeps_the_scan_and_fast_sines_downstream_of_a_filter(gpu_api):
    outs, names = _guard_renders(gpu_api, _guard_project("down"))
    rms = float(np.sqrt(np.mean((outs["guard"].astype(np.float64) - outs["exact"].astype(np.float64)) ** 2)))
    print("guarded scan + fast sines downstream of a filter: rms %.3g against the exact forms" % rms)
    assert rms <= 1e-6 and np.abs(outs["exact"]).max() > 0.05
    assert "k_band_scan" in names["guard"] and "k_sine_probe" in names["guard"], names["guard"]
    assert not any(n in names["guard"] for n in ("k_band_pass", "k_band_spec")), names["guard"]
    assert [n for n in names["guard"] if n.startswith("k_filt")] == FOLLOWER + FILTER


@pytest.mark.parametrize("shape", ["up", "key"])
def test_guard_renders_the_exact_forms_upstream_of_a_filter_and_of_its_key(gpu_api, shape):
    outs, names = _guard_renders(gpu_api, _guard_project(shape))
    assert np.array_equal(_bits(outs["guard"]), _bits(outs["exact"])) and np.abs(outs["exact"]).max() > 0.05
    assert "k_band_scan" not in names["guard"] and "k_sine_probe" not in names["guard"], names["guard"]
    assert any(n in names["guard"] for n in ("k_band_pass", "k_band_spec")), names["guard"]


def test_guard_carries_its_estimate_past_a_key_that_no_follower_hears(gpu_api):
    """env_oct == 0: the key edge is ignored, so the band-pass chain upstream of it keeps the scan."""
    outs, names = _guard_renders(gpu_api, _guard_project("key_unheard"))
    assert "k_band_scan" in names["guard"] and "k_sine_probe" in names["guard"], names["guard"]
    assert [n for n in names["guard"] if n.startswith("k_filt")] == FILTER


# ---- the front end ----
def test_front_end_renders_a_drum_bus_with_a_keyed_filter(gpu_api, tmp_path):
    fl = ("wah", 1.0, 0.0, 0.8, "lowpass", 300.0, 6.0, 1.0, 2.0, 0.25, "sine", 5.0, 12.0, 1.0, 120.0)
    p = W.drum_project(seconds=1.0)
    # the drum bus `drums` feeds the band-pass in front of the output: put the filter in between, keyed by the kick band
    i = p.calls["connect"].index(("drums", "band"))
    p.calls["connect"][i:i + 1] = [("drums", "wah"), ("wah", "band")]
    j = p.script_order.index(("connect", ("drums", "band")))
    p.script_order[j:j + 1] = [("add_filter", fl), ("connect", ("drums", "wah")), ("connect", ("wah", "band")), ("connect_key", ("kickband", "wah"))]
    p.calls["add_filter"].append(fl)
    p.calls["connect_key"].append(("kickband", "wah"))
    d = str(tmp_path / "proj")
    _write_project(p, d)
    out = str(tmp_path / "m.wav")
    r = subprocess.run([sys.executable, "-m", "termdaw_amd", d, "-o", out], env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    st = gpu_api.State(open_dir=d)
    assert st.refresh(), gpu_api.last_error()
    dump = st.dump_calls()
    assert 'add_filter("wah",' in dump and 'connect_key("kickband","wah")' in dump
    mem = st.render_to_memory()
    with wave.open(out, "rb") as w:
        words = np.frombuffer(w.readframes(w.getnframes()), np.int16).reshape(-1, 2)
    assert words.shape == mem.shape and np.array_equal(words, mem) and np.abs(mem).max() > 1000
    # ... and the filter is really in the path: without it the words differ
    q = W.drum_project(seconds=1.0)
    d2 = str(tmp_path / "plain")
    _write_project(q, d2)
    st2 = gpu_api.State(open_dir=d2)
    assert st2.refresh()
    assert not np.array_equal(st2.render_to_memory(), mem)
