"""The filter vertex on the device (td_graph_add_filter) against its float64 twin (tests/np_filter.py, the serial
restatement of the definition in include/termdaw_amd.h), run on the engine's own constants (td_filter_params).

The input of the vertex under test -- and its key -- always come from the engine itself: further renders of the same graph with
set_output on the vertex in front, read as f32 -- the oracle-verified part of the graph is not restated here.

Bounds.  wet = 1, gain = 1, angle = 0, per value:  |p' - p| <= 2^-23 |p| + E max|p| on the filter's output p, carried through the
definition's f32 lerp to the vertex' output (fx_rig.assert_close says why it is not asserted on the output as it stands).
The first term is the one f32 rounding of p, which may flip; E covers the float64 re-association of the scans, the follower's
included: 8 x what the numpy emulation of the tiled scans shows over this file's own grid and inputs (tests/filter_projects.py E,
derived and re-checked on the CPU by tests/test_filter_host.py; far under the cap 2^-28).  g[n] is the same bits on both sides
where e[n] is: IEEE add, multiply, floor, fabs, min and max on the same constants, and one correctly rounded division.
With wet in (0, 1), pan and gain: 4 x 2^-23 x max(|dry|, |p|) x |amplitude| absolute, as for the EQ.

Every case prints its worst error over the bound; DESIGN.md §3w records how many cases came out bit-identical."""
import os
import sys

import numpy as np
import pytest

from termdaw_amd import workloads as W

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fx_rig  # noqa: E402
import filter_projects as FP  # noqa: E402
import key_projects as KP  # noqa: E402
import np_filter as NF  # noqa: E402
from fx_rig import MIX, REL, _guard_renders, _pull_all, assert_close, build, render_f32  # noqa: E402

pytestmark = pytest.mark.gpu
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


FILT = fx_rig.FxKind("filter", "k_filt", FOLLOWER + FILTER, FP.add_filter, FP.base_project, CASE, CASE_HP, FP.E,
                     twin=lambda api, sr, case, x: (twin(api, sr, case, x)[0], x),
                     mix=lambda api, sr, case, x, **kw: NF.process(x, FP.spec(api, sr, case), **kw)[0])


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
    fx_rig.wet_pan_and_gain(gpu_api, FILT, wet, gain, angle, vertex="fl")


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
    fx_rig.in_front_of_a_normalize_output(gpu_api, FILT, vertex="fl")


def test_as_a_stem_and_two_in_series(gpu_api):
    fx_rig.as_a_stem_and_two_in_series(gpu_api, FILT, "f1", "f2")


def test_fed_by_an_inlined_loop_source_and_a_gain_stage(gpu_api):
    fx_rig.fed_by_an_inlined_loop_source_and_a_gain_stage(gpu_api, FILT, CASE, W.noise_int16(50, 20011), vertex="fl")


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
    # (every other project is the same ducking project: the first renders are not all different)
    fx_rig.batch_matches_own_renders(gpu_api, projects, distinct=False)


def test_projects_without_a_filter_launch_no_filter_kernel(gpu_api):
    fx_rig.projects_without_the_kind_launch_no_kernel_of_it(gpu_api, "k_filt")


# ---- the guard modes ----
def _guard_project(shape):
    p = fx_rig.gpu_guard_base()
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


def test_guard_keeps_the_scan_and_fast_sines_downstream_of_a_filter(gpu_api):
    fx_rig.guard_keeps_the_scan_and_fast_sines_downstream(gpu_api, _guard_project("down"), "filter", "k_filt", FOLLOWER + FILTER)


@pytest.mark.parametrize("shape", ["up", "key"])
def test_guard_renders_the_exact_forms_upstream_of_a_filter_and_of_its_key(gpu_api, shape):
    fx_rig.guard_renders_the_exact_forms_upstream(gpu_api, _guard_project(shape))


def test_guard_carries_its_estimate_past_a_key_that_no_follower_hears(gpu_api):
    """env_oct == 0: the key edge is ignored, so the band-pass chain upstream of it keeps the scan."""
    outs, names = _guard_renders(gpu_api, _guard_project("key_unheard"))
    assert "k_band_scan" in names["guard"] and "k_sine_probe" in names["guard"], names["guard"]
    assert [n for n in names["guard"] if n.startswith("k_filt")] == FILTER


# ---- the front end ----
def test_front_end_renders_a_drum_bus_with_a_keyed_filter(gpu_api, tmp_path):
    # the drum bus `drums` feeds the band-pass in front of the output: put the filter in between, keyed by the kick band
    fl = ("wah", 1.0, 0.0, 0.8, "lowpass", 300.0, 6.0, 1.0, 2.0, 0.25, "sine", 5.0, 12.0, 1.0, 120.0)
    p = fx_rig.into_the_drum_bus("add_filter", fl, key="kickband")
    mem = fx_rig.front_end_renders(gpu_api, tmp_path, p, 'add_filter("wah",', 'connect_key("kickband","wah")')
    fx_rig.front_end_words_differ(gpu_api, tmp_path, W.drum_project(seconds=1.0), mem)
