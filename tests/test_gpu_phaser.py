"""The phaser vertex on the device (td_graph_add_phaser) against its float64 twin (tests/np_phaser.py, the serial
restatement of the definition in include/termdaw_amd.h), run on the engine's own constants (td_phaser_params).

The input of the vertex under test always comes from the engine itself: a second render of the same graph with set_output on
the vertex in front, read as f32 -- the oracle-verified part of the graph is not restated here.

Bounds.  wet = 1, gain = 1, angle = 0, per value:  |p' - p| <= 2^-23 |p| + E max|p| on the chain's output p, carried through the
definition's f32 lerp to the vertex' output (fx_rig.assert_close says why it is not asserted on the output as it stands).
The first term is the one f32 rounding of the chain, which may flip; E covers the float64 re-association of the scan: 8 x what
the numpy emulation of the tiled scan shows over this file's own grid and inputs (tests/phaser_projects.py E, derived and
re-checked on the CPU by tests/test_phaser_host.py; far under the cap 2^-28).  a[n] is the same bits on both sides: IEEE add,
multiply, floor and fabs on the same constants.
With wet in (0, 1), pan and gain: 4 x 2^-23 x max(|dry|, |p|) x |amplitude| absolute, as for the EQ.  PCM cases: within one word
of the twin's quantised value.

Every case prints its worst error over the bound; DESIGN.md §3u records how many cases came out bit-identical."""
import os
import sys

import numpy as np
import pytest

from termdaw_amd import workloads as W

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fx_rig  # noqa: E402
import np_phaser as NP  # noqa: E402
import phaser_projects as PP  # noqa: E402
from fx_rig import MIX, REL, _pull_all, assert_close, build, render_f32  # noqa: E402

pytestmark = pytest.mark.gpu
PHASER_LAUNCHES = ["k_phaser_local", "k_phaser_carry", "k_phaser_apply"]
CASE = (4, 200.0, 2000.0, 1.0, 0.7, 0.25, "sine")   # stages, lo, hi, rate, feedback, stereo, shape
CASE8 = (8, 300.0, 6000.0, 0.5, -0.9, 0.5, "triangle")


def twin(api, sr, case, x, state=None, t0=0):
    """(p float32, end state) of the serial twin on the engine's constants."""
    v, end = NP.serial(x, PP.spec(api, sr, case), state, t0)
    return v.astype(np.float32), end


def close(y, x, p, what):
    return assert_close(y, x, p, what, PP.E)


PHASER = fx_rig.FxKind("phaser", "k_phaser", PHASER_LAUNCHES, PP.add_phaser, PP.base_project, CASE, CASE8, PP.E,
                       twin=lambda api, sr, case, x: (twin(api, sr, case, x)[0], x),
                       mix=lambda api, sr, case, x, **kw: NP.process(x, PP.spec(api, sr, case), **kw)[0])


# ---- the grid ----
@pytest.mark.parametrize("sr", PP.RATES)
@pytest.mark.parametrize("kind", PP.INPUTS)
def test_grid_matches_the_twin(gpu_api, sr, kind):
    cases = PP.grid_cases(sr)
    assert len(cases) == 108
    p = PP.base_project(kind, sr=sr)
    for i, c in enumerate(cases):
        PP.add_phaser(p, "p%d" % i, "bus", c)
    built = build(gpu_api, p)
    x = render_f32(gpu_api, built, "bus", p.cs)
    n = p.cs * p.bl
    assert np.abs(x).max() > 0.05 and n > 5 * NP.TILE
    worst, exact, acts = 0.0, 0, 0
    for N in (2, 4, 6, 8):
        idx = [i for i, c in enumerate(cases) if c[0] == N]
        vs, _ = NP.serial(x, [PP.spec(gpu_api, sr, cases[i]) for i in idx])   # (the cases of one stage count side by side)
        for i, v in zip(idx, vs):
            pw = v.astype(np.float32)
            y = render_f32(gpu_api, built, "p%d" % i, p.cs)
            worst = max(worst, close(y, x, pw, "%s %d %s" % (kind, sr, cases[i])))
            want = x + np.float32(1.0) * (pw - x)
            exact += int(np.array_equal(y.view(np.uint32), want.view(np.uint32)))
            acts += int(np.abs(want.astype(np.float64) - x).max() > 64.0 * (REL + PP.E) * np.abs(x).max())
    print("grid %s %d: %d cases, worst |y - want| %.3g x the plain bound, %d bit-identical to the twin" % (kind, sr, len(cases), worst, exact))
    assert acts == len(cases), acts   # (every case moves the signal: an all-pass chain turns every partial's phase)
    assert np.array_equal(render_f32(gpu_api, built, "bus", p.cs), x)   # (and every render above saw this input)


# ---- chunks, pulls, restarts ----
@pytest.mark.parametrize("bl", [1024, 64])
def test_chunked_and_pulled_renders_match_the_twin(gpu_api, bl):
    """0.5 s of noise: whole, in 4 096-frame chunks, and by block pulls of `bl` frames -- each inside the bound, and each
    restarted render bitwise the first."""
    p = PP.base_project("noise", bl=bl)
    PP.add_phaser(p, "ph", "bus", CASE)
    built = build(gpu_api, p)
    n = p.cs * bl
    x = render_f32(gpu_api, built, "bus", p.cs)
    pw, end = twin(gpu_api, 48000, CASE, x)
    forms = {}
    forms["whole"] = [render_f32(gpu_api, built, "ph", p.cs) for _ in range(2)]
    forms["chunks"] = [render_f32(gpu_api, built, "ph", p.cs, max_chunk_frames=4096) for _ in range(2)]
    assert n / 4096 > 5
    built[2].set_option("max_chunk_frames", 1 << 24)
    forms["pulls"] = [_pull_all(gpu_api, built, "ph", p.cs) for _ in range(2)]
    for name, (a, b) in forms.items():
        assert a.shape == pw.shape
        close(a, x, pw, "%s bl %d" % (name, bl))
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), name
    # the state really crosses the cuts: chunk 1 restarted from zero (at its own place on the LFO) is far outside the bound
    restart = twin(gpu_api, 48000, CASE, x[4096:8192], t0=4096)[0]
    assert np.abs(restart.astype(np.float64) - pw[4096:8192]).max() > 1e-3
    # a set_time in the middle of pulling restarts the state but NOT the LFO: two pulls, a jump, one pull -- the twin started
    # from zero at that absolute frame
    at = (4000 // bl) * bl
    got = []
    for out in ("ph", "bus"):
        sb, fb, g = p.build(gpu_api)
        assert g.set_output(out)
        for _ in range(2):
            g.render(sb, fb)
            fb.set_time_to_next_block()
        fb.set_time(at)
        g.set_time(at)
        got.append(np.stack(g.render(sb, fb), axis=1))
    assert np.abs(got[1]).max() > 0.01
    after = twin(gpu_api, 48000, CASE, got[1], t0=at)[0]
    close(got[0], got[1], after, "pull after set_time")
    # (the LFO restarted with the state would be another signal)
    assert np.abs(twin(gpu_api, 48000, CASE, got[1], t0=0)[0].astype(np.float64) - after).max() > 1e-4


def test_more_than_256_tiles(gpu_api):
    """12 s at 48 kHz of the looped noise input, 8 stages: 576 512 frames, 282 tiles in series through k_phaser_carry."""
    p = PP.base_project("noise", seconds=12.0)
    PP.add_phaser(p, "ph", "bus", CASE8)
    built = build(gpu_api, p)
    n = p.cs * p.bl
    assert n == 576512 and (n + NP.TILE - 1) // NP.TILE == 282
    x = render_f32(gpu_api, built, "bus", p.cs)
    pw, _ = twin(gpu_api, 48000, CASE8, x)
    y = render_f32(gpu_api, built, "ph", p.cs)
    close(y, x, pw, "282 tiles")


# ---- the mix ----
@pytest.mark.parametrize("wet,gain,angle", MIX)
def test_wet_pan_and_gain(gpu_api, wet, gain, angle):
    fx_rig.wet_pan_and_gain(gpu_api, PHASER, wet, gain, angle, vertex="ph")


def test_dry_passes_the_input_through_as_a_sum_launch(gpu_api):
    fx_rig.dry_passes_the_input_through(gpu_api, PHASER)


# ---- placement ----
def test_in_front_of_a_normalize_output(gpu_api):
    fx_rig.in_front_of_a_normalize_output(gpu_api, PHASER, vertex="ph")


def test_as_a_stem_and_two_in_series(gpu_api):
    fx_rig.as_a_stem_and_two_in_series(gpu_api, PHASER, "p1", "p2")


def test_fed_by_an_inlined_loop_source_and_a_gain_stage(gpu_api):
    fx_rig.fed_by_an_inlined_loop_source_and_a_gain_stage(gpu_api, PHASER, CASE, W.noise_int16(50, 20011), vertex="ph")


def test_batch_members_are_bitwise_their_own_renders(gpu_api):
    fx_rig.batch_members_are_bitwise_their_own_renders(gpu_api, PHASER, PP.INPUTS, PP.grid_cases(48000), vertex="ph")


def test_projects_without_a_phaser_launch_no_phaser_kernel(gpu_api):
    fx_rig.projects_without_the_kind_launch_no_kernel_of_it(gpu_api, "k_phaser")
    fx_rig.a_whole_render_launches_the_kinds_kernels(gpu_api, PHASER, vertex="ph")
    # a chunk of one tile is k_phaser_apply alone
    p = PP.base_project("drums", seconds=0.04)
    PP.add_phaser(p, "ph", "bus", CASE)
    p.set_output("ph")
    assert p.cs * p.bl == NP.TILE
    sb, fb, g = p.build(gpu_api)
    g.set_profiling(1)
    g.render_all(sb, fb, p.cs, 16, want_f32=False)
    assert [n for n in g.kernel_times() if n.startswith("k_phaser")] == ["k_phaser_apply"]


# ---- the guard modes ----
def _guard_project(phaser_first):
    return fx_rig.gpu_guard_project("add_phaser", "ph", CASE, phaser_first)


def test_guard_keeps_the_scan_and_fast_sines_downstream_of_a_phaser(gpu_api):
    fx_rig.guard_keeps_the_scan_and_fast_sines_downstream(gpu_api, _guard_project(True), "phaser", "k_phaser", PHASER_LAUNCHES)


def test_guard_renders_the_exact_forms_upstream_of_a_phaser(gpu_api):
    fx_rig.guard_renders_the_exact_forms_upstream(gpu_api, _guard_project(False))


# ---- the front end ----
def test_front_end_renders_a_drum_bus_with_a_phaser(gpu_api, tmp_path):
    # the drum bus `drums` feeds the band-pass in front of the output: put the phaser in between
    p = fx_rig.into_the_drum_bus("add_phaser", ("phaser", 1.0, 0.0, 0.5, 4, 200.0, 2000.0, 1.0, 0.7, 0.25, "sine"))
    mem = fx_rig.front_end_renders(gpu_api, tmp_path, p, 'add_phaser("phaser",')
    fx_rig.front_end_words_differ(gpu_api, tmp_path, W.drum_project(seconds=1.0), mem)
