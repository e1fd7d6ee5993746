"""The limiter vertex on the device (td_graph_add_limiter) against its float64 twin (tests/np_limiter.py, the
serial restatement of the definition in include/termdaw_amd.h), run on the engine's own constants (td_limiter_params).

The input of the vertex under test always comes from the engine itself: a second render of the same graph with set_output on
the vertex in front, read as f32 -- the oracle-verified part of the graph is not restated here.

Bounds.  wet = 1, gain = 1, angle = 0, per value:  |p' - p| <= 2^-23 |p| + E max|p| on the limited signal p, carried through the
definition's f32 lerp against the DELAYED input xd to the vertex' output (fx_rig.assert_close says why it is not asserted on
the output as it stands).  The first term is the one f32 rounding of the chain, which may flip; E covers the float64 order of the
release scan and of the prefix sums behind G: 8 x what the numpy emulation of the kernels' order shows over this file's own grid
and inputs (tests/limiter_projects.py E, derived and re-checked on the CPU by tests/test_limiter_host.py; E = 3.2e-10, under the
cap 2^-28).  Q is exact on both sides.  The ceiling is asserted on the device's own output, through the same lerp: no wet-path
value above c (1 + 2^-22).
With wet in (0, 1), pan and gain: 4 x 2^-23 x max(|dry|, |p|) x |amplitude| absolute, as for the EQ.  PCM cases: within one word
of the twin's quantised value.

Every case prints its worst error over the bound; DESIGN.md §3x records how many cases came out bit-identical."""
import os
import sys

import numpy as np
import pytest

from termdaw_amd import workloads as W

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fx_rig  # noqa: E402
import limiter_projects as LP  # noqa: E402
import np_limiter as NL  # noqa: E402
from fx_rig import MIX, _f32_down, _pull_all, assert_close, build, render_f32  # noqa: E402

pytestmark = pytest.mark.gpu
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


LIMITER = fx_rig.FxKind("limiter", "k_lim", LIM_LAUNCHES, LP.add_limiter, LP.base_project, CASE, (-12.0, 0.0, 5.0, 0.0), LP.E,
                        twin=lambda api, sr, case, x: twin(api, sr, case, x)[:2],
                        mix=lambda api, sr, case, x, **kw: NL.process(x, api.limiter_params(sr, *case), **kw)[0],
                        acts=lambda proc, xd: np.abs(proc - xd).max() > 1e-3)


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
    fx_rig.wet_pan_and_gain(gpu_api, LIMITER, wet, gain, angle, vertex="m", seconds=0.5)


def test_dry_passes_the_input_through_undelayed(gpu_api):
    fx_rig.dry_passes_the_input_through(gpu_api, LIMITER, seconds=0.5)


# ---- placement ----
def test_in_front_of_a_normalize_output(gpu_api):
    fx_rig.in_front_of_a_normalize_output(gpu_api, LIMITER, vertex="m")


def test_as_a_stem_and_two_in_series(gpu_api):
    fx_rig.as_a_stem_and_two_in_series(gpu_api, LIMITER, "m1", "m2")


def test_fed_by_an_inlined_loop_source_and_a_gain_stage(gpu_api):
    import gate_projects as GP
    case = (-12.0, 2.0, 30.0, 6.0)

    def works_and_its_gain_moves(x):
        G = twin(gpu_api, 48000, case, x)[2]
        assert G.min() < 0.7 and G.max() - G.min() > 0.2
    fx_rig.fed_by_an_inlined_loop_source_and_a_gain_stage(gpu_api, LIMITER, case, GP.gated_int16(3), vertex="m", check=works_and_its_gain_moves)


def test_batch_members_are_bitwise_their_own_renders(gpu_api):
    # (`noise` has a source called m: the limiters are lm)
    fx_rig.batch_members_are_bitwise_their_own_renders(gpu_api, LIMITER, LP.INPUTS, [c for c, _ in LP.grid_cases(48000)], vertex="lm")


def test_projects_without_a_limiter_launch_no_limiter_kernel(gpu_api):
    fx_rig.projects_without_the_kind_launch_no_kernel_of_it(gpu_api, "k_lim")
    sb, fb, g = fx_rig.a_whole_render_launches_the_kinds_kernels(gpu_api, LIMITER, vertex="m")
    # a render of one tile (2 048 frames) is k_lim_apply alone, as every block pull is
    g.set_time(0)
    fb.set_time(0)
    g.set_profiling(1)   # (the times add up over renders until profiling is set again)
    g.render_all(sb, fb, 2, 16, want_f32=False)
    assert [n for n in g.kernel_times() if n.startswith("k_lim")] == ["k_lim_apply"]


# ---- the guard modes ----
def _guard_project(limiter_first):
    return fx_rig.gpu_guard_project("add_limiter", "m", (-12.0, 5.0, 80.0, 6.0), limiter_first)


def test_guard_keeps_the_scan_and_fast_sines_downstream_of_a_limiter(gpu_api):
    fx_rig.guard_keeps_the_scan_and_fast_sines_downstream(gpu_api, _guard_project(True), "limiter", "k_lim", LIM_LAUNCHES)


def test_guard_renders_the_exact_forms_upstream_of_a_limiter(gpu_api):
    fx_rig.guard_renders_the_exact_forms_upstream(gpu_api, _guard_project(False))


# ---- the front end ----
def test_front_end_renders_a_limited_drum_bus(gpu_api, tmp_path):
    mem = fx_rig.front_end_renders(gpu_api, tmp_path, W.limiter_project(seconds=1.0), 'add_limiter("lim",')
    # the ceiling holds on the words: -1 dB of full scale
    assert np.abs(mem.astype(np.int64)).max() <= int(10.0 ** (-1.0 / 20.0) * 32767.0) + 1
    # ... and the limiter is really in the path: with it dry the words differ
    fx_rig.front_end_words_differ(gpu_api, tmp_path, W.limiter_project(seconds=1.0, wet=0.0), mem)
