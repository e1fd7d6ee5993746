"""The gate vertex on the device (td_graph_add_gate) against its float64 twin (tests/np_gate.py, the serial
restatement of the definition in include/termdaw_amd.h), run on the engine's own constants (td_gate_params).

The input of the vertex under test always comes from the engine itself: a second render of the same graph with set_output on
the vertex in front, read as f32 -- the oracle-verified part of the graph is not restated here.

Bounds.  wet = 1, gain = 1, angle = 0, per value:  |p' - p| <= 2^-23 |p| + E max|p| on the gated signal p, carried through the
definition's f32 lerp to the vertex' output (fx_rig.assert_close says why it is not asserted on the output as it stands).
The first term is the one f32 rounding of the chain, which may flip; E covers the float64 re-association of the fade's scan: 8 x
what the numpy emulation of the tiled scan shows over this file's own grid and inputs (tests/gate_projects.py E, derived and
re-checked on the CPU by tests/test_gate_host.py; E = 2e-12, far under the cap 2^-28).  The open / closed decision is exact on
both sides; a wrong one moves p by a factor of up to 1 / F (10 at range_db -20, 10^6 at -120), so the bound cannot hide one.
With wet in (0, 1), pan and gain: 4 x 2^-23 x max(|dry|, |p|) x |amplitude| absolute, as for the EQ.  PCM cases: within one word
of the twin's quantised value.

Every case prints its worst error over the bound; DESIGN.md §3s records how many cases came out bit-identical."""
import os
import sys

import numpy as np
import pytest

from termdaw_amd import workloads as W

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fx_rig  # noqa: E402
import gate_projects as GP  # noqa: E402
import np_gate as NG  # noqa: E402
from fx_rig import MIX, REL, _pull_all, assert_close, build, render_f32  # noqa: E402

pytestmark = pytest.mark.gpu
GATE_LAUNCHES = ["k_gate_detect", "k_gate_carry_hc", "k_gate_env", "k_gate_carry_env", "k_gate_apply"]
CASE = (-30.0, 6.0, 10.0, 1.0, 100.0, -20.0)   # threshold, hysteresis, hold, attack, release, range


def twin(api, sr, case, x, state=None):
    """(p float32, t, env, end state) of the serial twin on the engine's constants."""
    c = api.gate_params(sr, *case)
    t, env, end = NG.serial(NG.classes(x, c[0], c[1]), c, NG.closed(c[2]) if state is None else state)
    return NG.gain_stage(x, env, c[5], processed=True), t, env, end


def close(y, x, p, what):
    return assert_close(y, x, p, what, GP.E)


GATE = fx_rig.FxKind("gate", "k_gate", GATE_LAUNCHES, GP.add_gate, GP.base_project, CASE, (-20.0, 0.0, 0.0, 0.0, 30.0, -120.0), GP.E,
                     twin=lambda api, sr, case, x: (twin(api, sr, case, x)[0], x),
                     mix=lambda api, sr, case, x, **kw: NG.process(x, api.gate_params(sr, *case), **kw)[0])


# ---- the grid ----
@pytest.mark.parametrize("sr", GP.RATES)
@pytest.mark.parametrize("kind", GP.INPUTS)
def test_grid_matches_the_twin(gpu_api, sr, kind):
    cases = GP.grid_cases()
    assert len(cases) == 108
    p = GP.base_project(kind, sr=sr)
    for i, c in enumerate(cases):
        GP.add_gate(p, "g%d" % i, "bus", c)
    built = build(gpu_api, p)
    x = render_f32(gpu_api, built, "bus", p.cs)
    n = p.cs * p.bl
    assert np.abs(x).max() > 0.05 and n > 5 * 2048
    marks = np.arange(2048, n, 2048)
    worst, exact, acts = 0.0, 0, 0
    seen = {"hysteresis": 0, "hold": 0, "release": 0}
    serials = {}
    for i, c in enumerate(cases):
        k = gpu_api.gate_params(sr, *c)
        if k[:5] not in serials:   # (range_db enters neither t nor env)
            cl = NG.classes(x, k[0], k[1])
            serials[k[:5]] = (cl,) + NG.serial(cl, k, NG.closed(k[2])) + (NG.target(cl, k[2], NG.closed(k[2]))[0],)
        cl, t, env, end, h = serials[k[:5]]
        # the case is not vacuous: on `gated` the gate opens and closes (hold_ms 60 may bridge the short gaps)
        ups = int(np.sum(np.diff(np.concatenate([[0], t]).astype(np.int8)) == 1))
        downs = int(np.sum(np.diff(t.astype(np.int8)) == -1))
        if kind == "gated" and c[2] <= 10.0:
            assert ups >= 3 and downs >= 3, (c, ups, downs)
        # ... and tile boundaries fall inside the stretches no single tile can decide on its own
        seen["hysteresis"] += int(np.any((cl[marks] == 0) & (h[marks] == 1)))      # held open by the band between the thresholds
        seen["hold"] += int(np.any((h[marks] == 0) & (t[marks] == 1)))             # closed, the hold still counting
        seen["release"] += int(np.any((t[marks] == 0) & (env[marks] > 1e-3)))      # the target shut, the fade still on its way down
        pw = NG.gain_stage(x, env, k[5], processed=True)
        y = render_f32(gpu_api, built, "g%d" % i, p.cs)
        worst = max(worst, close(y, x, pw, "%s %d %s" % (kind, sr, c)))
        want = x + np.float32(1.0) * (pw - x)
        exact += int(np.array_equal(y.view(np.uint32), want.view(np.uint32)))
        acts += int(np.abs(want.astype(np.float64) - x).max() > 64.0 * (REL + GP.E) * np.abs(x).max())
    print("grid %s %d: %d cases, worst |y - want| %.3g x the plain bound, %d bit-identical to the twin; tile boundaries inside a "
          "hysteresis stretch / a hold / a release tail in %d / %d / %d cases" % (kind, sr, len(cases), worst, exact, seen["hysteresis"], seen["hold"], seen["release"]))
    # (every case really gates `gated`; drums and noise sit above the threshold most of the time, and a gate that opens in one
    # frame and never closes hands its input on)
    assert acts == len(cases) if kind == "gated" else acts >= len(cases) // 2, acts
    if kind == "gated":
        assert seen["hysteresis"] >= 1 and seen["hold"] >= 1 and seen["release"] >= 1, seen
    assert np.array_equal(render_f32(gpu_api, built, "bus", p.cs), x)   # (and every render above saw this input)


# ---- chunks, pulls, restarts ----
@pytest.mark.parametrize("bl", [1024, 64])
def test_chunked_and_pulled_renders_match_the_twin(gpu_api, bl):
    """0.5 s of `gated`: whole, in 4 096-frame chunks, and by block pulls of `bl` frames -- each inside the bound, and each
    restarted render bitwise the first."""
    p = GP.base_project("gated", bl=bl)
    GP.add_gate(p, "g", "bus", CASE)
    built = build(gpu_api, p)
    n = p.cs * bl
    x = render_f32(gpu_api, built, "bus", p.cs)
    pw, t, env, end = twin(gpu_api, 48000, CASE, x)
    forms = {}
    forms["whole"] = [render_f32(gpu_api, built, "g", p.cs) for _ in range(2)]
    forms["chunks"] = [render_f32(gpu_api, built, "g", p.cs, max_chunk_frames=4096) for _ in range(2)]
    assert n / 4096 > 5
    built[2].set_option("max_chunk_frames", 1 << 24)
    forms["pulls"] = [_pull_all(gpu_api, built, "g", p.cs) for _ in range(2)]
    for name, (a, b) in forms.items():
        assert a.shape == pw.shape
        close(a, x, pw, "%s bl %d" % (name, bl))
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), name
    # the state really crosses the cuts: chunk 1 starts open, restarted from closed it would be far outside the bound
    restart = twin(gpu_api, 48000, CASE, x[4096:8192])[0]
    assert np.abs(restart.astype(np.float64) - pw[4096:8192]).max() > 1e-3
    # a set_time in the middle of pulling restarts the gate from closed: two pulls, a jump into the band segment (which keeps
    # whatever state it is entered with: closed), one pull
    at = (4000 // bl) * bl
    got = []
    for out in ("g", "bus"):
        sb, fb, g = p.build(gpu_api)
        assert g.set_output(out)
        for _ in range(2):
            g.render(sb, fb)
            fb.set_time_to_next_block()
        fb.set_time(at)
        g.set_time(at)
        got.append(np.stack(g.render(sb, fb), axis=1))
    assert np.abs(got[1]).max() > 0.01
    after, t2, _, _ = twin(gpu_api, 48000, CASE, got[1])
    assert not t2.any() and t[at:at + bl].all()   # (closed after the jump, where the running render is open)
    close(got[0], got[1], after, "pull after set_time")


def test_more_than_256_tiles(gpu_api):
    """12 s at 48 kHz of the looped `gated` input: 576 000 frames, 282 tiles -- the carries' lanes fold two tiles each."""
    p = GP.base_project("gated", seconds=12.0)
    GP.add_gate(p, "g", "bus", CASE)
    built = build(gpu_api, p)
    n = p.cs * p.bl
    assert n == 576512 and (n + 2047) // 2048 == 282
    x = render_f32(gpu_api, built, "bus", p.cs)
    pw, t, env, end = twin(gpu_api, 48000, CASE, x)
    assert int(np.sum(np.diff(t.astype(np.int8)) == 1)) > 90
    y = render_f32(gpu_api, built, "g", p.cs)
    close(y, x, pw, "282 tiles")


# ---- the mix ----
@pytest.mark.parametrize("wet,gain,angle", MIX)
def test_wet_pan_and_gain(gpu_api, wet, gain, angle):
    fx_rig.wet_pan_and_gain(gpu_api, GATE, wet, gain, angle, vertex="g")


def test_dry_and_range_zero_pass_the_input_through(gpu_api):
    fx_rig.dry_passes_the_input_through(gpu_api, GATE, live=("unit", CASE[:5] + (0.0,)))


# ---- placement ----
def test_in_front_of_a_normalize_output(gpu_api):
    fx_rig.in_front_of_a_normalize_output(gpu_api, GATE, vertex="g")


def test_as_a_stem_and_two_in_series(gpu_api):
    fx_rig.as_a_stem_and_two_in_series(gpu_api, GATE, "g1", "g2")


def test_fed_by_an_inlined_loop_source_and_a_gain_stage(gpu_api):
    case = (-30.0, 6.0, 5.0, 1.0, 50.0, -40.0)

    def opens_and_closes(x):
        assert 0.1 < twin(gpu_api, 48000, case, x)[1].mean() < 0.9
    fx_rig.fed_by_an_inlined_loop_source_and_a_gain_stage(gpu_api, GATE, case, GP.gated_int16(3), vertex="g", check=opens_and_closes)


def test_batch_members_are_bitwise_their_own_renders(gpu_api):
    fx_rig.batch_members_are_bitwise_their_own_renders(gpu_api, GATE, GP.INPUTS, GP.grid_cases(), vertex="g")


def test_projects_without_a_gate_launch_no_gate_kernel(gpu_api):
    fx_rig.projects_without_the_kind_launch_no_kernel_of_it(gpu_api, "k_gate")
    fx_rig.a_whole_render_launches_the_kinds_kernels(gpu_api, GATE, vertex="g")


# ---- the guard modes ----
def _guard_project(gate_first):
    return fx_rig.gpu_guard_project("add_gate", "g", (-30.0, 6.0, 10.0, 1.0, 100.0, -20.0), gate_first)


def test_guard_keeps_the_scan_and_fast_sines_downstream_of_a_gate(gpu_api):
    fx_rig.guard_keeps_the_scan_and_fast_sines_downstream(gpu_api, _guard_project(True), "gate", "k_gate", GATE_LAUNCHES)


def test_guard_renders_the_exact_forms_upstream_of_a_gate(gpu_api):
    fx_rig.guard_renders_the_exact_forms_upstream(gpu_api, _guard_project(False))


# ---- the front end ----
def test_front_end_renders_a_gated_drum_bus(gpu_api, tmp_path):
    # the drum bus `drums` feeds the band-pass in front of the output: put the gate in between
    p = fx_rig.into_the_drum_bus("add_gate", ("gate", 1.0, 0.0, 1.0, -24.0, 6.0, 20.0, 1.0, 120.0, -40.0))
    mem = fx_rig.front_end_renders(gpu_api, tmp_path, p, 'add_gate("gate",')
    fx_rig.front_end_words_differ(gpu_api, tmp_path, W.drum_project(seconds=1.0), mem)
