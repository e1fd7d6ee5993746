"""The multiband vertex on the device (td_graph_add_multiband) against its float64 twin (tests/np_multiband.py, the
serial restatement of the definition in include/termdaw_amd.h), run on the engine's own constants (td_multiband_params).

The input of the vertex under test always comes from the engine itself: renders of the same graph with set_output on the vertex in
front, read as f32 -- the oracle-verified part of the graph is not restated here.

Bounds.  wet = 1, gain = 1, angle = 0, per value:  |p' - p| <= 2^-23 |p| + E max|p| on the bands' sum p, carried through the
definition's f32 lerp to the vertex' output (fx_rig.assert_close says why it is not asserted on the output as it stands).
The first term is the one f32 rounding of p, which may flip; E covers the float64 re-association of the scans and the device's
log10 / exp10: 8 x what the numpy emulation of the crossover's tiled scans shows over this file's own grid and inputs
(tests/multiband_projects.py E, derived and re-checked on the CPU by tests/test_multiband_host.py; under the cap 2^-28).  With wet
in (0, 1), pan and gain: 4 x 2^-23 x max(|dry|, |p|) x |amplitude| absolute, as for the EQ.

Chunked renders and block pulls go against the twin and the bound: a chunk boundary moves the tile boundaries, so they are not
bitwise the whole render.  24 576 frames are 12 tiles, 4 096-frame chunks two tiles each, pulls of 1 024 and 64 the one-launch
form; 9 blocks of 2 817 frames (25 353 = 24 576 + 777) end in a partial tile, whole and in every chunk."""
import os
import sys

import numpy as np
import pytest

from termdaw_amd import workloads as W

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fx_rig  # noqa: E402
import eq_projects as EP  # noqa: E402
import multiband_projects as MP  # noqa: E402
import np_multiband as NM  # noqa: E402
from fx_rig import assert_close, build, MIX, mix_bound, _pull_all, REL, render_f32  # noqa: E402

pytestmark = pytest.mark.gpu
MB_LAUNCHES = ["k_mb_local", "k_mb_carry", "k_mb_detect", "k_mb_carry_y1", "k_mb_env", "k_mb_carry_yl", "k_mb_apply"]
CASE = MP.case(200.0, 2000.0, MP.BAND_SETTINGS[0], 6.0, (5.0, 50.0))
CASE_LOW = MP.case(40.0, 80.0, MP.BAND_SETTINGS[1], 0.0, (0.0, 1.0))          # the poles nearest z = 1, a hard low band, no attack
CASE_WIDE = MP.case(1000.0, 21600.0, MP.BAND_SETTINGS[2], 40.0, (1000.0, 10000.0))


def _bits(a):
    return a.view(np.uint32)


def twin(api, sr, case, x, state=None):
    """(p float32, end state) of the serial twin on the engine's constants."""
    v, end = NM.serial(x, MP.spec(api, sr, case), state)
    return v.astype(np.float32), end


def close(y, x, p, what):
    return assert_close(y, x, p, what, MP.E)


MULTIBAND = fx_rig.FxKind("multiband", "k_mb", MB_LAUNCHES, MP.add_multiband, EP.base_project, CASE, CASE_LOW, MP.E,
                          twin=lambda api, sr, case, x: (twin(api, sr, case, x)[0], x),
                          mix=lambda api, sr, case, x, **kw: NM.process(x, MP.spec(api, sr, case), **kw)[0])


# ---- the grid ----
@pytest.mark.parametrize("sr", MP.RATES)
@pytest.mark.parametrize("kind", MP.INPUTS)
def test_grid_matches_the_twin(gpu_api, sr, kind):
    cases = MP.grid_cases(sr)
    assert len(cases) == 81
    p = EP.base_project(kind, sr=sr)
    for i, c in enumerate(cases):
        MP.add_multiband(p, "v%d" % i, "bus", c)
    built = build(gpu_api, p)
    x = render_f32(gpu_api, built, "bus", p.cs)
    assert np.abs(x).max() > 0.05 and p.cs * p.bl > 5 * NM.TILE
    vs, _ = NM.serial(x, [MP.spec(gpu_api, sr, c) for c in cases])   # (the cases side by side: three crossovers, 81 detectors)
    worst, exact, acts = 0.0, 0, 0
    for i, v in enumerate(vs):
        pw = v.astype(np.float32)
        y = render_f32(gpu_api, built, "v%d" % i, p.cs)
        worst = max(worst, close(y, x, pw, "%s %d %s" % (kind, sr, cases[i])))
        want = x + np.float32(1.0) * (pw - x)
        exact += int(np.array_equal(_bits(y), _bits(want)))
        acts += int(np.abs(want.astype(np.float64) - x).max() > 64.0 * (REL + MP.E) * np.abs(x).max())
    print("grid %s %d: %d cases, worst |y - want| %.3g x the plain bound, %d bit-identical to the twin" % (kind, sr, len(cases), worst, exact))
    assert acts == len(cases), acts   # (even with no band working the vertex is an all-pass, not the identity)
    assert np.array_equal(render_f32(gpu_api, built, "bus", p.cs), x)


# ---- chunks, pulls, restarts ----
@pytest.mark.parametrize("bl", [1024, 64, 2817])
def test_chunked_and_pulled_renders_match_the_twin(gpu_api, bl):
    """0.5 s: whole, in 4 096-frame chunks (bl 2 817: one block each, a partial second tile every time), and by block pulls of
    `bl` frames -- each inside the bound, and each restarted render bitwise the first."""
    p = EP.base_project("noise", bl=bl)
    MP.add_multiband(p, "v", "bus", CASE_LOW)
    built = build(gpu_api, p)
    n = p.cs * bl
    assert n == {1024: 24576, 64: 24000, 2817: 25353}[bl]   # (12 tiles; 11 tiles and 1 472 frames; 12 tiles and 777 frames)
    x = render_f32(gpu_api, built, "bus", p.cs)
    pw, end = twin(gpu_api, 48000, CASE_LOW, x)
    forms = {}
    forms["whole"] = [render_f32(gpu_api, built, "v", p.cs) for _ in range(2)]
    forms["chunks"] = [render_f32(gpu_api, built, "v", p.cs, max_chunk_frames=4096) for _ in range(2)]
    built[2].set_option("max_chunk_frames", 1 << 24)
    forms["pulls"] = [_pull_all(gpu_api, built, "v", p.cs) for _ in range(2)]
    for name, (a, b) in forms.items():
        assert a.shape == pw.shape
        close(a, x, pw, "%s bl %d" % (name, bl))
        assert np.array_equal(_bits(a), _bits(b)), name
    # the state really crosses the cuts: chunk 1 restarted from zero is far outside the bound
    restart = twin(gpu_api, 48000, CASE_LOW, x[4096:8192])[0]
    assert np.abs(restart.astype(np.float64) - pw[4096:8192]).max() > 1e-4 * np.abs(pw).max()
    # a set_time in the middle of pulling restarts the state: two pulls, a jump, one pull -- the twin started from zero there
    at = (4000 // bl) * bl
    got = []
    for out in ("v", "bus"):
        sb, fb, g = p.build(gpu_api)
        assert g.set_output(out)
        for _ in range(2):
            g.render(sb, fb)
            fb.set_time_to_next_block()
        fb.set_time(at)
        g.set_time(at)
        got.append(np.stack(g.render(sb, fb), axis=1))
    assert np.abs(got[1]).max() > 0.01
    close(got[0], got[1], twin(gpu_api, 48000, CASE_LOW, got[1])[0], "pull after set_time")


def test_more_than_256_tiles(gpu_api):
    """12 s at 48 kHz of the looped noise: 576 512 frames, 282 tiles -- every carry folds two tiles per lane."""
    p = EP.base_project("noise", seconds=12.0)
    MP.add_multiband(p, "v", "bus", CASE)
    built = build(gpu_api, p)
    n = p.cs * p.bl
    assert n == 576512 and (n + NM.TILE - 1) // NM.TILE == 282
    x = render_f32(gpu_api, built, "bus", p.cs)
    close(render_f32(gpu_api, built, "v", p.cs), x, twin(gpu_api, 48000, CASE, x)[0], "282 tiles")


# ---- the mix ----
@pytest.mark.parametrize("wet,gain,angle", MIX + [(1.0, 1.7, -75.0)])
def test_wet_pan_and_gain(gpu_api, wet, gain, angle):
    fx_rig.wet_pan_and_gain(gpu_api, MULTIBAND, wet, gain, angle)


def test_dry_is_a_sum_launch_and_leaves_the_line_alone(gpu_api):
    p = EP.base_project("drums")
    MP.add_multiband(p, "dry", "bus", CASE, wet=0.0)
    MP.add_multiband(p, "almost", "bus", CASE, wet=0.00009)
    MP.add_multiband(p, "wet", "bus", CASE)
    built = build(gpu_api, p)
    x = render_f32(gpu_api, built, "bus", p.cs)
    for name in ("dry", "almost"):
        y = render_f32(gpu_api, built, name, p.cs)
        assert np.array_equal(y, x), (name, np.argwhere(y != x)[:4].tolist())
    g = built[2]
    g.set_profiling(1)
    render_f32(gpu_api, built, "dry", p.cs)
    names = list(g.kernel_times())
    assert not any(n.startswith("k_mb") for n in names) and "k_sum" in names, names   # wet < 0.0001: a plain sum launch
    render_f32(gpu_api, built, "wet", p.cs)
    assert [n for n in g.kernel_times() if n.startswith("k_mb")] == MB_LAUNCHES
    # a chunk of one tile is k_mb_apply alone
    q = EP.base_project("drums", seconds=0.04)
    MP.add_multiband(q, "v", "bus", CASE)
    assert q.cs * q.bl == NM.TILE
    sb, fb, g = q.build(gpu_api)
    g.set_output("v")
    g.set_profiling(1)
    g.render_all(sb, fb, q.cs, 16, want_f32=False)
    assert [n for n in g.kernel_times() if n.startswith("k_mb")] == ["k_mb_apply"]
    # the line stays as it is while the vertex is dry: pulls of a wet vertex, with a dry one of the same graph rendered in between,
    # are the pulls without it
    r = EP.base_project("noise")
    MP.add_multiband(r, "v", "bus", CASE)
    MP.add_multiband(r, "d", "v", CASE_LOW, wet=0.0)
    a = _pull_all(gpu_api, r.build(gpu_api), "v", 6)
    sb, fb, g = r.build(gpu_api)
    blocks = []
    for i in range(6):
        assert g.set_output("d" if i % 2 else "v")
        blocks.append(np.stack(g.render(sb, fb), axis=1))
        fb.set_time_to_next_block()
    assert np.array_equal(_bits(np.concatenate(blocks)), _bits(a))


def test_projects_without_a_multiband_launch_no_multiband_kernel(gpu_api):
    fx_rig.projects_without_the_kind_launch_no_kernel_of_it(gpu_api, "k_mb")


# ---- non-vacuity ----
def test_only_the_high_band_works_on_a_two_tone_input(gpu_api):
    """0.25 sin 100 Hz + 0.25 sin 8 kHz at 48 kHz through a 400 / 3 000 Hz crossover, low and mid at ratio 1, high at (-30 dB, 4:1,
    attack 5, release 50, knee 6): over the last 8 192 frames of 24 576 the 8 kHz line of the render's spectrum falls by at least
    6 dB, the 100 Hz line moves by less than 0.1 dB, and both are within 0.01 dB of the twin's."""
    sr = 48000
    p = W.ProjectScript(sr, 1024)
    p.set_length(0.5)
    p.set_render_samplerate(sr)
    t = np.arange(sr) / sr   # (whole cycles of both tones in a second: the asset loops cleanly)
    tone = np.round(32767.0 * (0.25 * np.sin(2.0 * np.pi * 100.0 * t) + 0.25 * np.sin(2.0 * np.pi * 8000.0 * t))).astype(np.int16)
    p.assets["t"] = W.Asset(np.stack([tone, tone], axis=1), sr=sr)
    p.load_sample("t", "t", "")
    p.add_sampleloop("t", 0.5 * float(np.abs(tone).max()) / 32767.0, 0.0, "t")   # (a loaded sample is scaled to a peak of 1: back to 0.25 per tone, over two edges)
    p.add_sum("bus", 1.0, 0.0); p.connect("t", "bus"); p.connect("t", "bus")
    MP.add_multiband(p, "v", "bus", MP.TONE_CASE)
    p.set_output("v")
    built = build(gpu_api, p)
    x = render_f32(gpu_api, built, "bus", p.cs)
    y = render_f32(gpu_api, built, "v", p.cs)
    assert len(y) == 24576
    lo_in, hi_in = MP.tone_lines(x)
    lo_out, hi_out = MP.tone_lines(y)
    lo_twin, hi_twin = MP.tone_lines(twin(gpu_api, sr, MP.TONE_CASE, x)[0])
    print("100 Hz line in at %.2f dB, moves %.3g dB; 8 kHz line moves %.3f dB (twin: %.3g, %.3f)" % (lo_in, lo_out - lo_in, hi_out - hi_in, lo_twin - lo_in, hi_twin - hi_in))
    assert abs(lo_in - 20.0 * np.log10(0.25)) < 0.05 and abs(hi_in - lo_in) < 0.05
    assert hi_out - hi_in <= -6.0 and abs(lo_out - lo_in) < 0.1
    assert abs(lo_out - lo_twin) < 0.01 and abs(hi_out - hi_twin) < 0.01


# ---- the guard modes ----
def _guard_project(where):
    return fx_rig.gpu_guard_project("add_multiband", "v", CASE, where == "downstream")


def test_guard_keeps_the_scan_and_fast_sines_downstream_of_a_multiband(gpu_api):
    fx_rig.guard_keeps_the_scan_and_fast_sines_downstream(gpu_api, _guard_project("downstream"), "multiband", "k_mb", MB_LAUNCHES)


def test_guard_renders_the_exact_forms_upstream_of_a_multiband(gpu_api):
    fx_rig.guard_renders_the_exact_forms_upstream(gpu_api, _guard_project("input"), floor=1e-3)


# ---- batches ----
def test_batch_members_are_bitwise_their_own_renders(gpu_api):
    """Eight projects, each with two multibands of different settings in ONE level: the merged launches give every member the
    words of its own render."""
    projects = []
    cases = MP.grid_cases(48000)
    for i in range(8):
        p = EP.base_project(MP.INPUTS[i % 3], seconds=1.0)
        MP.add_multiband(p, "va", "bus", cases[(13 * i + 5) % len(cases)], wet=[1.0, 0.6][i % 2], gain=[1.0, 0.7][(i // 4) % 2])
        MP.add_multiband(p, "vb", "bus", cases[(29 * i + 1) % len(cases)])
        p.add_sum("mix", 0.5, 0.0); p.connect("va", "mix"); p.connect("vb", "mix")
        if i % 4 == 2:   # in front of a Normalize output
            p.add_normalize("out", 1.0, 0.0)
            p.connect("mix", "out")
            p.set_output("out")
        else:
            p.set_output("mix")
        projects.append(p)
    fx_rig.batch_matches_own_renders(gpu_api, projects)


# ---- the front end ----
def test_front_end_renders_the_multiband_project(gpu_api, tmp_path):
    mem = fx_rig.front_end_renders(gpu_api, tmp_path, W.multiband_project(seconds=1.0), 'add_multiband("mb",')
    # ... and the vertex is really in the path: dry, the same project is the plain bus
    fx_rig.front_end_words_differ(gpu_api, tmp_path, W.multiband_project(seconds=1.0, wet=0.0), mem)


# ---- random projects ----
def _fresh(api, p, out, form="whole"):
    """`out` rendered by a freshly built project: the event-driven sources of a random project keep the voices that are still
    sounding when a render ends, so only renders that start from a new build start from the same state."""
    built = p.build(api)
    if form == "chunks":
        built[2].set_option("max_chunk_frames", 4096)
    if form == "pulls":
        return _pull_all(api, built, out, p.cs)
    return render_f32(api, built, out, p.cs)


@pytest.mark.parametrize("seed", range(8))
def test_random_multiband_projects(gpu_api, seed):
    p = MP.random_multiband_project(seed)
    p.sine_mode = 1   # (the reference's sine: every render of a vertex gives the same bits whatever the output is)
    out = p.output_vertex
    whole = _fresh(gpu_api, p, out)
    assert np.array_equal(_bits(whole), _bits(_fresh(gpu_api, p, out))), seed
    # the first multiband that is not dry against the twin on the engine's own x, whole, in chunks and by pulls
    wets = [c for c in p.calls["add_multiband"] if c[3] >= 0.0001]
    if not wets:
        return
    args = wets[0]
    v, gain, angle, wet, case = args[0], args[1], args[2], args[3], tuple(args[4:])
    ins = [a for a, b in p.calls["connect"] if b == v]
    x = np.zeros((p.cs * p.bl, 2), np.float32)
    for nm in ins:
        x = x + _fresh(gpu_api, p, nm)
    sp = MP.spec(gpu_api, 48000, case)
    want, _ = NM.process(x, sp, wet=wet, gain=gain, angle=angle)
    proc = NM.serial(x, sp)[0].astype(np.float32)
    with np.errstate(invalid="ignore"):
        lim = mix_bound(x, proc, gain, angle)
    for form in ("whole", "chunks", "pulls"):
        y = _fresh(gpu_api, p, v, form)
        err = np.abs(y.astype(np.float64) - want.astype(np.float64))
        print("seed %d: %s, %s: worst error / bound %.3g" % (seed, v, form, float(np.nanmax(err / lim))))
        assert (err <= lim).all(), (seed, v, form, float(np.nanmax(err / lim)), np.argwhere(~(err <= lim))[:4].tolist())
