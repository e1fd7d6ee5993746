"""The phaser vertex on the device (td_graph_add_phaser) against its float64 twin (tests/np_phaser.py, the serial
restatement of the definition in include/termdaw_amd.h), run on the engine's own constants (td_phaser_params).

The input of the vertex under test always comes from the engine itself: a second render of the same graph with set_output on
the vertex in front, read as f32 -- the oracle-verified part of the graph is not restated here.

Bounds.  wet = 1, gain = 1, angle = 0, per value:  |p' - p| <= 2^-23 |p| + E max|p| on the chain's output p, carried through the
definition's f32 lerp to the vertex' output (test_gpu_eq.assert_close says why it is not asserted on the output as it stands).
The first term is the one f32 rounding of the chain, which may flip; E covers the float64 re-association of the scan: 8 x what
the numpy emulation of the tiled scan shows over this file's own grid and inputs (tests/phaser_projects.py E, derived and
re-checked on the CPU by tests/test_phaser_host.py; far under the cap 2^-28).  a[n] is the same bits on both sides: IEEE add,
multiply, floor and fabs on the same constants.
With wet in (0, 1), pan and gain: 4 x 2^-23 x max(|dry|, |p|) x |amplitude| absolute, as for the EQ.  PCM cases: within one word
of the twin's quantised value.

Every case prints its worst error over the bound; DESIGN.md §3u records how many cases came out bit-identical."""
import os
import subprocess
import sys
import wave

import numpy as np
import pytest

from termdaw_amd import workloads as W

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import np_phaser as NP  # noqa: E402
import phaser_projects as PP  # noqa: E402
from test_gpu_compressor import MIX, _quantise16  # noqa: E402
from test_gpu_eq import REL, F32_TINY, _pull_all, assert_close, build, mix_bound, render_f32  # noqa: E402
from test_gpu_stems import _write_project  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PHASER_LAUNCHES = ["k_phaser_local", "k_phaser_carry", "k_phaser_apply"]
CASE = (4, 200.0, 2000.0, 1.0, 0.7, 0.25, "sine")   # stages, lo, hi, rate, feedback, stereo, shape
CASE8 = (8, 300.0, 6000.0, 0.5, -0.9, 0.5, "triangle")


def twin(api, sr, case, x, state=None, t0=0):
    """(p float32, end state) of the serial twin on the engine's constants."""
    v, end = NP.serial(x, PP.spec(api, sr, case), state, t0)
    return v.astype(np.float32), end


def close(y, x, p, what):
    return assert_close(y, x, p, what, PP.E)


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
    p = PP.base_project("drums")
    PP.add_phaser(p, "ph", "bus", CASE, wet=wet, gain=gain, angle=angle)
    built = build(gpu_api, p)
    x = render_f32(gpu_api, built, "bus", p.cs)
    y = render_f32(gpu_api, built, "ph", p.cs)
    sp = PP.spec(gpu_api, 48000, CASE)
    want, _ = NP.process(x, sp, wet=wet, gain=gain, angle=angle)
    proc, _ = NP.process(x, sp, processed=True)
    lim = mix_bound(x, proc, gain, angle)
    err = np.abs(y.astype(np.float64) - want.astype(np.float64))
    print("wet %g gain %g angle %g: worst error / bound %.3g" % (wet, gain, angle, float(np.max(err / lim))))
    assert (err <= lim).all(), (float(np.max(err / lim)), np.argwhere(err > lim)[:4].tolist())
    assert np.abs(want - x).max() > 1e-3 * wet   # (the vertex does something, in proportion to the mix)


def test_dry_passes_the_input_through_as_a_sum_launch(gpu_api):
    p = PP.base_project("drums")
    PP.add_phaser(p, "dry", "bus", CASE, wet=0.0)
    PP.add_phaser(p, "almost", "bus", CASE, wet=0.00009)
    PP.add_phaser(p, "wet", "bus", CASE)
    built = build(gpu_api, p)
    x = render_f32(gpu_api, built, "bus", p.cs)
    for name in ("dry", "almost"):
        y = render_f32(gpu_api, built, name, p.cs)
        assert np.array_equal(y, x), (name, np.argwhere(y != x)[:4].tolist())
    g = built[2]
    g.set_profiling(1)
    render_f32(gpu_api, built, "dry", p.cs)
    names = list(g.kernel_times())
    assert not any(n.startswith("k_phaser") for n in names) and "k_sum" in names, names   # wet < 0.0001: a plain sum launch
    render_f32(gpu_api, built, "wet", p.cs)
    assert [n for n in g.kernel_times() if n.startswith("k_phaser")] == PHASER_LAUNCHES


# ---- placement ----
def test_in_front_of_a_normalize_output(gpu_api):
    p = PP.base_project("drums", seconds=1.0)
    PP.add_phaser(p, "ph", "bus", CASE)
    p.add_normalize("out", 1.0, 0.0)
    p.connect("ph", "out")
    built = build(gpu_api, p)
    x = render_f32(gpu_api, built, "bus", p.cs)
    c = render_f32(gpu_api, built, "ph", p.cs)
    close(c, x, twin(gpu_api, 48000, CASE, x)[0], "in front of Normalize")
    # normalize_gen (extensions.rs:321-329) on what the phaser really handed on: the running block peak from 1e-6, f32
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
    p = PP.base_project("drums", seconds=1.0)
    PP.add_phaser(p, "p1", "bus", CASE)
    PP.add_phaser(p, "p2", "p1", CASE8, gain=0.8, angle=-20.0)
    p.add_sum("post", 0.5, 10.0)
    p.connect("p2", "post")
    built = build(gpu_api, p)
    x = render_f32(gpu_api, built, "bus", p.cs)
    y1 = render_f32(gpu_api, built, "p1", p.cs)
    close(y1, x, twin(gpu_api, 48000, CASE, x)[0], "first of two")
    # the second one against the twin on what the first one really handed it
    y2 = render_f32(gpu_api, built, "p2", p.cs)
    s2 = PP.spec(gpu_api, 48000, CASE8)
    w2, _ = NP.process(y1, s2, gain=0.8, angle=-20.0)
    proc, _ = NP.process(y1, s2, processed=True)
    assert (np.abs(y2.astype(np.float64) - w2) <= mix_bound(y1, proc, 0.8, -20.0)).all()
    # both as stems of a render whose output sits downstream
    sb, fb, g = built
    g.set_output("post")
    g.set_stems(["p2", "p1"])
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
    p.add_sampleloop("l0", 0.7, 30.0, "a0")     # read by the phaser itself (term kinds 1 / 3)
    p.add_sampleloop("l1", 0.02, 0.0, "a1")
    p.add_sum("stage", 0.5, -45.0)              # one input: a gain / pan stage, read through (term kind 4)
    p.connect("l1", "stage")
    PP.add_phaser(p, "ph", "l0", CASE)
    p.connect("stage", "ph")
    p.set_output("ph")
    built = p.build(gpu_api)
    a = render_f32(gpu_api, built, "l0", p.cs)
    b = render_f32(gpu_api, built, "stage", p.cs)
    x = (np.float32(0.0) + a) + b               # sum_inputs (extensions.rs:310-319), f32, in connect() order
    pw, _ = twin(gpu_api, 48000, CASE, x)
    for packed in (1, 0):
        y = render_f32(gpu_api, built, "ph", p.cs, packed_samples=packed)
        close(y, x, pw, "inlined terms, packed_samples %d" % packed)


def test_batch_members_are_bitwise_their_own_renders(gpu_api):
    projects = []
    cases = PP.grid_cases(48000)
    for i in range(8):
        p = PP.base_project(PP.INPUTS[i % 3], seconds=1.0, seed=i)
        c = cases[(13 * i + 5) % len(cases)]
        PP.add_phaser(p, "ph", "bus", c, wet=[1.0, 0.6][i % 2], gain=[1.0, 0.7][(i // 4) % 2])
        if i % 4 == 1:     # a second one in series, as the output
            PP.add_phaser(p, "ph2", "ph", cases[(29 * i + 1) % len(cases)])
            p.set_output("ph2")
        elif i % 4 == 2:   # in front of a Normalize output
            p.add_normalize("out", 1.0, 0.0)
            p.connect("ph", "out")
            p.set_output("out")
        else:
            p.set_output("ph")
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


def test_projects_without_a_phaser_launch_no_phaser_kernel(gpu_api):
    for p in (W.drum_project(seconds=1.0), W.config2(seconds=1.0, n_src=8)):
        sb, fb, g = p.build(gpu_api)
        g.set_profiling(1)
        g.render_all(sb, fb, p.cs, 16, want_f32=False)
        names = list(g.kernel_times())
        assert names and not any(n.startswith("k_phaser") for n in names), names
    p = PP.base_project("drums")
    PP.add_phaser(p, "ph", "bus", CASE)
    p.set_output("ph")
    sb, fb, g = p.build(gpu_api)
    g.set_profiling(1)
    g.render_all(sb, fb, p.cs, 16, want_f32=False)
    assert [n for n in g.kernel_times() if n.startswith("k_phaser")] == PHASER_LAUNCHES
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
    p.add_phaser("ph", 1.0, 0.0, 1.0, *CASE)
    if phaser_first:   # loop -> phaser -> band-pass chain; the synth joins behind the phaser
        p.connect("s", "ph"); p.connect("ph", "b1"); p.connect("b1", "b2"); p.connect("b2", "bus"); p.connect("y", "bus")
        p.set_output("bus")
    else:              # band-pass chain and synth -> bus -> phaser
        p.connect("s", "b1"); p.connect("b1", "b2"); p.connect("b2", "bus"); p.connect("y", "bus"); p.connect("bus", "ph")
        p.set_output("ph")
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


def test_guard_keeps_the_scan_and_fast_sines_downstream_of_a_phaser(gpu_api):
    outs, names = _guard_renders(gpu_api, _guard_project(True))
    rms = float(np.sqrt(np.mean((outs["guard"].astype(np.float64) - outs["exact"].astype(np.float64)) ** 2)))
    print("guarded scan + fast sines downstream of a phaser: rms %.3g against the exact forms" % rms)
    assert rms <= 1e-6 and np.abs(outs["exact"]).max() > 0.05
    assert "k_band_scan" in names["guard"] and "k_sine_probe" in names["guard"], names["guard"]
    assert not any(n in names["guard"] for n in ("k_band_pass", "k_band_spec")), names["guard"]
    assert [n for n in names["guard"] if n.startswith("k_phaser")] == PHASER_LAUNCHES


def test_guard_renders_the_exact_forms_upstream_of_a_phaser(gpu_api):
    outs, names = _guard_renders(gpu_api, _guard_project(False))
    assert np.array_equal(outs["guard"].view(np.uint32), outs["exact"].view(np.uint32)) and np.abs(outs["exact"]).max() > 0.05
    assert "k_band_scan" not in names["guard"] and "k_sine_probe" not in names["guard"], names["guard"]
    assert any(n in names["guard"] for n in ("k_band_pass", "k_band_spec")), names["guard"]


# ---- the front end ----
def test_front_end_renders_a_drum_bus_with_a_phaser(gpu_api, tmp_path):
    ph = ("phaser", 1.0, 0.0, 0.5, 4, 200.0, 2000.0, 1.0, 0.7, 0.25, "sine")
    p = W.drum_project(seconds=1.0)
    # the drum bus `drums` feeds the band-pass in front of the output: put the phaser in between
    i = p.calls["connect"].index(("drums", "band"))
    p.calls["connect"][i:i + 1] = [("drums", "phaser"), ("phaser", "band")]
    j = p.script_order.index(("connect", ("drums", "band")))
    p.script_order[j:j + 1] = [("add_phaser", ph), ("connect", ("drums", "phaser")), ("connect", ("phaser", "band"))]
    p.calls["add_phaser"].append(ph)
    d = str(tmp_path / "proj")
    _write_project(p, d)
    out = str(tmp_path / "m.wav")
    r = subprocess.run([sys.executable, "-m", "termdaw_amd", d, "-o", out], env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    st = gpu_api.State(open_dir=d)
    assert st.refresh(), gpu_api.last_error()
    assert 'add_phaser("phaser",' in st.dump_calls()
    mem = st.render_to_memory()
    with wave.open(out, "rb") as w:
        words = np.frombuffer(w.readframes(w.getnframes()), np.int16).reshape(-1, 2)
    assert words.shape == mem.shape and np.array_equal(words, mem) and np.abs(mem).max() > 1000
    # ... and the phaser is really in the path: without it the words differ
    q = W.drum_project(seconds=1.0)
    d2 = str(tmp_path / "plain")
    _write_project(q, d2)
    st2 = gpu_api.State(open_dir=d2)
    assert st2.refresh()
    assert not np.array_equal(st2.render_to_memory(), mem)
