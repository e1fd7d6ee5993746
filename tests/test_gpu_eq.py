"""The parametric EQ vertex on the device (td_graph_add_eq) against its float64 twin (tests/np_eq.py, the serial
restatement of the definition in include/termdaw_amd.h), run on the engine's own coefficients (td_eq_coefficients).

The input of the vertex under test always comes from the engine itself: a second render of the same graph with set_output on
the vertex in front, read as f32 -- the oracle-verified part of the graph is not restated here.

Bounds.  wet = 1, gain = 1, angle = 0, per value:  |p' - p| <= 2^-23 |p| + E max|p| on the filtered signal p, carried through
the definition's f32 lerp to the vertex' output (assert_close says why it is not asserted on the output as it stands).  The
first term is the one f32 rounding of the chain, which may flip; E covers the float64 re-association of the scan where |p| is
near zero: 8 x what the
numpy emulation of the tiled scan shows over this file's own grid and inputs (tests/eq_projects.py E, derived and re-checked on
the CPU by tests/test_eq_host.py; E <= 2^-28).  With wet in (0, 1), pan and gain: 4 x 2^-23 x max(|dry|, |p|) x |amplitude|
absolute -- three more f32 operations of the lerp, two of pan / gain, each half an ulp of an operand no larger than that.  PCM
cases: within one word of the twin's quantised value.

Every case prints its worst error over the bound.  No device figures are recorded yet."""
import os
import sys

import numpy as np
import pytest

from termdaw_amd import workloads as W

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fx_rig  # noqa: E402
import eq_projects as EP  # noqa: E402
import np_eq as NE  # noqa: E402
from fx_rig import MIX, REL, _pull_all, _quantise16, assert_close, build, mix_bound, over_bound, render_f32  # noqa: E402

pytestmark = pytest.mark.gpu


def coeffs(api, sr, kind, f, q, g):
    b, a, _ = api.eq_coefficients(kind, sr, f, q, g)
    return np.concatenate([b, a[1:]])


def twin_p(api_coeffs, x):
    return NE.eq(x, api_coeffs, processed=True)[0]


def _grid(gpu_api, sr, kind, cases, E):
    p = EP.base_project(kind, sr=sr)
    for i, (k, f, q, g) in enumerate(cases):
        EP.add_eq(p, "e%d" % i, "bus", k, f, q, g)
    built = build(gpu_api, p)
    x = render_f32(gpu_api, built, "bus", p.cs)
    assert np.abs(x).max() > 0.05 and p.cs * p.bl > 5 * 2048
    cs = np.array([coeffs(gpu_api, sr, *c) for c in cases])
    ser, _ = NE.biquad(x, cs)
    worst, exact = 0.0, 0
    for i, c in enumerate(cases):
        y = render_f32(gpu_api, built, "e%d" % i, p.cs)
        pw = ser[i].astype(np.float32)
        want = x + np.float32(1.0) * (pw - x)   # the lerp at wet = 1, f32
        w = assert_close(y, x, pw, "%s %d %s" % (kind, sr, c), E)
        worst = max(worst, w)
        exact += int(np.array_equal(y.view(np.uint32), want.view(np.uint32)))
        # the filter acts: also at 0 dB-like corners (a 10 Hz high-pass, a low-pass at 0.45 sr) the output is far from the input
        assert np.abs(want.astype(np.float64) - x).max() > 64.0 * (REL + E) * np.abs(x).max(), c
    print("grid %s %d: %d cases, worst |y - want| %.3g x the plain bound, %d bit-identical to the twin" % (kind, sr, len(cases), worst, exact))
    assert np.array_equal(render_f32(gpu_api, built, "bus", p.cs), x)   # (and every render above saw this input)


@pytest.mark.parametrize("sr", EP.RATES)
@pytest.mark.parametrize("kind", EP.INPUTS)
def test_grid_matches_the_twin(gpu_api, sr, kind):
    _grid(gpu_api, sr, kind, EP.grid_cases(sr), EP.E)


@pytest.mark.parametrize("kind", EP.INPUTS)
def test_below_the_grid_at_96_khz(gpu_api, kind):
    """10 and 20 Hz at 96 kHz, where the float64 recurrence itself is only defined to about 1e-9 of the peak: the same bound
    with the constant these cases' own emulation gives (tests/eq_projects.py E_LOW)."""
    _grid(gpu_api, 96000, kind, EP.low_cases(), EP.E_LOW)


PEAK = ("peak", 900.0, 2.5, 9.0)
EQ_LAUNCHES = ["k_eq_local", "k_eq_carry", "k_eq_apply"]
# (of the shared bodies the EQ takes the mix test alone: its other placement tests have cases and bounds of their own)
EQ = fx_rig.FxKind("EQ", "k_eq", EQ_LAUNCHES, lambda p, name, src, case, **kw: EP.add_eq(p, name, src, *case, **kw), EP.base_project, PEAK, None, EP.E,
                   twin=lambda api, sr, case, x: (twin_p(coeffs(api, sr, *case), x), x),
                   mix=lambda api, sr, case, x, **kw: NE.eq(x, coeffs(api, sr, *case), **kw)[0])


@pytest.mark.parametrize("wet,gain,angle", MIX)
def test_wet_pan_and_gain(gpu_api, wet, gain, angle):
    fx_rig.wet_pan_and_gain(gpu_api, EQ, wet, gain, angle, vertex="e")


def test_dry_passes_the_input_through_as_a_sum_launch(gpu_api):
    p = EP.base_project("drums")
    EP.add_eq(p, "dry", "bus", *PEAK, wet=0.0)
    EP.add_eq(p, "almost", "bus", *PEAK, wet=0.00009)
    built = build(gpu_api, p)
    x = render_f32(gpu_api, built, "bus", p.cs)
    for name in ("dry", "almost"):
        y = render_f32(gpu_api, built, name, p.cs)
        assert np.array_equal(y, x), (name, np.argwhere(y != x)[:4].tolist())
    g = built[2]
    g.set_profiling(1)
    render_f32(gpu_api, built, "dry", p.cs)
    names = list(g.kernel_times())
    assert not any(n.startswith("k_eq") for n in names) and "k_sum" in names, names   # wet < 0.0001: a plain sum launch


CHUNK = ("lowshelf", 120.0, 0.9, 9.0)


@pytest.mark.parametrize("bl", [1024, 64])
def test_chunked_and_pulled_renders_match_the_twin(gpu_api, bl):
    """20 s: whole, in >= 3 chunks, and by block pulls of `bl` frames -- each inside the bound, each bitwise repeatable."""
    p = EP.base_project("drums", bl=bl, seconds=20.0)
    EP.add_eq(p, "e", "bus", *CHUNK)
    built = build(gpu_api, p)
    n = p.cs * bl
    x = render_f32(gpu_api, built, "bus", p.cs)
    c = coeffs(gpu_api, 48000, *CHUNK)
    want, end = NE.eq(x, c)
    pt = twin_p(c, x)
    forms = {}
    forms["whole"] = [render_f32(gpu_api, built, "e", p.cs) for _ in range(2)]
    cap = (n // 3 // bl) * bl - 7 * bl
    assert n / cap > 3
    forms["chunks"] = [render_f32(gpu_api, built, "e", p.cs, max_chunk_frames=cap) for _ in range(2)]
    built[2].set_option("max_chunk_frames", 1 << 24)
    forms["pulls"] = [_pull_all(gpu_api, built, "e", p.cs) for _ in range(2)]
    for name, (a, b) in forms.items():
        assert_close(a, x, pt, "%s bl %d" % (name, bl))
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), name
    # the filter really carries state across the cuts: restarting it at a cut is far outside the bound
    restart, _ = NE.eq(x[cap:2 * cap], c)
    worst, _ = over_bound(restart, want[cap:2 * cap], EP.E)
    assert worst > 1000.0, worst
    assert np.array_equal(render_f32(gpu_api, built, "bus", p.cs), x)
    # a set_time in the middle of pulling restarts the filter from zero: two pulls, a jump, one pull (two fresh builds: one for
    # the vertex, one for its input)
    half = (p.cs // 2) * bl
    got = []
    for out in ("e", "bus"):
        sb, fb, g = p.build(gpu_api)
        assert g.set_output(out)
        for _ in range(2):
            g.render(sb, fb)
            fb.set_time_to_next_block()
        fb.set_time(half)
        g.set_time(half)
        got.append(np.stack(g.render(sb, fb), axis=1))
    assert np.abs(got[1]).max() > 0.01
    assert_close(got[0], got[1], twin_p(c, got[1]), "pull after set_time")


def test_batch_members_are_bitwise_their_own_renders(gpu_api):
    projects = []
    for i in range(8):
        kind = ["drums", "noise", "burst"][i % 3]
        p = EP.base_project(kind, seconds=1.0, seed=i)
        case = (NE.KINDS[i % 7], [10.0, 150.0, 2500.0, 21600.0][i % 4], [0.1, 0.707, 20.0][i % 3], [-24.0, 6.0, 24.0][(i // 2) % 3])
        EP.add_eq(p, "e", "bus", *case, wet=[1.0, 0.6][i % 2], gain=[1.0, 0.7][(i // 4) % 2])
        if i % 4 == 1:     # a second one in series, as the output
            EP.add_eq(p, "e2", "e", "highshelf", 6000.0, 0.707, -8.0)
            p.set_output("e2")
        elif i % 4 == 2:   # in front of a Normalize output
            p.add_normalize("out", 1.0, 0.0)
            p.connect("e", "out")
            p.set_output("out")
        else:
            p.set_output("e")
        projects.append(p)
    cs = projects[0].cs
    own = []   # per project: its first and its second render (the second starts with the voices the first left sounding)
    for p in projects:
        sb, fb, g = p.build(gpu_api)
        first = g.render_all(sb, fb, cs, 16, want_f32=False)[0]
        g.reset_normalize_vertices()
        fb.set_time(0)
        own.append((first, g.render_all(sb, fb, cs, 16, want_f32=False)[0]))
    assert len({o[0].tobytes() for o in own}) == 8
    batch = gpu_api.Batch()
    for p in projects:
        batch.add(*p.build(gpu_api))
    for rep in range(2):   # (two rewinds: the second render enters with a fresh state again)
        batch.rewind()
        assert batch.render_all(cs, 16) == cs * 1024
        for i in range(8):
            assert np.array_equal(batch.read_pcm(i, cs), own[i][rep]), (rep, i)


def test_in_front_of_a_normalize_output(gpu_api):
    case = ("peak", 200.0, 4.0, 12.0)
    p = EP.base_project("drums", seconds=1.0)
    EP.add_eq(p, "e", "bus", *case)
    p.add_normalize("out", 1.0, 0.0)
    p.connect("e", "out")
    built = build(gpu_api, p)
    x = render_f32(gpu_api, built, "bus", p.cs)
    c, _ = NE.eq(x, coeffs(gpu_api, 48000, *case))
    # normalize_gen (extensions.rs:321-329): the running block peak from 1e-6 (state.rs:467), f32
    pk = np.abs(c).reshape(-1, p.bl * 2).max(axis=1)
    run = np.maximum.accumulate(np.concatenate([[np.float32(0.000001)], pk]).astype(np.float32))[1:]
    want = c * np.repeat(np.float32(1.0) / run, p.bl)[:, None]
    sb, fb, g = built
    g.set_output("out")
    fb.set_time(0)
    g.set_time(0)
    g.reset_normalize_vertices()
    pcm, f = g.render_all(sb, fb, p.cs, 16)
    assert np.abs(pcm.astype(np.int64) - _quantise16(want)).max() <= 1
    assert np.abs(f.astype(np.float64) - want).max() <= 4.0 * REL * np.abs(want).max()


def test_as_a_stem_and_two_in_series(gpu_api):
    c1, c2 = ("lowshelf", 150.0, 0.707, 9.0), ("notch", 3000.0, 8.0, 0.0)
    p = EP.base_project("drums", seconds=1.0)
    EP.add_eq(p, "e1", "bus", *c1)
    EP.add_eq(p, "e2", "e1", *c2, gain=0.8, angle=-20.0)
    p.add_sum("post", 0.5, 10.0)
    p.connect("e2", "post")
    built = build(gpu_api, p)
    x = render_f32(gpu_api, built, "bus", p.cs)
    y1 = render_f32(gpu_api, built, "e1", p.cs)
    assert_close(y1, x, twin_p(coeffs(gpu_api, 48000, *c1), x), "first of two")
    # the second one against the twin on what the first one really handed it
    y2 = render_f32(gpu_api, built, "e2", p.cs)
    k2 = coeffs(gpu_api, 48000, *c2)
    w2, _ = NE.eq(y1, k2, gain=0.8, angle=-20.0)
    proc, _ = NE.eq(y1, k2, processed=True)
    assert (np.abs(y2.astype(np.float64) - w2) <= mix_bound(y1, proc, 0.8, -20.0)).all()
    # both as stems of a render whose output sits downstream
    sb, fb, g = built
    g.set_output("post")
    g.set_stems(["e2", "e1"])
    fb.set_time(0)
    g.set_time(0)
    g.render_all(sb, fb, p.cs, 16)
    assert np.abs(g.read_stem_pcm(0).astype(np.int64) - _quantise16(w2)).max() <= 1
    assert np.abs(g.read_stem_pcm(1).astype(np.int64) - _quantise16(y1)).max() == 0
    g.set_stems([])


def test_fed_by_an_inlined_loop_source_and_a_gain_stage(gpu_api):
    case = ("highpass", 300.0, 0.707, 0.0)
    p = W.ProjectScript(48000, 1024)
    p.set_length(0.5)
    for k, (n, mode) in enumerate(((20011, ""), (9001, "normalize-seperate"))):
        p.assets["a%d" % k] = W.Asset(W.noise_int16(50 + k, n))
        p.load_sample("a%d" % k, "a%d" % k, mode)
    p.add_sampleloop("l0", 0.7, 30.0, "a0")     # read by the EQ itself (term kinds 1 / 3)
    p.add_sampleloop("l1", 0.4, 0.0, "a1")
    p.add_sum("stage", 0.5, -45.0)              # one input: a gain / pan stage, read through (term kind 4)
    p.connect("l1", "stage")
    EP.add_eq(p, "e", "l0", *case)
    p.connect("stage", "e")
    p.set_output("e")
    built = p.build(gpu_api)
    a = render_f32(gpu_api, built, "l0", p.cs)
    b = render_f32(gpu_api, built, "stage", p.cs)
    x = (np.float32(0.0) + a) + b               # sum_inputs (extensions.rs:310-319), f32, in connect() order
    for packed in (1, 0):
        y = render_f32(gpu_api, built, "e", p.cs, packed_samples=packed)
        assert_close(y, x, twin_p(coeffs(gpu_api, 48000, *case), x), "inlined terms, packed_samples %d" % packed)


def test_a_non_finite_input_frame_leaves_later_frames_finite(gpu_api):
    """An infinite sample in a loop source: its frames' p are the input itself, the state never sees it."""
    case = ("lowshelf", 500.0, 0.707, 12.0)
    bl, cs = 1024, 12
    raw = W.noise_int16(9, 30011).astype(np.float32).reshape(-1).copy()   # interleaved 16-bit words as floats
    raw[2 * 5000] = np.inf          # frame 5 000, left
    raw[2 * 7000 + 1] = np.nan      # frame 7 000, right
    sb = gpu_api.SampleBank(48000)
    sb.add_decoded("a", raw, 2, 48000, 16, "")
    fb = gpu_api.FlowwBank(48000, bl)
    g = gpu_api.Graph(bl, 48000)
    g.add_sampleloop("l", 0.5, 0.0, sb.get_index("a"))
    g.add_sum("bus", 1.0, 0.0)
    g.add_eq("e", 1.0, 0.0, 1.0, *case)
    assert g.connect("l", "bus") and g.connect("bus", "e")
    built = (sb, fb, g)
    x = render_f32(gpu_api, built, "bus", cs)
    bad = ~np.isfinite(x)
    assert bad.sum() == 2 and not np.isfinite(x[5000, 0]) and not np.isfinite(x[7000, 1])
    y = render_f32(gpu_api, built, "e", cs)
    assert (np.isfinite(y) == np.isfinite(x)).all()   # only the input's own non-finite samples
    want, end = NE.eq(x, coeffs(gpu_api, 48000, *case))
    ok = np.isfinite(x).all(axis=1)
    assert_close(y[ok], x[ok], twin_p(coeffs(gpu_api, 48000, *case), x)[ok], "around non-finite frames")
    assert np.isfinite(end).all()


def test_front_end_renders_a_drum_bus_with_an_eq(gpu_api, tmp_path):
    # the drum bus `drums` feeds the band-pass in front of the output: put the EQ in between
    p = fx_rig.into_the_drum_bus("add_eq", ("eq", 1.0, 0.0, 1.0, "peak", 180.0, 1.5, 9.0))
    mem = fx_rig.front_end_renders(gpu_api, tmp_path, p, 'add_eq("eq",', '"peak"')
    fx_rig.front_end_words_differ(gpu_api, tmp_path, W.drum_project(seconds=1.0), mem)


def test_guard_keeps_the_scan_and_fast_sines_in_front_of_an_eq(gpu_api):
    """A scanned band-pass chain plus fast sines in front of a +12 dB peak EQ, in the front-end's defaults (band_mode 2,
    sine_mode 2): within 1e-6 RMS of the exact forms (band_mode 0, sine_mode 1), and the upstream launches are the scan forms."""
    p = fx_rig.gpu_guard_project("add_eq", "e", ("peak", 1000.0, 2.0, 12.0), False)
    outs, names = {}, {}
    for mode, (bm, sm) in (("guard", (2, 2)), ("exact", (0, 1))):
        sb, fb, g = p.build(gpu_api)
        g.set_option("band_mode", bm)
        g.set_option("sine_mode", sm)
        g.set_profiling(1)
        outs[mode] = g.render_all(sb, fb, p.cs, 16, want_pcm=False)[1]
        names[mode] = list(g.kernel_times())
        if mode == "guard":
            st = g.band_guard_stats()
            assert st["audits"] >= 1 and st["redos"] == 0 and st["last_est"] > 0.0, st
    rms = float(np.sqrt(np.mean((outs["guard"].astype(np.float64) - outs["exact"].astype(np.float64)) ** 2)))
    print("guarded scan + fast sines in front of a +12 dB peak: rms %.3g against the exact forms" % rms)
    assert rms <= 1e-6 and np.abs(outs["exact"]).max() > 0.05
    assert "k_band_scan" in names["guard"] and "k_sine_probe" in names["guard"], names["guard"]
    assert not any(n in names["guard"] for n in ("k_band_pass", "k_band_spec")), names["guard"]
    assert "k_band_scan" not in names["exact"] and "k_sine_probe" not in names["exact"], names["exact"]
    for m in names:
        assert [n for n in names[m] if n.startswith("k_eq")] == EQ_LAUNCHES, names[m]


def test_kernel_names_with_and_without_an_eq(gpu_api):
    fx_rig.projects_without_the_kind_launch_no_kernel_of_it(gpu_api, "k_eq")
    p = EP.base_project("drums")
    EP.add_eq(p, "e", "bus", *CHUNK)
    p.set_output("e")
    sb, fb, g = p.build(gpu_api)
    g.set_profiling(1)
    g.render_all(sb, fb, p.cs, 16, want_f32=False)
    kt = g.kernel_times()
    assert [n for n in kt if n.startswith("k_eq")] == EQ_LAUNCHES, list(kt)
    assert all(kt[n][1] == 1 for n in EQ_LAUNCHES), kt
