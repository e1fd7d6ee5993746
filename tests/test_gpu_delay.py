"""The feedback delay vertex on the device (td_graph_add_delay) against its float64 twin (tests/np_delay.py, the
serial restatement of the definition in include/termdaw_amd.h), run on the engine's own constants (td_delay_params).

The input of the vertex under test always comes from the engine itself: a second render of the same graph with set_output on
the vertex in front, read as f32 -- the oracle-verified part of the graph is not restated here.

Bounds.  wet = 1, gain = 1, angle = 0, per value:  |p' - p| <= 2^-23 |p| + E max|p| on the echoed signal p = (float)(x + w),
carried through the definition's f32 lerp to the vertex' output (tests/fx_rig.py assert_close, which says why).  The first
term is the one f32 rounding of the chain, which may flip; E covers the float64 re-association of the scan: 8 x what the numpy
emulation of the tiled scan shows over this file's own grid and inputs (tests/delay_projects.py E, derived and re-checked on the
CPU by tests/test_delay_host.py; E <= 2^-28).  Where one tile covers the chunk the vertex takes k_delay_apply alone, nothing is
re-associated and the output has the twin's bits: asserted, with the form read from the launch list.  With wet in (0, 1), pan and
gain: fx_rig.py's mix_bound.  PCM cases: within one word of the twin's quantised value.

Every case prints its worst error over the bound."""
import os
import subprocess
import sys
import wave

import numpy as np
import pytest

from termdaw_amd import workloads as W

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import delay_projects as DP  # noqa: E402
import np_delay as ND  # noqa: E402
import fx_rig as TG  # noqa: E402
from fx_rig import _write_project  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REL, MIX = TG.REL, TG.MIX
THREE = ["k_delay_local", "k_delay_carry", "k_delay_apply"]
build, render_f32, over_bound, mix_bound, _pull_all, _quantise16 = TG.build, TG.render_f32, TG.over_bound, TG.mix_bound, TG._pull_all, TG._quantise16


def assert_close(y, x, p, what=""):
    return TG.assert_close(y, x, p, what, DP.E)


def consts(api, sr, t, f, c):
    D, gs, gc, _ = api.delay_params(sr, t, f, c)
    return D, gs, gc


def twin_p(k, x, line=None):
    return ND.delay(x, *k, processed=True, line=line)[0]


def delay_names(g):
    return [n for n in g.kernel_times() if n.startswith("k_delay")]


@pytest.mark.parametrize("sr", DP.RATES)
@pytest.mark.parametrize("kind", DP.INPUTS)
def test_grid_matches_the_twin(gpu_api, sr, kind):
    cases = DP.grid_cases(sr)
    p = DP.base_project(kind, sr=sr)
    for i, c in enumerate(cases):
        DP.add_delay(p, "d%d" % i, "bus", *c)
    built = build(gpu_api, p)
    g = built[2]
    x = render_f32(gpu_api, built, "bus", p.cs)
    n = p.cs * p.bl
    assert np.abs(x).max() > 0.05
    worst, exact, single = 0.0, 0, 0
    for i, c in enumerate(cases):
        k = consts(gpu_api, sr, *c)
        g.set_profiling(1)
        y = render_f32(gpu_api, built, "d%d" % i, p.cs)
        names = delay_names(g)
        g.set_profiling(0)
        pw = twin_p(k, x)
        want = x + np.float32(1.0) * (pw - x)   # the lerp at wet = 1, f32
        worst = max(worst, assert_close(y, x, pw, "%s %d %s" % (kind, sr, c)))
        same = np.array_equal(y.view(np.uint32), want.view(np.uint32))
        exact += int(same)
        # one tile covers the chunk: k_delay_apply alone, and the twin's bits
        if ND.tiling(n, k[0])[1] == 1:
            single += 1
            assert names == ["k_delay_apply"] and same, (c, names)
        else:
            assert names == THREE, (c, names)
        # the echo sounds: the output is far from the input
        assert np.abs(want.astype(np.float64) - x).max() > 64.0 * (REL + DP.E) * np.abs(x).max(), c
    print("grid %s %d: %d cases (%d single-launch), worst |y - want| %.3g x the plain bound, %d bit-identical to the twin" % (kind, sr, len(cases), single, worst, exact))
    assert 0 < single < len(cases)
    assert np.array_equal(render_f32(gpu_api, built, "bus", p.cs), x)   # (and every render above saw this input)


@pytest.mark.parametrize("tile", ND.TILES)
def test_every_tile_length_matches_the_twin(gpu_api, tile):
    """The candidate steps per tile ("debug.delay_tile"): the same bound, odd and even D."""
    p = DP.base_project("noise", seconds=1.0)
    cases = [(1.0, 0.98, 0.35), (1.5, 0.98, 1.0), (7.3, 0.5, 0.0), (30.0 + 1.0 / 48.0, 0.98, 0.35)]
    for i, c in enumerate(cases):
        DP.add_delay(p, "d%d" % i, "bus", *c)
    built = build(gpu_api, p)
    built[2].set_option("debug.delay_tile", tile)
    x = render_f32(gpu_api, built, "bus", p.cs)
    for i, c in enumerate(cases):
        k = consts(gpu_api, 48000, *c)
        assert_close(render_f32(gpu_api, built, "d%d" % i, p.cs), x, twin_p(k, x), "tile %d %s D %d" % (tile, c, k[0]))
    assert consts(gpu_api, 48000, *cases[3])[0] == 1441


ECHO = (30.0, 0.6, 0.35)
# (of the shared bodies the delay takes the mix test alone: its other placement tests check its line and its launches too)
DELAY = TG.FxKind("delay", "k_delay", THREE, lambda p, name, src, case, **kw: DP.add_delay(p, name, src, *case, **kw), DP.base_project, ECHO, None, DP.E,
                  twin=lambda api, sr, case, x: (twin_p(consts(api, sr, *case), x), x),
                  mix=lambda api, sr, case, x, **kw: ND.delay(x, *consts(api, sr, *case), **kw)[0])


@pytest.mark.parametrize("wet,gain,angle", MIX)
def test_wet_pan_and_gain(gpu_api, wet, gain, angle):
    TG.wet_pan_and_gain(gpu_api, DELAY, wet, gain, angle, vertex="d")


def test_dry_passes_the_input_through_as_a_sum_launch(gpu_api):
    p = DP.base_project("drums")
    DP.add_delay(p, "dry", "bus", *ECHO, wet=0.0)
    DP.add_delay(p, "almost", "bus", *ECHO, wet=0.00009)
    built = build(gpu_api, p)
    x = render_f32(gpu_api, built, "bus", p.cs)
    for name in ("dry", "almost"):
        y = render_f32(gpu_api, built, name, p.cs)
        assert np.array_equal(y, x), (name, np.argwhere(y != x)[:4].tolist())
    g = built[2]
    g.set_profiling(1)
    render_f32(gpu_api, built, "dry", p.cs)
    names = list(g.kernel_times())
    assert not any(n.startswith("k_delay") for n in names) and "k_sum" in names, names   # wet < 0.0001: a plain sum launch


# (block length) -> delay times: D below, equal to and above the block length; and, for 1 024, D = 96 000 above a 65 536-frame chunk
LONG = {1024: (10.0, 1024.0 / 48.0, 30.0, 2000.0), 64: (1.0, 64.0 / 48.0, 30.0)}


@pytest.mark.parametrize("bl", [1024, 64])
def test_chunked_and_pulled_renders_match_the_twin(gpu_api, bl):
    """20 s: whole, in >= 3 chunks, and by block pulls of `bl` frames -- each inside the bound, each bitwise repeatable."""
    p = DP.base_project("drums", bl=bl, seconds=20.0)
    fb_, cr = 0.7, 0.35
    for i, t in enumerate(LONG[bl]):
        DP.add_delay(p, "d%d" % i, "bus", t, fb_, cr)
    built = build(gpu_api, p)
    g = built[2]
    n = p.cs * bl
    x = render_f32(gpu_api, built, "bus", p.cs)
    cap = (n // 3 // bl) * bl - 7 * bl
    assert n / cap > 3
    Ds = []
    for i, t in enumerate(LONG[bl]):
        name = "d%d" % i
        k = consts(gpu_api, 48000, t, fb_, cr)
        Ds.append(k[0])
        pt = twin_p(k, x)
        forms = {}
        forms["whole"] = [render_f32(gpu_api, built, name, p.cs) for _ in range(2)]
        forms["chunks"] = [render_f32(gpu_api, built, name, p.cs, max_chunk_frames=cap) for _ in range(2)]
        if k[0] > 65536:   # D above a chunk: every chunk is one tile, the line is only partly rewritten by each
            g.set_profiling(1)
            forms["short chunks"] = [render_f32(gpu_api, built, name, p.cs, max_chunk_frames=65536) for _ in range(2)]
            kt = g.kernel_times()
            g.set_profiling(0)
            assert [n_ for n_ in kt if n_.startswith("k_delay")] == ["k_delay_apply"] and kt["k_delay_apply"][1] >= 2 * 14, kt
        g.set_option("max_chunk_frames", 1 << 24)
        g.set_profiling(1)
        forms["pulls"] = [_pull_all(gpu_api, built, name, p.cs) for _ in range(2 if i == 0 else 1)]
        names = delay_names(g)
        g.set_profiling(0)
        # a pull is one tile where ceil(bl / D) <= 16 steps: k_delay_apply alone, and then the pulled render has the twin's bits
        one = ND.tiling(bl, k[0])[1] == 1
        assert names == (["k_delay_apply"] if one else THREE), (t, names)
        for form, runs in forms.items():
            assert_close(runs[0], x, pt, "%s bl %d D %d" % (form, bl, k[0]))
            for b in runs[1:]:
                assert np.array_equal(runs[0].view(np.uint32), b.view(np.uint32)), (form, t)
        if one:
            want = x + np.float32(1.0) * (pt - x)
            assert np.array_equal(forms["pulls"][0].view(np.uint32), want.view(np.uint32)), t
        # the line really carries across the cuts: restarting it at a cut is far outside the bound
        if 2 * cap + k[0] < n:
            restart = twin_p(k, x[cap:2 * cap])
            worst, _ = over_bound(restart, pt[cap:2 * cap], DP.E)
            assert worst > 1000.0, (t, worst)
    assert Ds[0] < bl and Ds[1] == bl and Ds[2] > bl, Ds
    assert np.array_equal(render_f32(gpu_api, built, "bus", p.cs), x)
    # a set_time in the middle of pulling restarts the line from zero: two pulls, a jump, two pulls (two fresh builds: one for the
    # vertex, one for its input); the twin starts from an empty line at the jump
    half = (p.cs // 2) * bl
    k = consts(gpu_api, 48000, LONG[bl][0], fb_, cr)
    got = []
    for out in ("d0", "bus"):
        sb, fb, g2 = p.build(gpu_api)
        assert g2.set_output(out)
        for _ in range(2):
            g2.render(sb, fb)
            fb.set_time_to_next_block()
        fb.set_time(half)
        g2.set_time(half)
        blocks = []
        for _ in range(2):
            blocks.append(np.stack(g2.render(sb, fb), axis=1))
            fb.set_time_to_next_block()
        got.append(np.concatenate(blocks))
    assert np.abs(got[1]).max() > 0.01
    assert_close(got[0], got[1], twin_p(k, got[1]), "pulls after set_time")


def test_the_line_is_counted_and_goes_with_the_vertices(gpu_api):
    p = DP.base_project("drums")
    DP.add_delay(p, "d", "bus", 2000.0, 0.5, 0.0)
    sb, fb, g = p.build(gpu_api)
    assert g.set_output("bus")
    g.render_all(sb, fb, p.cs, 16)
    before = g.device_bytes()
    assert g.set_output("d")
    fb.set_time(0)
    g.set_time(0)
    g.render_all(sb, fb, p.cs, 16)
    assert g.device_bytes() - before >= 16 * 96000   # (the line; and perhaps one more edge buffer)
    assert g.device_bytes() - before < 16 * 96000 + 4 * 8 * (p.cs * p.bl + 4)
    # td_graph_reset takes the vertices and their lines (the edge-buffer pool stays): the line's bytes come off the count
    with_line = g.device_bytes()
    gpu_api.lib().td_graph_reset(g.h)
    # (... and the event tables of the vertices that went, a few kilobytes)
    assert 16 * 96000 <= with_line - g.device_bytes() < 16 * 96000 + (1 << 20), (with_line, g.device_bytes(), before)


def test_batch_members_are_bitwise_their_own_renders(gpu_api):
    projects = []
    for i in range(8):
        kind = ["drums", "noise", "burst"][i % 3]
        p = DP.base_project(kind, seconds=1.0, seed=i)
        case = ([1.0, 7.3, 30.0, 375.0][i % 4], [0.0, 0.5, 0.98][i % 3], [0.0, 0.35, 1.0][(i // 2) % 3])
        DP.add_delay(p, "d", "bus", *case, wet=[1.0, 0.6][i % 2], gain=[1.0, 0.7][(i // 4) % 2])
        if i % 4 == 1:     # a second one in series, as the output
            DP.add_delay(p, "d2", "d", 120.0, 0.4, 1.0)
            p.set_output("d2")
        elif i % 4 == 2:   # in front of a Normalize output
            p.add_normalize("out", 1.0, 0.0)
            p.connect("d", "out")
            p.set_output("out")
        else:
            p.set_output("d")
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
    batch.set_profiling(True)
    for rep in range(2):   # (two rewinds: the second render enters with an empty line again)
        batch.rewind()
        assert batch.render_all(cs, 16) == cs * 1024
        for i in range(8):
            assert np.array_equal(batch.read_pcm(i, cs), own[i][rep]), (rep, i)
    kt = batch.kernel_times()
    # the launches merge per level: the first delay of the six projects whose chunk takes several tiles in one grid per step,
    # those of the two that one tile covers (375 ms) in k_delay_apply's single-launch instantiation, d2 (120 ms) likewise
    assert [n for n in kt if n.startswith("k_delay")] == THREE and kt["k_delay_local"][1] == 2 and kt["k_delay_apply"][1] == 2 * 3, kt


def test_in_front_of_a_normalize_output(gpu_api):
    case = (30.0, 0.7, 0.35)
    p = DP.base_project("drums", seconds=1.0)
    DP.add_delay(p, "d", "bus", *case)
    p.add_normalize("out", 1.0, 0.0)
    p.connect("d", "out")
    built = build(gpu_api, p)
    x = render_f32(gpu_api, built, "bus", p.cs)
    c, _ = ND.delay(x, *consts(gpu_api, 48000, *case))
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
    c1, c2 = (30.0, 0.7, 0.35), (7.3, 0.5, 1.0)
    p = DP.base_project("drums", seconds=1.0)
    DP.add_delay(p, "d1", "bus", *c1)
    DP.add_delay(p, "d2", "d1", *c2, gain=0.8, angle=-20.0)
    p.add_sum("post", 0.5, 10.0)
    p.connect("d2", "post")
    built = build(gpu_api, p)
    x = render_f32(gpu_api, built, "bus", p.cs)
    y1 = render_f32(gpu_api, built, "d1", p.cs)
    assert_close(y1, x, twin_p(consts(gpu_api, 48000, *c1), x), "first of two")
    # the second one against the twin on what the first one really handed it
    y2 = render_f32(gpu_api, built, "d2", p.cs)
    k2 = consts(gpu_api, 48000, *c2)
    w2, _ = ND.delay(y1, *k2, gain=0.8, angle=-20.0)
    assert (np.abs(y2.astype(np.float64) - w2) <= mix_bound(y1, twin_p(k2, y1), 0.8, -20.0)).all()
    # both as stems of a render whose output sits downstream
    sb, fb, g = built
    g.set_output("post")
    g.set_stems(["d2", "d1"])
    fb.set_time(0)
    g.set_time(0)
    g.render_all(sb, fb, p.cs, 16)
    assert np.abs(g.read_stem_pcm(0).astype(np.int64) - _quantise16(w2)).max() <= 1
    assert np.abs(g.read_stem_pcm(1).astype(np.int64) - _quantise16(y1)).max() == 0
    g.set_stems([])


@pytest.mark.parametrize("case", [(7.3, 0.7, 0.35), (400.0, 0.7, 0.35)])
def test_fed_by_an_inlined_loop_source_and_a_gain_stage(gpu_api, case):
    """The term loop inside k_delay_local (7.3 ms: 69 steps) and inside the single-launch k_delay_apply (400 ms: two steps)."""
    p = W.ProjectScript(48000, 1024)
    p.set_length(0.5)
    for k, (n, mode) in enumerate(((20011, ""), (9001, "normalize-seperate"))):
        p.assets["a%d" % k] = W.Asset(W.noise_int16(50 + k, n))
        p.load_sample("a%d" % k, "a%d" % k, mode)
    p.add_sampleloop("l0", 0.7, 30.0, "a0")     # read by the delay itself (term kinds 1 / 3)
    p.add_sampleloop("l1", 0.4, 0.0, "a1")
    p.add_sum("stage", 0.5, -45.0)              # one input: a gain / pan stage, read through (term kind 4)
    p.connect("l1", "stage")
    DP.add_delay(p, "d", "l0", *case)
    p.connect("stage", "d")
    p.set_output("d")
    built = p.build(gpu_api)
    a = render_f32(gpu_api, built, "l0", p.cs)
    b = render_f32(gpu_api, built, "stage", p.cs)
    x = (np.float32(0.0) + a) + b               # sum_inputs (extensions.rs:310-319), f32, in connect() order
    for packed in (1, 0):
        y = render_f32(gpu_api, built, "d", p.cs, packed_samples=packed)
        assert_close(y, x, twin_p(consts(gpu_api, 48000, *case), x), "inlined terms, packed_samples %d, %s" % (packed, case))


def test_a_non_finite_input_frame_leaves_later_frames_finite(gpu_api):
    """An infinite and a NaN sample in a loop source: their frames' p are the input itself, the line never sees them."""
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
    g.add_delay("short", 1.0, 0.0, 1.0, 1.0, 0.98, 0.35)
    g.add_delay("long", 1.0, 0.0, 1.0, 30.0, 0.98, 1.0)
    assert g.connect("l", "bus") and g.connect("bus", "short") and g.connect("bus", "long")
    built = (sb, fb, g)
    x = render_f32(gpu_api, built, "bus", cs)
    assert (~np.isfinite(x)).sum() == 2 and not np.isfinite(x[5000, 0]) and not np.isfinite(x[7000, 1])
    for name, case in (("short", (1.0, 0.98, 0.35)), ("long", (30.0, 0.98, 1.0))):
        y = render_f32(gpu_api, built, name, cs)
        assert (np.isfinite(y) == np.isfinite(x)).all()   # only the input's own non-finite samples
        k = consts(gpu_api, 48000, *case)
        ok = np.isfinite(x).all(axis=1)
        assert_close(y[ok], x[ok], twin_p(k, x)[ok], "around non-finite frames, %s" % name)


def test_front_end_renders_a_drum_bus_with_a_delay(gpu_api, tmp_path):
    p = W.drum_project(seconds=1.0)
    # the drum bus `drums` feeds the band-pass in front of the output: put the delay in between
    line = ("echo", 1.0, 0.0, 0.5, 125.0, 0.5, 1.0)
    i = p.calls["connect"].index(("drums", "band"))
    p.calls["connect"][i:i + 1] = [("drums", "echo"), ("echo", "band")]
    j = p.script_order.index(("connect", ("drums", "band")))
    p.script_order[j:j + 1] = [("add_delay", line), ("connect", ("drums", "echo")), ("connect", ("echo", "band"))]
    p.calls["add_delay"].append(line)
    d = str(tmp_path / "proj")
    _write_project(p, d)
    out = str(tmp_path / "m.wav")
    r = subprocess.run([sys.executable, "-m", "termdaw_amd", d, "-o", out], env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    st = gpu_api.State(open_dir=d)
    assert st.refresh(), gpu_api.last_error()
    assert 'add_delay("echo",' in st.dump_calls()
    mem = st.render_to_memory()
    with wave.open(out, "rb") as w:
        words = np.frombuffer(w.readframes(w.getnframes()), np.int16).reshape(-1, 2)
    assert words.shape == mem.shape and np.array_equal(words, mem) and np.abs(mem).max() > 1000
    # ... every render of the State starts from an empty line again: once the drum voices that a render leaves sounding (the
    # reference's carried state) have settled -- from the third render on, with and without the delay -- the words repeat
    st.render_to_memory()
    third = st.render_to_memory()
    assert np.array_equal(st.render_to_memory(), third)
    # ... and the delay is really in the path: without it the words differ
    q = W.drum_project(seconds=1.0)
    d2 = str(tmp_path / "plain")
    _write_project(q, d2)
    st2 = gpu_api.State(open_dir=d2)
    assert st2.refresh()
    assert not np.array_equal(st2.render_to_memory(), mem)


def _guard_project(bl=1024, seconds=1.0):
    return TG.gpu_guard_project("add_delay", "d", (10.0, 0.5, 0.35), False, bl=bl, seconds=seconds)


def test_guard_keeps_the_scan_and_fast_sines_in_front_of_a_delay(gpu_api):
    """A scanned band-pass chain plus fast sines in front of a delay with feedback 0.5, in the front-end's defaults (band_mode 2,
    sine_mode 2): within 1e-6 RMS of the exact forms (band_mode 0, sine_mode 1), and the upstream launches are the scan forms."""
    p = _guard_project()
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
    print("guarded scan + fast sines in front of a delay (feedback 0.5): rms %.3g against the exact forms" % rms)
    assert rms <= 1e-6 and np.abs(outs["exact"]).max() > 0.05
    assert "k_band_scan" in names["guard"] and "k_sine_probe" in names["guard"], names["guard"]
    assert not any(n in names["guard"] for n in ("k_band_pass", "k_band_spec")), names["guard"]
    assert "k_band_scan" not in names["exact"] and "k_sine_probe" not in names["exact"], names["exact"]
    for m in names:
        assert [n for n in names[m] if n.startswith("k_delay")] == THREE, names[m]


def test_a_guarded_pull_forced_to_run_again_has_the_exact_bytes(gpu_api):
    """Block pulls under the guard with a bound of 0 (every audited render is done again, with the exact kernels): the line each
    pull entered with is put back in front of the second run, so the pulled frames are the exact modes' to the bit."""
    p = _guard_project(seconds=0.25)
    got = {}
    for mode, (bm, sm, ppb) in (("redo", (2, 2, 0)), ("exact", (0, 1, 200))):
        sb, fb, g = p.build(gpu_api)
        g.set_option("band_mode", bm)
        g.set_option("sine_mode", sm)
        g.set_option("band_guard_ppb", ppb)
        blocks = []
        for _ in range(p.cs):
            l, r = g.render(sb, fb)
            fb.set_time_to_next_block()
            blocks.append(np.stack([l, r], axis=1))
        got[mode] = np.concatenate(blocks)
        if mode == "redo":
            st = g.band_guard_stats()
            assert st["redos"] >= p.cs - 1, st
    assert np.abs(got["exact"]).max() > 0.05
    assert np.array_equal(got["redo"].view(np.uint32), got["exact"].view(np.uint32))


def test_kernel_names_with_and_without_a_delay(gpu_api):
    TG.projects_without_the_kind_launch_no_kernel_of_it(gpu_api, "k_delay")
    p = DP.base_project("drums")
    DP.add_delay(p, "d", "bus", *ECHO)
    p.set_output("d")
    sb, fb, g = p.build(gpu_api)
    g.set_profiling(1)
    g.render_all(sb, fb, p.cs, 16, want_f32=False)
    kt = g.kernel_times()
    assert [n for n in kt if n.startswith("k_delay")] == THREE, list(kt)
    assert all(kt[n][1] == 1 for n in THREE), kt
