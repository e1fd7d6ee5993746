"""The compressor vertex on the device (td_graph_add_compressor) against its float64 twin
(tests/np_compressor.py, the serial restatement of the definition in include/termdaw_amd.h).

The input of the vertex under test always comes from the engine itself: a second render of the same graph with set_output on
the vertex in front, read as f32 -- the oracle-verified part of the graph is not restated here.

Bounds.  wet = 1, gain = 1, angle = 0: |y - want| <= 2^-23 |want| + the smallest subnormal, per value -- the chain is f64 with
one rounding to f32 (half an ulp, 2^-24 relative); the factor 2 covers a last-bit difference between the device's and numpy's
f64 log10 / pow (and the scans' f64 re-association) flipping that rounding.  With wet in (0, 1), pan and gain:
4 x 2^-23 x max(|dry|, |p|) x |amplitude| absolute -- three more f32 operations of the lerp, two of pan / gain, each half an
ulp of an operand no larger than that.  PCM cases: within one word of the twin's quantised value."""
import itertools
import os
import sys

import numpy as np
import pytest

from termdaw_amd import workloads as W

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fx_rig  # noqa: E402
import np_compressor as NC  # noqa: E402
from np_twin import pan_gain  # noqa: E402
from fx_rig import MIX, REL, _pull_all, _quantise16, assert_close_f32 as assert_close, build, render_f32  # noqa: E402

pytestmark = pytest.mark.gpu

PARAMS = ["threshold_db", "ratio", "attack_ms", "release_ms", "knee_db", "makeup_db"]


def base_project(kind, sr=48000, bl=1024, seconds=0.5, seed=0):
    """Sources -> Sum `bus` (the vertex in front of the compressors under test)."""
    p = W.ProjectScript(sr, bl)
    p.set_length(seconds)
    p.set_render_samplerate(sr)
    if kind == "drums":   # kick and snare hits through sample_multi
        p.assets["kick"] = W.Asset(W.kick_int16(12 + seed, 15000, sr), sr=sr)
        p.assets["snare"] = W.Asset(W.snare_int16(5 + seed, 9000), sr=sr)
        p.load_sample("kick", "kick", "")
        p.load_sample("snare", "snare", "")
        n = max(1, int(seconds / 0.125))
        p.event_files["k"] = np.array([(0.25 * i + 0.002, 36.0, 1.0 - 0.1 * (i % 4)) for i in range((n + 1) // 2)], np.float32)
        p.event_files["s"] = np.array([(0.125 * i + 0.06, 38.0, 0.2 + 0.15 * (i % 5)) for i in range(n)], np.float32)
        p.load_midi_floww("k", "k")
        p.load_midi_floww("s", "s")
        p.add_sample_multi("kick", 0.9, 0.0, "kick", "k", -1)
        p.add_sample_multi("snare", 0.6, 25.0, "snare", "s", -1)
        srcs = ["kick", "snare"]
    elif kind == "noise":
        p.assets["n"] = W.Asset(W.noise_int16(31 + seed, 20011), sr=sr)
        p.assets["m"] = W.Asset(W.noise_int16(32 + seed, 7001), sr=sr)
        p.load_sample("n", "n", "")
        p.load_sample("m", "m", "normalize-seperate")
        p.add_sampleloop("n", 0.5, 0.0, "n")
        p.add_sampleloop("m", 0.02, -40.0, "m")
        srcs = ["n", "m"]
    else:                 # silence, then one burst (and silence again once it has rung out)
        p.assets["b"] = W.Asset(W.noise_int16(77 + seed, int(0.12 * sr)), sr=sr)
        p.assets["t"] = W.Asset(W.tone_int16(78 + seed, int(0.05 * sr)), sr=sr)
        p.load_sample("b", "b", "")
        p.load_sample("t", "t", "")
        p.event_files["b"] = np.array([(0.21, 60.0, 0.9)], np.float32)
        p.event_files["t"] = np.array([(0.23, 60.0, 0.5)], np.float32)
        p.load_midi_floww("b", "b")
        p.load_midi_floww("t", "t")
        p.add_sample_multi("b", 1.0, 0.0, "b", "b", -1)
        p.add_sample_multi("t", 0.7, -20.0, "t", "t", -1)
        srcs = ["b", "t"]
    p.add_sum("bus", 1.0, 0.0)
    for s in srcs:
        p.connect(s, "bus")
    p.set_output("bus")
    return p


def add_comp(p, name, src, wet=1.0, gain=1.0, angle=0.0, **kw):
    p.add_compressor(name, gain, angle, wet, *[kw[k] for k in PARAMS])
    p.connect(src, name)


GRID = list(itertools.product((0.0, 1.0, 40.0), (1.0, 100.0, 2000.0), (1.0, 2.0, 1000.0)))   # attack, release, ratio


@pytest.mark.parametrize("sr", [44100, 48000, 96000])
@pytest.mark.parametrize("kind", ["drums", "noise", "burst"])
@pytest.mark.parametrize("knee", [0.0, 9.0])
def test_grid_matches_the_twin(gpu_api, sr, kind, knee):
    p = base_project(kind, sr=sr)
    combos = []
    for i, (att, rel, ratio) in enumerate(GRID):
        kw = dict(threshold_db=-30.0 if kind != "noise" else -20.0, ratio=ratio, attack_ms=att, release_ms=rel, knee_db=knee,
                  makeup_db=[0.0, 6.0, -3.5][i % 3])
        add_comp(p, "c%d" % i, "bus", **kw)
        combos.append(kw)
    built = build(gpu_api, p)
    x = render_f32(gpu_api, built, "bus", p.cs)
    assert np.abs(x).max() > 0.05 and p.cs * p.bl > 5 * 2048
    reduced = 0
    for i, kw in enumerate(combos):
        y = render_f32(gpu_api, built, "c%d" % i, p.cs)
        want, _ = NC.compress(x, sr, **kw)
        assert_close(y, want, "%s %d %s" % (kind, sr, kw))
        reduced += int(kw["ratio"] > 1.0 and np.abs(want.astype(np.float64) - x * 10.0 ** (kw["makeup_db"] / 20.0)).max() > 1e-3)
    assert reduced == sum(1 for kw in combos if kw["ratio"] > 1.0)   # (the grid really compresses)
    assert np.array_equal(render_f32(gpu_api, built, "bus", p.cs), x)   # (and every render above saw this input)


# (of the shared bodies the compressor takes the mix test alone: its bound is on the output as it stands, its cases are keywords)
COMP = fx_rig.FxKind("compressor", "k_comp", None, lambda p, name, src, case, **kw: add_comp(p, name, src, **kw, **case), base_project,
                     dict(threshold_db=-28.0, ratio=5.0, attack_ms=2.0, release_ms=60.0, knee_db=6.0, makeup_db=3.0), None, None,
                     twin=lambda api, sr, case, x: (NC.compress(x, sr, processed=True, **case)[0], x),
                     mix=lambda api, sr, case, x, **kw: NC.compress(x, sr, **kw, **case)[0])


@pytest.mark.parametrize("wet,gain,angle", MIX)
def test_wet_pan_and_gain(gpu_api, wet, gain, angle):
    fx_rig.wet_pan_and_gain(gpu_api, COMP, wet, gain, angle, vertex="c")


def test_unit_ratio_and_dry_pass_the_input_through(gpu_api):
    p = base_project("drums")
    add_comp(p, "unit", "bus", threshold_db=-40.0, ratio=1.0, attack_ms=3.0, release_ms=50.0, knee_db=12.0, makeup_db=0.0)
    add_comp(p, "dry", "bus", wet=0.0, threshold_db=-40.0, ratio=20.0, attack_ms=3.0, release_ms=50.0, knee_db=0.0, makeup_db=9.0)
    add_comp(p, "almost", "bus", wet=0.00009, threshold_db=-40.0, ratio=20.0, attack_ms=3.0, release_ms=50.0, knee_db=0.0, makeup_db=9.0)
    built = build(gpu_api, p)
    x = render_f32(gpu_api, built, "bus", p.cs)
    for name in ("unit", "dry", "almost"):
        y = render_f32(gpu_api, built, name, p.cs)
        assert np.array_equal(y, x), (name, np.argwhere(y != x)[:4].tolist())
    g = built[2]
    g.set_profiling(1)
    render_f32(gpu_api, built, "dry", p.cs)
    assert not any(n.startswith("k_comp") for n in g.kernel_times())   # wet < 0.0001: a plain sum launch


CHUNK_KW = dict(threshold_db=-26.0, ratio=4.0, attack_ms=5.0, release_ms=400.0, knee_db=6.0, makeup_db=2.0)


@pytest.mark.parametrize("bl", [1024, 64])
def test_chunked_and_pulled_renders_match_the_twin(gpu_api, bl):
    """20 s: whole, in >= 3 chunks, and by block pulls of `bl` frames -- each inside the bound, each bitwise repeatable."""
    p = base_project("drums", bl=bl, seconds=20.0)
    add_comp(p, "c", "bus", **CHUNK_KW)
    built = build(gpu_api, p)
    n = p.cs * bl
    x = render_f32(gpu_api, built, "bus", p.cs)
    want, end = NC.compress(x, 48000, **CHUNK_KW)
    forms = {}
    forms["whole"] = [render_f32(gpu_api, built, "c", p.cs) for _ in range(2)]
    cap = (n // 3 // bl) * bl - 7 * bl
    assert n / cap > 3
    forms["chunks"] = [render_f32(gpu_api, built, "c", p.cs, max_chunk_frames=cap) for _ in range(2)]
    built[2].set_option("max_chunk_frames", 1 << 24)
    forms["pulls"] = [_pull_all(gpu_api, built, "c", p.cs) for _ in range(2)]
    for name, (a, b) in forms.items():
        assert a.shape == want.shape
        assert_close(a, want, "%s bl %d" % (name, bl))
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), name
    # the detector really carries state across the cuts: restarting it at every chunk would be far outside the bound
    restart, _ = NC.compress(x[cap:2 * cap], 48000, **CHUNK_KW)
    assert np.abs(restart.astype(np.float64) - want[cap:2 * cap]).max() > 1e-3
    assert np.array_equal(render_f32(gpu_api, built, "bus", p.cs), x)
    # a set_time in the middle of pulling restarts the detector from (0, 0): two pulls, a jump, one pull (two fresh builds:
    # one for the vertex, one for its input)
    half = (p.cs // 2) * bl
    got = []
    for out in ("c", "bus"):
        sb, fb, g = p.build(gpu_api)
        assert g.set_output(out)
        for _ in range(2):
            g.render(sb, fb)
            fb.set_time_to_next_block()
        fb.set_time(half)
        g.set_time(half)
        got.append(np.stack(g.render(sb, fb), axis=1))
    assert np.abs(got[1]).max() > 0.01
    assert_close(got[0], NC.compress(got[1], 48000, **CHUNK_KW)[0], "pull after set_time")


def test_batch_members_are_bitwise_their_own_renders(gpu_api):
    projects = []
    for i in range(8):
        kind = ["drums", "noise", "burst"][i % 3]
        p = base_project(kind, seconds=1.0, seed=i)
        kw = dict(threshold_db=-35.0 + 3 * i, ratio=[2.0, 4.0, 1000.0][i % 3], attack_ms=[0.0, 1.0, 40.0][(i // 2) % 3],
                  release_ms=[1.0, 100.0, 2000.0][i % 3], knee_db=[0.0, 6.0][i % 2], makeup_db=float(i) - 3.0)
        add_comp(p, "c", "bus", wet=[1.0, 0.6][i % 2], gain=[1.0, 0.7][(i // 4) % 2], **kw)
        if i % 4 == 1:     # a second one in series, as the output
            add_comp(p, "c2", "c", **dict(kw, threshold_db=-20.0))
            p.set_output("c2")
        elif i % 4 == 2:   # in front of a Normalize output
            p.add_normalize("out", 1.0, 0.0)
            p.connect("c", "out")
            p.set_output("out")
        else:
            p.set_output("c")
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
    for rep in range(2):
        batch.rewind()
        assert batch.render_all(cs, 16) == cs * 1024
        for i in range(8):
            assert np.array_equal(batch.read_pcm(i, cs), own[i][rep]), (rep, i)


def test_in_front_of_a_normalize_output(gpu_api):
    kw = dict(threshold_db=-30.0, ratio=8.0, attack_ms=1.0, release_ms=150.0, knee_db=4.0, makeup_db=0.0)
    p = base_project("drums", seconds=1.0)
    add_comp(p, "c", "bus", **kw)
    p.add_normalize("out", 1.0, 0.0)
    p.connect("c", "out")
    built = build(gpu_api, p)
    x = render_f32(gpu_api, built, "bus", p.cs)
    c, _ = NC.compress(x, 48000, **kw)
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
    # (a last-bit difference in c moves a block's peak by an ulp at most: one more half-ulp step on top of the vertex' bound)
    assert (np.abs(f.astype(np.float64) - want) <= 2.0 * REL * np.abs(want) + NC.F32_TINY).all()
    assert np.abs(pcm.astype(np.int64) - _quantise16(want)).max() <= 1


def test_as_a_stem_and_two_in_series(gpu_api):
    kw1 = dict(threshold_db=-30.0, ratio=3.0, attack_ms=2.0, release_ms=80.0, knee_db=6.0, makeup_db=4.0)
    kw2 = dict(threshold_db=-12.0, ratio=1000.0, attack_ms=0.0, release_ms=30.0, knee_db=0.0, makeup_db=0.0)
    p = base_project("drums", seconds=1.0)
    add_comp(p, "c1", "bus", **kw1)
    add_comp(p, "c2", "c1", gain=0.8, angle=-20.0, **kw2)
    p.add_sum("post", 0.5, 10.0)
    p.connect("c2", "post")
    built = build(gpu_api, p)
    x = render_f32(gpu_api, built, "bus", p.cs)
    y1 = render_f32(gpu_api, built, "c1", p.cs)
    assert_close(y1, NC.compress(x, 48000, **kw1)[0], "first of two")
    # the second one against the twin on what the first one really handed it
    y2 = render_f32(gpu_api, built, "c2", p.cs)
    w2, _ = NC.compress(y1, 48000, gain=0.8, angle=-20.0, **kw2)
    proc, _ = NC.compress(y1, 48000, processed=True, **kw2)
    al, ar = pan_gain(np.ones(1, np.float32), np.ones(1, np.float32), 0.8, -20.0)
    lim = 4.0 * REL * np.maximum(np.abs(y1), np.abs(proc)).astype(np.float64) * np.abs(np.array([float(al[0]), float(ar[0])]))[None, :] + NC.F32_TINY
    assert (np.abs(y2.astype(np.float64) - w2) <= lim).all()
    assert np.abs(y2).max() <= 0.8 * 10.0 ** (-12.0 / 20.0) * 1.001   # ratio 1000, no attack: a limiter at the threshold
    # both as stems of a render whose output sits downstream
    sb, fb, g = built
    g.set_output("post")
    g.set_stems(["c2", "c1"])
    fb.set_time(0)
    g.set_time(0)
    g.render_all(sb, fb, p.cs, 16)
    assert np.abs(g.read_stem_pcm(0).astype(np.int64) - _quantise16(w2)).max() <= 1
    assert np.abs(g.read_stem_pcm(1).astype(np.int64) - _quantise16(y1)).max() == 0
    g.set_stems([])


def test_fed_by_an_inlined_loop_source_and_a_gain_stage(gpu_api):
    kw = dict(threshold_db=-24.0, ratio=4.0, attack_ms=1.0, release_ms=100.0, knee_db=6.0, makeup_db=0.0)
    p = W.ProjectScript(48000, 1024)
    p.set_length(0.5)
    for k, (n, mode) in enumerate(((20011, ""), (9001, "normalize-seperate"))):
        p.assets["a%d" % k] = W.Asset(W.noise_int16(50 + k, n))
        p.load_sample("a%d" % k, "a%d" % k, mode)
    p.add_sampleloop("l0", 0.7, 30.0, "a0")     # read by the compressor itself (term kinds 1 / 3)
    p.add_sampleloop("l1", 0.4, 0.0, "a1")
    p.add_sum("stage", 0.5, -45.0)              # one input: a gain / pan stage, read through (term kind 4)
    p.connect("l1", "stage")
    add_comp(p, "c", "l0", **kw)
    p.connect("stage", "c")
    p.set_output("c")
    built = p.build(gpu_api)
    a = render_f32(gpu_api, built, "l0", p.cs)
    b = render_f32(gpu_api, built, "stage", p.cs)
    x = (np.float32(0.0) + a) + b               # sum_inputs (extensions.rs:310-319), f32, in connect() order
    for packed in (1, 0):
        y = render_f32(gpu_api, built, "c", p.cs, packed_samples=packed)
        assert_close(y, NC.compress(x, 48000, **kw)[0], "inlined terms, packed_samples %d" % packed)


def test_projects_without_a_compressor_launch_no_compressor_kernel(gpu_api):
    fx_rig.projects_without_the_kind_launch_no_kernel_of_it(gpu_api, "k_comp")
    p = base_project("drums")
    add_comp(p, "c", "bus", **CHUNK_KW)
    p.set_output("c")
    sb, fb, g = p.build(gpu_api)
    g.set_profiling(1)
    g.render_all(sb, fb, p.cs, 16, want_f32=False)
    names = list(g.kernel_times())
    assert [n for n in names if n.startswith("k_comp")] == ["k_comp_detect", "k_comp_carry_y1", "k_comp_env", "k_comp_carry_yl", "k_comp_apply"], names


def test_front_end_renders_a_compressed_drum_bus(gpu_api, tmp_path):
    # the drum bus `drums` feeds the band-pass in front of the output: put the compressor in between
    p = fx_rig.into_the_drum_bus("add_compressor", ("comp", 1.0, 0.0, 1.0, -24.0, 4.0, 2.0, 120.0, 6.0, 3.0))
    mem = fx_rig.front_end_renders(gpu_api, tmp_path, p, 'add_compressor("comp",')
    fx_rig.front_end_words_differ(gpu_api, tmp_path, W.drum_project(seconds=1.0), mem)
