"""The saturator vertex on the device (td_graph_add_saturator) against its float64 twin (tests/np_saturator.py,
the serial restatement of the definition in include/termdaw_amd.h), run on the engine's own taps and constants
(td_saturator_taps, td_saturator_params).

The input of the vertex under test always comes from the engine itself: a second render of the same graph with set_output on
the vertex in front, read as f32 -- the oracle-verified part of the graph is not restated here.

Bound: none.  Every output frame is a sum the kernel accumulates from 0.0 in the definition's order, on its own, whatever the
tiling and the chunking: at wet = 1, gain = 1, angle = 0 every finite f32 is BIT-EQUAL to the twin and the non-finite ones sit at
the same frames.  With wet in (0, 1), pan and gain: tests/fx_rig.py's mix_bound (the pan amplitudes come from two sine
implementations).  PCM cases: within one word of the twin's quantised value.  Every test renders 0.25 s at the most."""
import os
import sys

import numpy as np
import pytest

from termdaw_amd import workloads as W

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import np_saturator as NS  # noqa: E402
import sat_projects as SP  # noqa: E402
import fx_rig as TG  # noqa: E402

pytestmark = pytest.mark.gpu
build, render_f32, mix_bound, _pull_all, _quantise16 = TG.build, TG.render_f32, TG.mix_bound, TG._pull_all, TG._quantise16
SOFT = ("soft", 12.0, 0.2, -3.0, 4)


def twin(api, x, case, wet=1.0, gain=1.0, angle=0.0, line=None):
    kind, d, b, o, R = case
    k = api.saturator_params(kind, R, d, b, o)
    return NS.saturator(x, kind, R, d, b, o, wet, gain, angle, h=api.saturator_taps(R) if R > 1 else None, line=line, consts=k[:3])


def assert_same_bits(y, want, what=""):
    fy, fw = np.isfinite(y), np.isfinite(want)
    assert np.array_equal(fy, fw), (what, "non-finite values at other frames", np.argwhere(fy != fw)[:4].tolist())
    a, b = np.where(fy, y, np.float32(0)).view(np.uint32), np.where(fw, want, np.float32(0)).view(np.uint32)
    bad = np.argwhere(a != b)
    assert not len(bad), (what, len(bad), bad[:4].tolist(), [(float(y[i, j]), float(want[i, j])) for i, j in bad[:4]])


def sat_names(kt):
    """The saturator's launches in a kernel_times() reading (read once, while profiling is on), in launch order."""
    return [n for n in kt if n.startswith("k_sat")]


@pytest.mark.parametrize("kind", SP.INPUTS)
def test_grid_has_the_twins_bits(gpu_api, kind):
    cases = SP.grid_cases()
    p = SP.base_project(kind)
    for i, c in enumerate(cases):
        SP.add_saturator(p, "w%d" % i, "bus", *c)
    built = build(gpu_api, p)
    x = render_f32(gpu_api, built, "bus", p.cs)
    assert np.abs(x).max() > 0.05
    moved = 0
    for i, c in enumerate(cases):
        y = render_f32(gpu_api, built, "w%d" % i, p.cs)
        want, _ = twin(gpu_api, x, c)
        assert_same_bits(y, want, "%s %s" % (kind, c))
        lat = 0 if c[4] == 1 else NS.LATENCY
        moved += int(np.abs(y[lat:].astype(np.float64) - x[:len(x) - lat]).max() > 1e-3 * np.abs(x).max())
    print("grid %s: %d cases bit-identical to the twin, %d of them audibly shaped" % (kind, len(cases), moved))
    assert moved >= len(cases) // 2   # (the vertex does something: drive 12 and 36 dB clip every input)
    assert np.array_equal(render_f32(gpu_api, built, "bus", p.cs), x)   # (and every render above saw this input)


@pytest.mark.parametrize("tile", NS.TILES)
def test_every_tile_length_has_the_twins_bits(gpu_api, tile):
    """The candidate frames per workgroup ("debug.sat_tile"): chunks of F - 1, F, F + 1 and 2 F + 63 frames (one block each), and
    a chunk long enough for the two-launch form."""
    for n in (tile - 1, tile, tile + 1, 2 * tile + 63, 5 * 1024 + 1):
        p = SP.base_project("noise+6", bl=n)
        cases = [("hard", 12.0, 0.2, 0.0, 2), ("cubic", 12.0, 0.2, 0.0, 4), ("soft", 36.0, -0.5, 0.0, 8)]
        for i, c in enumerate(cases):
            SP.add_saturator(p, "w%d" % i, "bus", *c)
        built = p.build(gpu_api)
        built[2].set_option("debug.sat_tile", tile)
        x = render_f32(gpu_api, built, "bus", 1)
        assert x.shape == (n, 2)
        built[2].set_profiling(1)
        for i, c in enumerate(cases):
            assert_same_bits(render_f32(gpu_api, built, "w%d" % i, 1), twin(gpu_api, x, c)[0], "tile %d frames %d %s" % (tile, n, c))
        kt = built[2].kernel_times()
        assert sat_names(kt) == (["k_sat"] if n <= 4096 else ["k_sat_sum", "k_sat"]), (n, kt)


@pytest.mark.parametrize("bl", [64, 333, 1024])
def test_chunked_and_pulled_renders_have_the_one_piece_twins_bits(gpu_api, bl):
    """Whole, in chunks of three blocks, and by block pulls of `bl` frames (64: shorter than the line): the one-piece twin's bits."""
    p = SP.base_project("drums", bl=bl)
    cases = [("hard", 12.0, 0.2, 0.0, 2), SOFT, ("cubic", 36.0, -0.5, 0.0, 8), ("cubic", 12.0, 0.0, 0.0, 1)]
    for i, c in enumerate(cases):
        SP.add_saturator(p, "w%d" % i, "bus", *c)
    built = build(gpu_api, p)
    g = built[2]
    x = render_f32(gpu_api, built, "bus", p.cs)
    for i, c in enumerate(cases):
        name = "w%d" % i
        want, _ = twin(gpu_api, x, c)
        assert_same_bits(render_f32(gpu_api, built, name, p.cs), want, "whole %s" % (c,))
        assert_same_bits(render_f32(gpu_api, built, name, p.cs, max_chunk_frames=3 * bl), want, "chunks %s" % (c,))
        g.set_option("max_chunk_frames", 1 << 24)
        g.set_profiling(1)
        got = _pull_all(gpu_api, built, name, p.cs)
        kt = g.kernel_times()
        g.set_profiling(0)
        assert_same_bits(got, want, "pulls %s" % (c,))
        # the launch list of a pull is one launch
        one = "k_sat1" if c[4] == 1 else "k_sat"
        assert sat_names(kt) == [one] and kt[one][1] == p.cs, kt
        # the line really carries across the cuts: restarting it at a cut differs
        if c[4] > 1:
            cut = 3 * bl
            assert not np.array_equal(twin(gpu_api, x[cut:2 * cut], c)[0], want[cut:2 * cut])


def test_a_set_time_restarts_from_a_silent_line(gpu_api):
    bl = 256
    p = SP.base_project("noise-20", bl=bl)
    SP.add_saturator(p, "w", "bus", *SOFT)
    half = (p.cs // 2) * bl
    got = []
    for out in ("w", "bus"):
        sb, fb, g = p.build(gpu_api)
        assert g.set_output(out)
        for _ in range(2):
            g.render(sb, fb)
            fb.set_time_to_next_block()
        fb.set_time(half)
        g.set_time(half)
        blocks = []
        for _ in range(2):
            blocks.append(np.stack(g.render(sb, fb), axis=1))
            fb.set_time_to_next_block()
        got.append(np.concatenate(blocks))
    assert np.abs(got[1]).max() > 0.01
    assert_same_bits(got[0], twin(gpu_api, got[1], SOFT)[0], "pulls after set_time")
    # (... and nothing of the line the first two pulls left: continuing from it gives other values)
    assert not np.array_equal(twin(gpu_api, got[1], SOFT, line=np.full((NS.LINE, 2), 0.05, np.float32))[0], got[0])


@pytest.mark.parametrize("wet,gain,angle", TG.MIX)
def test_wet_pan_and_gain(gpu_api, wet, gain, angle):
    p = SP.base_project("drums")
    SP.add_saturator(p, "w", "bus", *SOFT, wet=wet, gain=gain, angle=angle)
    SP.add_saturator(p, "w1", "bus", "cubic", 12.0, 0.0, 0.0, 1, wet=wet, gain=gain, angle=angle)
    built = build(gpu_api, p)
    x = render_f32(gpu_api, built, "bus", p.cs)
    for name, c in (("w", SOFT), ("w1", ("cubic", 12.0, 0.0, 0.0, 1))):
        y = render_f32(gpu_api, built, name, p.cs)
        want, _ = twin(gpu_api, x, c, wet=wet, gain=gain, angle=angle)
        proc, _ = twin(gpu_api, x, c)
        lat = 0 if c[4] == 1 else NS.LATENCY
        xd = np.concatenate([np.zeros((lat, 2), np.float32), x[:len(x) - lat]])
        lim = mix_bound(xd, proc, gain, angle)
        err = np.abs(y.astype(np.float64) - want.astype(np.float64))
        print("%s wet %g gain %g angle %g: worst error / bound %.3g" % (name, wet, gain, angle, float(np.max(err / lim))))
        assert (err <= lim).all(), (float(np.max(err / lim)), np.argwhere(err > lim)[:4].tolist())
        assert np.abs(want - xd).max() > 1e-3 * wet   # (the vertex does something, in proportion to the mix)


def test_dry_passes_the_input_through_as_a_sum_launch(gpu_api):
    p = SP.base_project("drums")
    SP.add_saturator(p, "dry", "bus", *SOFT, wet=0.0)
    SP.add_saturator(p, "almost", "bus", *SOFT, wet=0.00009)
    built = build(gpu_api, p)
    x = render_f32(gpu_api, built, "bus", p.cs)
    for name in ("dry", "almost"):
        y = render_f32(gpu_api, built, name, p.cs)
        assert np.array_equal(y, x), (name, np.argwhere(y != x)[:4].tolist())   # (no latency either)
    g = built[2]
    g.set_profiling(1)
    render_f32(gpu_api, built, "dry", p.cs)
    names = list(g.kernel_times())
    assert not any(n.startswith("k_sat") for n in names) and "k_sum" in names, names


def test_a_non_finite_input_frame_comes_out_once_at_the_latency(gpu_api):
    """An infinite and a NaN sample in a loop source come out non-finite 64 frames later and nowhere else; every other frame is
    the twin's render of the input with those two samples zeroed.  One of them sits 10 frames in front of a chunk boundary.  (A
    second, clean loop feeds the bus as well: the sample bank scales an asset by figures taken over all its samples, so what the
    asset with the infinite sample contributes elsewhere is the bank's business; the bus the vertex reads is read back as it is.)"""
    bl, cs = 1024, 12
    raw = W.noise_int16(9, 30011).astype(np.float32).reshape(-1).copy()   # interleaved 16-bit words as floats
    raw[2 * 5000] = np.inf               # frame 5 000, left
    raw[2 * (7 * 1024 - 10) + 1] = np.nan   # frame 7 158, right: its output frame lies in the next block
    case = ("soft", 12.0, 0.2, 0.0, 4)
    sb = gpu_api.SampleBank(48000)
    sb.add_decoded("a", raw, 2, 48000, 16, "")
    sb.add_decoded("b", W.noise_int16(10, 30011).astype(np.float32).reshape(-1).copy(), 2, 48000, 16, "")
    fb = gpu_api.FlowwBank(48000, bl)
    g = gpu_api.Graph(bl, 48000)
    g.add_sampleloop("l", 0.5, 0.0, sb.get_index("a"))
    g.add_sampleloop("m", 0.4, 0.0, sb.get_index("b"))
    g.add_sum("bus", 1.0, 0.0)
    g.add_saturator("w", 1.0, 0.0, 1.0, *case)
    assert g.connect("l", "bus") and g.connect("m", "bus") and g.connect("bus", "w")
    built = (sb, fb, g)
    x = render_f32(gpu_api, built, "bus", cs)
    assert (~np.isfinite(x)).sum() == 2 and not np.isfinite(x[5000, 0]) and not np.isfinite(x[7158, 1])
    zeroed = np.where(np.isfinite(x), x, np.float32(0.0))
    assert np.abs(zeroed).max() > 0.05
    ref, _ = twin(gpu_api, zeroed, case)
    assert np.isfinite(ref).all()
    forms = (("whole", render_f32(gpu_api, built, "w", cs)), ("chunks", render_f32(gpu_api, built, "w", cs, max_chunk_frames=bl)),
             ("pulls", _pull_all(gpu_api, built, "w", cs)))
    for form, y in forms:
        bad = np.argwhere(~np.isfinite(y)).tolist()
        assert bad == [[5000 + 64, 0], [7158 + 64, 1]], (form, bad)
        ok = np.isfinite(y)
        assert np.array_equal(y[ok].view(np.uint32), ref[ok].view(np.uint32)), form
        assert_same_bits(y, twin(gpu_api, x, case)[0], form)


def test_the_line_is_counted_and_goes_with_the_vertices(gpu_api):
    p = SP.base_project("drums")
    SP.add_saturator(p, "w", "bus", *SOFT)
    sb, fb, g = p.build(gpu_api)
    assert g.set_output("bus")
    g.render_all(sb, fb, p.cs, 16)
    before = g.device_bytes()
    assert g.set_output("w")
    fb.set_time(0)
    g.set_time(0)
    g.render_all(sb, fb, p.cs, 16)
    assert g.device_bytes() - before >= 2048   # (the line; and perhaps one more edge buffer)
    assert g.device_bytes() - before < 2048 + 4 * 8 * (p.cs * p.bl + 4)
    with_line = g.device_bytes()
    gpu_api.lib().td_graph_reset(g.h)
    # (... and the event tables of the vertices that went, a few kilobytes)
    assert 2048 <= with_line - g.device_bytes() < 2048 + (1 << 20), (with_line, g.device_bytes(), before)


def test_batch_members_are_bitwise_their_own_renders(gpu_api):
    projects = []
    for i in range(8):
        kind = SP.INPUTS[i % 4]
        p = SP.base_project(kind, seed=i)
        case = (NS.KINDS[i % 3], [0.0, 12.0, 36.0][(i // 2) % 3], [0.0, 0.2, -0.5][i % 3], -3.0, [2, 4, 8, 1][i % 4])
        SP.add_saturator(p, "w", "bus", *case, wet=[1.0, 0.6][i % 2], gain=[1.0, 0.7][(i // 4) % 2])
        if i % 4 == 1:     # a second one in series, as the output
            SP.add_saturator(p, "w2", "w", "soft", 6.0, 0.0, 0.0, 2)
            p.set_output("w2")
        elif i % 4 == 2:   # in front of a Normalize output
            p.add_normalize("out", 1.0, 0.0)
            p.connect("w", "out")
            p.set_output("out")
        else:
            p.set_output("w")
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
    for rep in range(2):   # (two rewinds: the second render enters with a silent line again)
        batch.rewind()
        assert batch.render_all(cs, 16) == cs * 1024
        for i in range(8):
            assert np.array_equal(batch.read_pcm(i, cs), own[i][rep]), (rep, i)
    kt = batch.kernel_times()
    # the launches merge per level and oversampling factor: unmerged, a render is ten k_sat (eight w, two w2), eight k_sat_sum and
    # two k_sat1.  Projects i and i + 4 have the same shape and factor, so at most one k_sat per factor (2, 4, 8) plus one for the
    # two w2 (which shares the first group's launch where the levels coincide), one k_sat1, and one k_sat_sum per level that holds
    # filtered vertices (w2 sits below its w: at least two; the three input kinds may sit on different levels: at most four)
    assert sorted(sat_names(kt)) == ["k_sat", "k_sat1", "k_sat_sum"], list(kt)
    assert 2 * 3 <= kt["k_sat"][1] <= 2 * 4 and kt["k_sat1"][1] == 2 * 1 and 2 * 2 <= kt["k_sat_sum"][1] <= 2 * 4, kt


def test_in_front_of_a_normalize_output(gpu_api):
    p = SP.base_project("drums")
    SP.add_saturator(p, "w", "bus", *SOFT)
    p.add_normalize("out", 1.0, 0.0)
    p.connect("w", "out")
    built = build(gpu_api, p)
    x = render_f32(gpu_api, built, "bus", p.cs)
    c, _ = twin(gpu_api, x, SOFT)
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
    assert np.abs(f.astype(np.float64) - want).max() <= 4.0 * TG.REL * np.abs(want).max()


def test_as_a_stem_and_two_in_series(gpu_api):
    c1, c2 = SOFT, ("cubic", 6.0, 0.0, 0.0, 2)
    p = SP.base_project("drums")
    SP.add_saturator(p, "w1", "bus", *c1)
    SP.add_saturator(p, "w2", "w1", *c2, gain=0.8, angle=-20.0)
    p.add_sum("post", 0.5, 10.0)
    p.connect("w2", "post")
    built = build(gpu_api, p)
    x = render_f32(gpu_api, built, "bus", p.cs)
    y1 = render_f32(gpu_api, built, "w1", p.cs)
    assert_same_bits(y1, twin(gpu_api, x, c1)[0], "first of two")
    # the second one against the twin on what the first one really handed it; together they delay by 128 frames
    y2 = render_f32(gpu_api, built, "w2", p.cs)
    w2, _ = twin(gpu_api, y1, c2, gain=0.8, angle=-20.0)
    y1d = np.concatenate([np.zeros((64, 2), np.float32), y1[:-64]])
    assert (np.abs(y2.astype(np.float64) - w2) <= mix_bound(y1d, twin(gpu_api, y1, c2)[0], 0.8, -20.0)).all()
    # both as stems of a render whose output sits downstream
    sb, fb, g = built
    g.set_output("post")
    g.set_stems(["w2", "w1"])
    fb.set_time(0)
    g.set_time(0)
    g.render_all(sb, fb, p.cs, 16)
    assert np.abs(g.read_stem_pcm(0).astype(np.int64) - _quantise16(w2)).max() <= 1
    assert np.abs(g.read_stem_pcm(1).astype(np.int64) - _quantise16(y1)).max() == 0
    g.set_stems([])


def test_two_in_series_have_a_latency_of_128_frames(gpu_api):
    """A one-sample click through two gentle saturators: the output's peak sits 128 frames after the click."""
    bl, cs = 1024, 2
    words = np.zeros(2 * 4096, np.float32)
    words[2 * 700] = words[2 * 700 + 1] = 3000.0
    sb = gpu_api.SampleBank(48000)
    sb.add_decoded("a", words, 2, 48000, 16, "")
    fb = gpu_api.FlowwBank(48000, bl)
    g = gpu_api.Graph(bl, 48000)
    g.add_sampleloop("l", 1.0, 0.0, sb.get_index("a"))
    g.add_sum("bus", 1.0, 0.0)
    g.add_saturator("w1", 1.0, 0.0, 1.0, "soft", 0.0, 0.0, 0.0, 4)
    g.add_saturator("w2", 1.0, 0.0, 1.0, "soft", 0.0, 0.0, 0.0, 8)
    assert g.connect("l", "bus") and g.connect("bus", "w1") and g.connect("w1", "w2")
    y = render_f32(gpu_api, (sb, fb, g), "w2", cs)
    assert int(np.argmax(np.abs(y[:, 0]))) == 700 + 128 and np.abs(y[:, 0]).max() > 0.02


@pytest.mark.parametrize("over", [4, 1])
def test_fed_by_an_inlined_loop_source_and_a_gain_stage(gpu_api, over):
    """The term loop inside k_sat (short chunks: blocks of 1 024 in chunks of 4 096), inside k_sat_sum (the whole render) and
    inside k_sat1."""
    p = W.ProjectScript(48000, 1024)
    p.set_length(0.25)
    for k, (n, mode) in enumerate(((20011, ""), (9001, "normalize-seperate"))):
        p.assets["a%d" % k] = W.Asset(W.noise_int16(50 + k, n))
        p.load_sample("a%d" % k, "a%d" % k, mode)
    p.add_sampleloop("l0", 0.7, 30.0, "a0")     # read by the saturator itself (term kinds 1 / 3)
    p.add_sampleloop("l1", 0.4, 0.0, "a1")
    p.add_sum("stage", 0.5, -45.0)              # one input: a gain / pan stage, read through (term kind 4)
    p.connect("l1", "stage")
    case = ("cubic", 12.0, 0.2, 0.0, over)
    SP.add_saturator(p, "w", "l0", *case)
    p.connect("stage", "w")
    p.set_output("w")
    built = p.build(gpu_api)
    a = render_f32(gpu_api, built, "l0", p.cs)
    b = render_f32(gpu_api, built, "stage", p.cs)
    x = (np.float32(0.0) + a) + b               # sum_inputs (extensions.rs:310-319), f32, in connect() order
    want, _ = twin(gpu_api, x, case)
    for packed in (1, 0):
        for cap in (1 << 24, 4096):
            y = render_f32(gpu_api, built, "w", p.cs, packed_samples=packed, max_chunk_frames=cap)
            assert_same_bits(y, want, "inlined terms, packed_samples %d, chunks of %d" % (packed, cap))


def test_front_end_renders_a_drum_bus_with_a_saturator(gpu_api, tmp_path):
    # the drum bus `drums` feeds the band-pass in front of the output: put the saturator in between
    p = TG.into_the_drum_bus("add_saturator", ("drive", 1.0, 0.0, 0.7, "cubic", 18.0, 0.1, -6.0, 4), seconds=0.25)
    mem = TG.front_end_renders(gpu_api, tmp_path, p, 'add_saturator("drive",', '"cubic"')
    TG.front_end_words_differ(gpu_api, tmp_path, W.drum_project(seconds=0.25), mem)


def _guard_project(bl=1024, seconds=0.25):
    return TG.gpu_guard_project("add_saturator", "w", ("cubic", 6.0, 0.1, 0.0, 4), False, bl=bl, seconds=seconds, notes=TG.SHORT_NOTES)


def test_guard_keeps_the_scan_and_fast_sines_in_front_of_a_saturator(gpu_api):
    """A scanned band-pass chain plus fast sines in front of a saturator, in the front-end's defaults (band_mode 2, sine_mode 2):
    within 1e-6 RMS of the exact forms (band_mode 0, sine_mode 1), and the upstream launches are the scan forms."""
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
    print("guarded scan + fast sines in front of a saturator (cubic, +6 dB): rms %.3g against the exact forms" % rms)
    assert rms <= 1e-6 and np.abs(outs["exact"]).max() > 0.05
    assert "k_band_scan" in names["guard"] and "k_sine_probe" in names["guard"], names["guard"]
    assert not any(n in names["guard"] for n in ("k_band_pass", "k_band_spec")), names["guard"]
    assert "k_band_scan" not in names["exact"] and "k_sine_probe" not in names["exact"], names["exact"]
    for m in names:
        assert [n for n in names[m] if n.startswith("k_sat")] == ["k_sat_sum", "k_sat"], names[m]


def test_a_guarded_pull_forced_to_run_again_has_the_exact_bytes(gpu_api):
    """Block pulls under the guard with a bound of 0 (every audited render is done again, with the exact kernels): the line each
    pull entered with is put back in front of the second run, and the parity with it, so the pulled frames are the exact modes'
    to the bit."""
    p = _guard_project()
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


def test_kernel_names_with_and_without_a_saturator(gpu_api):
    for p in (W.drum_project(seconds=0.25), W.config2(seconds=0.25, n_src=8)):
        sb, fb, g = p.build(gpu_api)
        g.set_profiling(1)
        g.render_all(sb, fb, p.cs, 16, want_f32=False)
        names = list(g.kernel_times())
        assert names and not any(n.startswith("k_sat") for n in names), names
    p = SP.base_project("drums")
    SP.add_saturator(p, "w", "bus", *SOFT)
    SP.add_saturator(p, "w1", "w", "hard", 0.0, 0.0, 0.0, 1)
    p.set_output("w1")
    sb, fb, g = p.build(gpu_api)
    g.set_profiling(1)
    g.render_all(sb, fb, p.cs, 16, want_f32=False)
    kt = g.kernel_times()
    assert sat_names(kt) == ["k_sat_sum", "k_sat", "k_sat1"], list(kt)
    assert all(kt[n][1] == 1 for n in sat_names(kt)), kt
