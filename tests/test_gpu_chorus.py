"""The chorus vertex on the device (td_graph_add_chorus) against its float64 twin (tests/np_chorus.py, the serial
restatement of the definition in include/termdaw_amd.h), run on the engine's own constants (td_chorus_params).

The input of the vertex under test always comes from the engine itself: a second render of the same graph with set_output on
the vertex in front, read as f32 -- the oracle-verified part of the graph is not restated here.

Bound: none.  Every output frame is a sum the kernel accumulates from 0.0 in the definition's order, on its own, from IEEE add,
multiply, floor and fabs alone, whatever the tiling and the chunking: at wet = 1, gain = 1, angle = 0 every finite f32 is
BIT-EQUAL to the twin and the non-finite ones sit at the same frames.  With wet in (0, 1), pan and gain: tests/fx_rig.py's
mix_bound (the pan amplitudes come from two sine implementations).  PCM cases: within one word of the twin's quantised value.
Every test renders 0.25 s at 48 kHz at the most."""
import os
import sys

import numpy as np
import pytest

from termdaw_amd import workloads as W

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import chorus_projects as CP  # noqa: E402
import np_chorus as NC  # noqa: E402
import fx_rig as TG  # noqa: E402

pytestmark = pytest.mark.gpu
SR = 48000
build, render_f32, mix_bound, _pull_all, _quantise16 = TG.build, TG.render_f32, TG.mix_bound, TG._pull_all, TG._quantise16
LUSH = CP.case(3, (20.0, 4.0, 0.8, 0.25), "sine")         # H = 1 216
DEEP = CP.case(2, CP.LONG, "sine")                          # H = 2 432
FLANGE = CP.case(4, CP.SHORT, "triangle")                   # H = 192


def twin(api, x, case, wet=1.0, gain=1.0, angle=0.0, line=None, t0=0):
    k = api.chorus_params(SR, *case)
    return NC.chorus(x, SR, *case, wet=wet, gain=gain, angle=angle, line=line, t0=t0, consts=k[:4])


def assert_same_bits(y, want, what=""):
    fy, fw = np.isfinite(y), np.isfinite(want)
    assert np.array_equal(fy, fw), (what, "non-finite values at other frames", np.argwhere(fy != fw)[:4].tolist())
    a, b = np.where(fy, y, np.float32(0)).view(np.uint32), np.where(fw, want, np.float32(0)).view(np.uint32)
    bad = np.argwhere(a != b)
    assert not len(bad), (what, len(bad), bad[:4].tolist(), [(float(y[i, j]), float(want[i, j])) for i, j in bad[:4]])


def chorus_names(kt):
    """The chorus' launches in a kernel_times() reading (read once, while profiling is on), in launch order."""
    return [n for n in kt if n.startswith("k_chorus")]


@pytest.mark.parametrize("kind", CP.INPUTS)
def test_grid_has_the_twins_bits(gpu_api, kind):
    cases = CP.grid_cases()
    p = CP.base_project(kind)
    for i, c in enumerate(cases):
        CP.add_chorus(p, "c%d" % i, "bus", *c)
    built = build(gpu_api, p)
    x = render_f32(gpu_api, built, "bus", p.cs)
    assert np.abs(x).max() > 0.05
    moved = 0
    for i, c in enumerate(cases):
        y = render_f32(gpu_api, built, "c%d" % i, p.cs)
        want, _ = twin(gpu_api, x, c)
        assert_same_bits(y, want, "%s %s" % (kind, c))
        moved += int(np.abs(y.astype(np.float64) - x).max() > 1e-3 * np.abs(x).max())
    print("grid %s: %d cases bit-identical to the twin, %d of them audibly moved" % (kind, len(cases), moved))
    assert moved == len(cases)   # (the vertex does something: every case delays by 1 ms at the least)
    assert np.array_equal(render_f32(gpu_api, built, "bus", p.cs), x)   # (and every render above saw this input)


@pytest.mark.parametrize("tile", NC.TILES)
def test_every_chunk_length_and_tile_length_has_the_twins_bits(gpu_api, tile):
    """The candidate frames per workgroup ("debug.chorus_tile") on chunks of 63, 64, 65, H - 1, H + 1, 4 096 and 4 097 frames (one
    block each) for the longest line and for one below a tile: one launch up to the inline limit, two above it."""
    cases = [DEEP, FLANGE]
    hs = [gpu_api.chorus_params(SR, *c)[3] for c in cases]
    assert hs == [2432, 192]
    for n in (63, 64, 65, 191, 193, 2431, 2433, 4096, 4097):
        p = CP.base_project("noise+6", bl=n)
        for i, c in enumerate(cases):
            CP.add_chorus(p, "c%d" % i, "bus", *c)
        built = p.build(gpu_api)
        built[2].set_option("debug.chorus_tile", tile)
        x = render_f32(gpu_api, built, "bus", 1)
        assert x.shape == (n, 2)
        built[2].set_profiling(1)
        for i, c in enumerate(cases):
            assert_same_bits(render_f32(gpu_api, built, "c%d" % i, 1), twin(gpu_api, x, c)[0], "tile %d frames %d %s" % (tile, n, c))
        kt = built[2].kernel_times()
        assert chorus_names(kt) == (["k_chorus"] if n <= NC.INLINE else ["k_chorus_sum", "k_chorus"]), (n, kt)


@pytest.mark.parametrize("bl", [64, 333, 1024])
def test_chunked_and_pulled_renders_have_the_one_piece_twins_bits(gpu_api, bl):
    """Whole, in chunks of three blocks, and by block pulls of `bl` frames (64 against a line of 2 432): the one-piece twin's bits."""
    p = CP.base_project("drums", bl=bl)
    cases = [DEEP, LUSH, FLANGE]
    for i, c in enumerate(cases):
        CP.add_chorus(p, "c%d" % i, "bus", *c)
    built = build(gpu_api, p)
    g = built[2]
    x = render_f32(gpu_api, built, "bus", p.cs)
    for i, c in enumerate(cases):
        name = "c%d" % i
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
        assert chorus_names(kt) == ["k_chorus"] and kt["k_chorus"][1] == p.cs, kt
        # the line really carries across the cuts: restarting it at a cut (the LFO kept at the absolute time) differs
        # (at a block boundary past the longest delay, over a stretch where the bus sounds)
        cut = bl * (-(-4096 // bl))
        assert np.abs(x[cut - 2432:cut]).max() > 0.01
        assert not np.array_equal(twin(gpu_api, x[cut:cut + 2432], c, t0=cut)[0], want[cut:cut + 2432])


def test_a_read_that_reaches_the_lines_first_word(gpu_api):
    """D0 + A = 62 - 4.8e-7 frames with H = 64 = floor(D0 + A) + 3 + no rounding up: where the sine polynomial overshoots 1 (by 3.6e-6,
    times A = 20 frames), floor(d) is 62 = H - 2 and the oldest of the four frames read lies exactly H back -- word 0 of the line in
    a pull of 64 frames, the window's first frame in a whole render.  Both have the twin's bits."""
    c = CP.case(1, (0.875, 0.4166666567325592, 2.0, 0.0), "sine")
    D0, A, f, H = gpu_api.chorus_params(SR, *c)[:4]
    assert H == 64 and np.floor(D0 + A) == 61.0
    nn = np.arange(12000, dtype=np.float64) * f
    far = np.floor(D0 + A * NC.lfo("sine", nn - np.floor(nn))) + 2.0
    assert far.max() == H and (far == H).sum() >= 2, (far.max(), int((far == H).sum()))
    p = CP.base_project("noise-20", bl=64)
    CP.add_chorus(p, "c", "bus", *c)
    built = build(gpu_api, p)
    x = render_f32(gpu_api, built, "bus", p.cs)
    assert np.abs(x[np.flatnonzero(far == H) - 64]).max() > 0.0   # (the word that is reached holds a value)
    want, _ = twin(gpu_api, x, c)
    assert_same_bits(render_f32(gpu_api, built, "c", p.cs), want, "whole")
    built[2].set_option("max_chunk_frames", 1 << 24)
    assert_same_bits(_pull_all(gpu_api, built, "c", p.cs), want, "pulls")


def test_a_set_time_restarts_from_a_silent_line_at_the_absolute_times_phase(gpu_api):
    bl = 256
    p = CP.base_project("noise-20", bl=bl)
    CP.add_chorus(p, "c", "bus", *LUSH)
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
        blocks = []
        for _ in range(8):
            blocks.append(np.stack(g.render(sb, fb), axis=1))
            fb.set_time_to_next_block()
        got.append(np.concatenate(blocks))
    assert np.abs(got[1]).max() > 0.01
    assert_same_bits(got[0], twin(gpu_api, got[1], LUSH, t0=half)[0], "pulls after set_time")
    # (the LFO is a function of the absolute time: the twin started at time 0 gives other values ...
    assert not np.array_equal(twin(gpu_api, got[1], LUSH, t0=0)[0], got[0])
    # ... and nothing of the line the first two pulls left is read: continuing from it gives other values)
    h = gpu_api.chorus_params(SR, *LUSH)[3]
    assert not np.array_equal(twin(gpu_api, got[1], LUSH, t0=half, line=np.full((h, 2), 0.05, np.float32))[0], got[0])


@pytest.mark.parametrize("wet,gain,angle", TG.MIX)
def test_wet_pan_and_gain(gpu_api, wet, gain, angle):
    p = CP.base_project("drums")
    CP.add_chorus(p, "c", "bus", *LUSH, wet=wet, gain=gain, angle=angle)
    CP.add_chorus(p, "c1", "bus", *FLANGE, wet=wet, gain=gain, angle=angle)
    built = build(gpu_api, p)
    x = render_f32(gpu_api, built, "bus", p.cs)
    for name, c in (("c", LUSH), ("c1", FLANGE)):
        y = render_f32(gpu_api, built, name, p.cs)
        want, _ = twin(gpu_api, x, c, wet=wet, gain=gain, angle=angle)
        proc, _ = twin(gpu_api, x, c)
        lim = mix_bound(x, proc, gain, angle)
        err = np.abs(y.astype(np.float64) - want.astype(np.float64))
        print("%s wet %g gain %g angle %g: worst error / bound %.3g" % (name, wet, gain, angle, float(np.max(err / lim))))
        assert (err <= lim).all(), (float(np.max(err / lim)), np.argwhere(err > lim)[:4].tolist())
        assert np.abs(want - x).max() > 1e-3 * wet   # (the vertex does something, in proportion to the mix)


def test_dry_passes_the_input_through_as_a_sum_launch(gpu_api):
    p = CP.base_project("drums")
    CP.add_chorus(p, "dry", "bus", *LUSH, wet=0.0)
    CP.add_chorus(p, "almost", "bus", *LUSH, wet=0.00009)
    built = build(gpu_api, p)
    x = render_f32(gpu_api, built, "bus", p.cs)
    for name in ("dry", "almost"):
        y = render_f32(gpu_api, built, name, p.cs)
        assert np.array_equal(y, x), (name, np.argwhere(y != x)[:4].tolist())
    g = built[2]
    g.set_profiling(1)
    before = g.device_bytes()
    render_f32(gpu_api, built, "dry", p.cs)
    names = list(g.kernel_times())
    assert not any(n.startswith("k_chorus") for n in names) and "k_sum" in names, names
    assert g.device_bytes() == before   # (no line either)


def test_a_non_finite_input_frame_makes_its_own_output_frame_non_finite_and_no_other(gpu_api):
    """An infinite and a NaN sample in a loop source come out non-finite at their own frames (the dry leg of the lerp) and nowhere
    else; every other frame is the twin's render of the input with those two samples zeroed.  One of them sits 10 frames in
    front of a block boundary, so the frames that read it as history lie in the next block.  (A second, clean loop feeds the bus
    as well: the sample bank scales an asset by figures taken over all its samples, so what the asset with the infinite sample
    contributes elsewhere is the bank's business; the bus the vertex reads is read back as it is.)"""
    bl, cs = 1024, 12
    raw = W.noise_int16(9, 30011).astype(np.float32).reshape(-1).copy()   # interleaved 16-bit words as floats
    raw[2 * 5000] = np.inf               # frame 5 000, left
    raw[2 * (7 * 1024 - 10) + 1] = np.nan   # frame 7 158, right
    case = FLANGE                        # (delays of 48 .. 144 frames: the reads of frame 7 158 cross into the next block)
    sb = gpu_api.SampleBank(48000)
    sb.add_decoded("a", raw, 2, 48000, 16, "")
    sb.add_decoded("b", W.noise_int16(10, 30011).astype(np.float32).reshape(-1).copy(), 2, 48000, 16, "")
    fb = gpu_api.FlowwBank(48000, bl)
    g = gpu_api.Graph(bl, 48000)
    g.add_sampleloop("l", 0.5, 0.0, sb.get_index("a"))
    g.add_sampleloop("m", 0.4, 0.0, sb.get_index("b"))
    g.add_sum("bus", 1.0, 0.0)
    g.add_chorus("c", 1.0, 0.0, 1.0, *case)
    assert g.connect("l", "bus") and g.connect("m", "bus") and g.connect("bus", "c")
    built = (sb, fb, g)
    x = render_f32(gpu_api, built, "bus", cs)
    assert (~np.isfinite(x)).sum() == 2 and not np.isfinite(x[5000, 0]) and not np.isfinite(x[7158, 1])
    zeroed = np.where(np.isfinite(x), x, np.float32(0.0))
    assert np.abs(zeroed).max() > 0.05
    ref, _ = twin(gpu_api, zeroed, case)
    assert np.isfinite(ref).all()
    forms = (("whole", render_f32(gpu_api, built, "c", cs)), ("chunks", render_f32(gpu_api, built, "c", cs, max_chunk_frames=bl)),
             ("pulls", _pull_all(gpu_api, built, "c", cs)))
    for form, y in forms:
        bad = np.argwhere(~np.isfinite(y)).tolist()
        assert bad == [[5000, 0], [7158, 1]], (form, bad)
        ok = np.isfinite(y)
        # (at the two frames themselves the zeroed input's lerp is finite; everywhere else the bits agree)
        assert np.array_equal(y[ok].view(np.uint32), ref[ok].view(np.uint32)), form
        assert_same_bits(y, twin(gpu_api, x, case)[0], form)


def test_the_line_is_counted_and_goes_with_the_vertices(gpu_api):
    p = CP.base_project("drums")
    CP.add_chorus(p, "c", "bus", *DEEP)
    line = 2 * 2432 * 8
    sb, fb, g = p.build(gpu_api)
    assert g.set_output("bus")
    g.render_all(sb, fb, p.cs, 16)
    before = g.device_bytes()
    assert g.set_output("c")
    fb.set_time(0)
    g.set_time(0)
    g.render_all(sb, fb, p.cs, 16)
    assert g.device_bytes() - before >= line   # (the line; and perhaps more edge buffers)
    assert g.device_bytes() - before < line + 4 * 8 * (p.cs * p.bl + 4)
    with_line = g.device_bytes()
    gpu_api.lib().td_graph_reset(g.h)
    # (... and the event tables of the vertices that went, a few kilobytes)
    assert line <= with_line - g.device_bytes() < line + (1 << 20), (with_line, g.device_bytes(), before)


def test_batch_members_are_bitwise_their_own_renders(gpu_api):
    projects = []
    grid = CP.grid_cases()
    for i in range(8):
        kind = CP.INPUTS[i % 4]
        p = CP.base_project(kind, seed=i)
        CP.add_chorus(p, "c", "bus", *grid[(5 * i) % len(grid)], wet=[1.0, 0.6][i % 2], gain=[1.0, 0.7][(i // 4) % 2])
        if i % 4 == 1:     # a second one in series, as the output
            CP.add_chorus(p, "c2", "c", *FLANGE)
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
    batch.set_profiling(True)
    for rep in range(2):   # (two rewinds: the second render enters with a silent line again)
        batch.rewind()
        assert batch.render_all(cs, 16) == cs * 1024
        for i in range(8):
            assert np.array_equal(batch.read_pcm(i, cs), own[i][rep]), (rep, i)
    kt = batch.kernel_times()
    # the launches merge per level: unmerged, a render is ten k_chorus (eight c, two c2) and ten k_chorus_sum.  c2 sits below its
    # c, so there are at least two levels; the three input kinds may put their c on different levels: at most four
    assert sorted(chorus_names(kt)) == ["k_chorus", "k_chorus_sum"], list(kt)
    assert 2 * 2 <= kt["k_chorus"][1] <= 2 * 4 and kt["k_chorus_sum"][1] == kt["k_chorus"][1], kt


def test_in_front_of_a_normalize_output(gpu_api):
    p = CP.base_project("drums")
    CP.add_chorus(p, "c", "bus", *LUSH)
    p.add_normalize("out", 1.0, 0.0)
    p.connect("c", "out")
    built = build(gpu_api, p)
    x = render_f32(gpu_api, built, "bus", p.cs)
    c, _ = twin(gpu_api, x, LUSH)
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
    c1, c2 = LUSH, FLANGE
    p = CP.base_project("drums")
    CP.add_chorus(p, "c1", "bus", *c1)
    CP.add_chorus(p, "c2", "c1", *c2, gain=0.8, angle=-20.0)
    p.add_sum("post", 0.5, 10.0)
    p.connect("c2", "post")
    built = build(gpu_api, p)
    x = render_f32(gpu_api, built, "bus", p.cs)
    y1 = render_f32(gpu_api, built, "c1", p.cs)
    assert_same_bits(y1, twin(gpu_api, x, c1)[0], "first of two")
    # the second one against the twin on what the first one really handed it
    y2 = render_f32(gpu_api, built, "c2", p.cs)
    w2, _ = twin(gpu_api, y1, c2, gain=0.8, angle=-20.0)
    assert (np.abs(y2.astype(np.float64) - w2) <= mix_bound(y1, twin(gpu_api, y1, c2)[0], 0.8, -20.0)).all()
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
    """The term loop inside k_chorus (short chunks: blocks of 1 024 in chunks of 4 096) and inside k_chorus_sum (the whole
    render)."""
    p = W.ProjectScript(48000, 1024)
    p.set_length(0.25)
    for k, (n, mode) in enumerate(((20011, ""), (9001, "normalize-seperate"))):
        p.assets["a%d" % k] = W.Asset(W.noise_int16(50 + k, n))
        p.load_sample("a%d" % k, "a%d" % k, mode)
    p.add_sampleloop("l0", 0.7, 30.0, "a0")     # read by the chorus itself (term kinds 1 / 3)
    p.add_sampleloop("l1", 0.4, 0.0, "a1")
    p.add_sum("stage", 0.5, -45.0)              # one input: a gain / pan stage, read through (term kind 4)
    p.connect("l1", "stage")
    CP.add_chorus(p, "c", "l0", *LUSH)
    p.connect("stage", "c")
    p.set_output("c")
    built = p.build(gpu_api)
    a = render_f32(gpu_api, built, "l0", p.cs)
    b = render_f32(gpu_api, built, "stage", p.cs)
    x = (np.float32(0.0) + a) + b               # sum_inputs (extensions.rs:310-319), f32, in connect() order
    want, _ = twin(gpu_api, x, LUSH)
    for packed in (1, 0):
        for cap in (1 << 24, 4096):
            y = render_f32(gpu_api, built, "c", p.cs, packed_samples=packed, max_chunk_frames=cap)
            assert_same_bits(y, want, "inlined terms, packed_samples %d, chunks of %d" % (packed, cap))


def test_front_end_renders_a_drum_bus_with_a_chorus(gpu_api, tmp_path):
    # the drum bus `drums` feeds the band-pass in front of the output: put the chorus in between
    p = TG.into_the_drum_bus("add_chorus", ("wide", 1.0, 0.0, 0.5, 3, 20.0, 4.0, 0.8, 0.25, "sine"), seconds=0.25)
    mem = TG.front_end_renders(gpu_api, tmp_path, p, 'add_chorus("wide",', '"sine"')
    TG.front_end_words_differ(gpu_api, tmp_path, W.drum_project(seconds=0.25), mem)


def _guard_project(bl=1024, seconds=0.25):
    return TG.gpu_guard_project("add_chorus", "c", (3, 20.0, 4.0, 0.8, 0.25, "sine"), False, wet=0.5, bl=bl, seconds=seconds, notes=TG.SHORT_NOTES)


def test_guard_keeps_the_scan_and_fast_sines_in_front_of_a_chorus(gpu_api):
    """A scanned band-pass chain plus fast sines in front of a chorus, in the front-end's defaults (band_mode 2, sine_mode 2):
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
    print("guarded scan + fast sines in front of a chorus (3 voices, wet 0.5): rms %.3g against the exact forms" % rms)
    assert rms <= 1e-6 and np.abs(outs["exact"]).max() > 0.05
    assert "k_band_scan" in names["guard"] and "k_sine_probe" in names["guard"], names["guard"]
    assert not any(n in names["guard"] for n in ("k_band_pass", "k_band_spec")), names["guard"]
    assert "k_band_scan" not in names["exact"] and "k_sine_probe" not in names["exact"], names["exact"]
    for m in names:
        assert [n for n in names[m] if n.startswith("k_chorus")] == ["k_chorus_sum", "k_chorus"], names[m]


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


def test_kernel_names_with_and_without_a_chorus(gpu_api):
    for p in (W.drum_project(seconds=0.25), W.config2(seconds=0.25, n_src=8)):
        sb, fb, g = p.build(gpu_api)
        g.set_profiling(1)
        g.render_all(sb, fb, p.cs, 16, want_f32=False)
        names = list(g.kernel_times())
        assert names and not any(n.startswith("k_chorus") for n in names), names
    p = CP.base_project("drums")
    CP.add_chorus(p, "c", "bus", *LUSH)
    p.set_output("c")
    sb, fb, g = p.build(gpu_api)
    g.set_profiling(1)
    g.render_all(sb, fb, p.cs, 16, want_f32=False)
    kt = g.kernel_times()
    assert chorus_names(kt) == ["k_chorus_sum", "k_chorus"], list(kt)
    assert all(kt[n][1] == 1 for n in chorus_names(kt)), kt
