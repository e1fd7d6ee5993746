"""The reverb vertex on the device (td_graph_add_reverb) against its float64 twin (tests/np_reverb.py, the serial
restatement of the definition in include/termdaw_amd.h), run on the engine's own constants (td_reverb_params).

The input of the vertex under test always comes from the engine itself: a second render of the same graph with set_output on
the vertex in front, read as f32 -- the oracle-verified part of the graph is not restated here.

Bounds.  "debug.reverb_form" 0, the serial form, re-associates nothing: at wet = 1, gain = 1, angle = 0 every finite f32 is
BIT-EQUAL to the twin, whatever the window length and the chunking.  Form 1, the wave scan: |p' - p| <= 2^-23 |p| + E max|p| per
value (tests/fx_rig.py's assert_close), E = tests/reverb_projects.py's, derived on the CPU by tests/test_reverb_host.py; with
damp 0 the scan adds only zeros and is bit-equal too.  With wet in (0, 1), pan and gain: fx_rig.py's mix_bound.  PCM: within
one word of the twin's quantised value.  Every project is 0.5 s at the most."""
import os
import sys

import numpy as np
import pytest

from termdaw_amd import workloads as W

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import np_reverb as NR  # noqa: E402
import reverb_projects as RP  # noqa: E402
import fx_rig as TG  # noqa: E402

pytestmark = pytest.mark.gpu
SR = 48000
build, render_f32, mix_bound, _pull_all, _quantise16 = TG.build, TG.render_f32, TG.mix_bound, TG._pull_all, TG._quantise16
HALL = (0.84, 0.2, 1.0, 1.0)       # 48 kHz: shortest line 245, B = 128
SMALL = (0.5, 0.5, 0.5, 0.5)       # shortest line 122, B = 64
LARGE = (1.0, 1.0, 0.5, 2.0)       # shortest line 490, B = 256; g = 0.98, d1 = 0.4; longest line 3 570
REVERB = ["k_reverb_sum", "k_reverb"]


def consts(api, sr, case):
    return api.reverb_params(sr, *case)


def assert_same_bits(y, want, what=""):
    fy, fw = np.isfinite(y), np.isfinite(want)
    assert np.array_equal(fy, fw), (what, "non-finite values at other frames", np.argwhere(fy != fw)[:4].tolist())
    a, b = np.where(fy, y, np.float32(0)).view(np.uint32), np.where(fw, want, np.float32(0)).view(np.uint32)
    bad = np.argwhere(a != b)
    assert not len(bad), (what, len(bad), bad[:4].tolist(), [(float(y[i, j]), float(want[i, j])) for i, j in bad[:4]])


def assert_close(y, x, p, what=""):
    return TG.assert_close(y, x, p, what, E=RP.E)


def lerp1(x, p):
    """What the vertex hands on at wet = 1: the definition's f32 lerp of p."""
    return x + np.float32(1.0) * (p - x)


def reverb_names(kt):
    return [n for n in kt if n.startswith("k_reverb")]


@pytest.mark.parametrize("sr", RP.RATES)
@pytest.mark.parametrize("kind", RP.INPUTS)
def test_grid_serial_form_has_the_twins_bits_and_the_scan_is_inside_the_bound(gpu_api, sr, kind):
    cases = RP.grid_cases()
    p = RP.base_project(kind, sr=sr)
    for i, c in enumerate(cases):
        RP.add_reverb(p, "r%d" % i, "bus", *c)
    built = build(gpu_api, p)
    x = render_f32(gpu_api, built, "bus", p.cs)
    assert np.abs(x).max() > 0.05
    blocks = set()
    for i, c in enumerate(cases):
        k = consts(gpu_api, sr, c)
        blocks.add(k["B"])
        pt, _ = NR.process(x, k)
        want = lerp1(x, pt)
        y0 = render_f32(gpu_api, built, "r%d" % i, p.cs, **{"debug.reverb_form": 0})
        assert_same_bits(y0, want, "form 0 %s %d %s" % (kind, sr, c))
        y1 = render_f32(gpu_api, built, "r%d" % i, p.cs, **{"debug.reverb_form": 1})
        assert_close(y1, x, pt, "form 1 %s %d %s" % (kind, sr, c))
        if k["d1"] == 0.0:   # (damp 0: the scan adds only zeros)
            assert_same_bits(y1, want, "form 1, damp 0 %s %d %s" % (kind, sr, c))
        assert np.abs(y0.astype(np.float64) - x).max() > 1e-3 * np.abs(x).max()   # (the vertex does something)
    assert blocks == ({64, 128, 256} if sr == 44100 else {128, 256}), blocks   # (size 0.5 brings B below 256)
    assert np.array_equal(render_f32(gpu_api, built, "bus", p.cs), x)   # (and every render above saw this input)


@pytest.mark.parametrize("cap", NR.BLOCKS)
def test_every_window_length_gives_the_same_result_on_every_chunk_length(gpu_api, cap):
    """"debug.reverb_block" 64, 128 and 256 on a vertex whose shortest line takes 256, rendered in chunks of one block of 63, 64, 65,
    255, 257 and 4 097 frames: shorter than every line, no multiple of the window, longer than the longest line (3 570) -- the slots
    wrap many times.  Form 0: the twin's bits; form 1: inside the bound."""
    k = consts(gpu_api, SR, LARGE)
    assert k["B"] == 256 and max(NR.lengths(k)) == 3570 and min(NR.lengths(k)) == 490
    for n in (63, 64, 65, 255, 257, 4097):
        p = RP.base_project("noise", bl=n, seconds=0.25)
        RP.add_reverb(p, "r", "bus", *LARGE)
        built = build(gpu_api, p)
        g = built[2]
        g.set_option("debug.reverb_block", cap)
        x = render_f32(gpu_api, built, "bus", p.cs, max_chunk_frames=1 << 24)
        assert len(x) == p.cs * n > 3 * 3570
        pt, _ = NR.process(x, k)
        g.set_profiling(1)
        y0 = render_f32(gpu_api, built, "r", p.cs, max_chunk_frames=n, **{"debug.reverb_form": 0})
        kt = g.kernel_times()
        g.set_profiling(0)
        assert reverb_names(kt) == REVERB and kt["k_reverb"][1] == p.cs, (n, kt)   # (one chunk per block)
        assert_same_bits(y0, lerp1(x, pt), "form 0, cap %d, chunks of %d" % (cap, n))
        y1 = render_f32(gpu_api, built, "r", p.cs, max_chunk_frames=n, **{"debug.reverb_form": 1})
        assert_close(y1, x, pt, "form 1, cap %d, chunks of %d" % (cap, n))


@pytest.mark.parametrize("bl", [64, 333, 1024])
def test_chunked_and_pulled_renders_equal_the_whole_render(gpu_api, bl):
    """Whole, in chunks of three blocks under an odd max_chunk_frames, and by block pulls of `bl` frames: form 0 bit for bit the
    whole render (and the twin), form 1 inside the bound."""
    p = RP.base_project("drums", bl=bl)
    cases = [HALL, SMALL, LARGE]
    for i, c in enumerate(cases):
        RP.add_reverb(p, "r%d" % i, "bus", *c)
    built = build(gpu_api, p)
    g = built[2]
    x = render_f32(gpu_api, built, "bus", p.cs)
    cap = 3 * bl + 1 - (bl % 2)
    assert cap % 2 == 1
    for i, c in enumerate(cases):
        name = "r%d" % i
        k = consts(gpu_api, SR, c)
        pt, _ = NR.process(x, k)
        for form in (0, 1):
            g.set_option("debug.reverb_form", form)
            g.set_profiling(1)
            whole = render_f32(gpu_api, built, name, p.cs, max_chunk_frames=1 << 24)
            assert g.kernel_times()["k_reverb"][1] == 1
            g.set_profiling(1)   # (which also clears the counts)
            chunks = render_f32(gpu_api, built, name, p.cs, max_chunk_frames=cap)
            assert g.kernel_times()["k_reverb"][1] == -(-p.cs // 3)
            g.set_option("max_chunk_frames", 1 << 24)
            g.set_profiling(1)
            pulls = _pull_all(gpu_api, built, name, p.cs)
            kt = g.kernel_times()
            g.set_profiling(0)
            assert reverb_names(kt) == REVERB and kt["k_reverb"][1] == p.cs, kt   # (the summed input is materialised for a pull too)
            for what, y in (("whole", whole), ("chunks", chunks), ("pulls", pulls)):
                if form == 0:
                    assert_same_bits(y, lerp1(x, pt), "form 0 %s bl %d %s" % (what, bl, c))
                    assert np.array_equal(y.view(np.uint32), whole.view(np.uint32)), (what, bl, c)
                else:
                    assert_close(y, x, pt, "form 1 %s bl %d %s" % (what, bl, c))
        # the state really carries across the cuts: restarting it at a cut differs (over a stretch where the bus sounds)
        cut = bl * (-(-8192 // bl))
        assert np.abs(x[cut - 4000:cut]).max() > 0.01
        assert not np.array_equal(NR.process(x[cut:cut + 4000], k)[0], pt[cut:cut + 4000])


def test_a_set_time_restarts_from_silence(gpu_api):
    bl = 256
    p = RP.base_project("noise", bl=bl)
    RP.add_reverb(p, "r", "bus", *HALL)
    half = (p.cs // 2) * bl
    k = consts(gpu_api, SR, HALL)
    for form in (0, 1):
        got = []
        for out in ("r", "bus"):
            sb, fb, g = p.build(gpu_api)
            g.set_option("debug.reverb_form", form)
            assert g.set_output(out)
            for _ in range(8):   # (2 048 frames: every line has wrapped)
                g.render(sb, fb)
                fb.set_time_to_next_block()
            fb.set_time(half)
            g.set_time(half)
            blocks = []
            for _ in range(12):
                blocks.append(np.stack(g.render(sb, fb), axis=1))
                fb.set_time_to_next_block()
            got.append(np.concatenate(blocks))
        assert np.abs(got[1]).max() > 0.01
        pt, _ = NR.process(got[1], k)
        if form == 0:
            assert_same_bits(got[0], lerp1(got[1], pt), "pulls after set_time")
        else:
            assert_close(got[0], got[1], pt, "pulls after set_time, form 1")
        # ... and nothing of what the first pulls left is read: continuing from a state that sounds gives other values
        st = NR.new_state(k)
        for ln in st["lines"]:
            ln[:] = 0.01
        st["total"] = 8 * bl
        assert not np.array_equal(NR.process(got[1], k, state=st)[0], pt)


@pytest.mark.parametrize("wet,gain,angle", TG.MIX)
def test_wet_pan_and_gain(gpu_api, wet, gain, angle):
    p = RP.base_project("drums")
    RP.add_reverb(p, "r", "bus", *HALL, wet=wet, gain=gain, angle=angle)
    RP.add_reverb(p, "r1", "bus", *SMALL, wet=wet, gain=gain, angle=angle)
    built = build(gpu_api, p)
    x = render_f32(gpu_api, built, "bus", p.cs)
    for name, c in (("r", HALL), ("r1", SMALL)):
        k = consts(gpu_api, SR, c)
        y = render_f32(gpu_api, built, name, p.cs)
        want, _ = NR.reverb(x, k, wet=wet, gain=gain, angle=angle)
        proc, _ = NR.reverb(x, k)
        lim = mix_bound(x, proc, gain, angle)
        err = np.abs(y.astype(np.float64) - want.astype(np.float64))
        print("%s wet %g gain %g angle %g: worst error / bound %.3g" % (name, wet, gain, angle, float(np.max(err / lim))))
        assert (err <= lim).all(), (float(np.max(err / lim)), np.argwhere(err > lim)[:4].tolist())
        assert np.abs(want - x).max() > 1e-3 * wet   # (the vertex does something, in proportion to the mix)


def test_dry_passes_the_input_through_as_a_sum_launch(gpu_api):
    p = RP.base_project("drums")
    RP.add_reverb(p, "dry", "bus", *HALL, wet=0.0)
    RP.add_reverb(p, "almost", "bus", *HALL, wet=0.00009)
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
    assert not any(n.startswith("k_reverb") for n in names) and "k_sum" in names, names
    assert g.device_bytes() == before   # (no state block either)


def test_pcm_is_within_one_word_of_the_twin(gpu_api):
    p = RP.base_project("drums")
    RP.add_reverb(p, "r", "bus", *HALL, wet=0.4)
    built = build(gpu_api, p)
    x = render_f32(gpu_api, built, "bus", p.cs)
    want, _ = NR.reverb(x, consts(gpu_api, SR, HALL), wet=0.4)
    sb, fb, g = built
    assert g.set_output("r")
    fb.set_time(0)
    g.set_time(0)
    pcm, f = g.render_all(sb, fb, p.cs, 16)
    assert np.abs(pcm).max() > 1000
    assert np.abs(pcm.astype(np.int64) - _quantise16(want)).max() <= 1


def test_a_non_finite_input_frame_makes_its_own_output_frame_non_finite_and_no_other(gpu_api):
    """An infinite and a NaN sample in a loop source come out non-finite at their own frames (the dry leg of the lerp) and nowhere
    else: they enter the lines as 0, so every other frame is the twin's render of the input with those two samples zeroed."""
    bl, cs = 1024, 12
    raw = W.noise_int16(9, 30011).astype(np.float32).reshape(-1).copy()   # interleaved 16-bit words as floats
    raw[2 * 5000] = np.inf
    raw[2 * (7 * 1024 - 10) + 1] = np.nan
    sb = gpu_api.SampleBank(48000)
    sb.add_decoded("a", raw, 2, 48000, 16, "")
    sb.add_decoded("b", W.noise_int16(10, 30011).astype(np.float32).reshape(-1).copy(), 2, 48000, 16, "")
    fb = gpu_api.FlowwBank(48000, bl)
    g = gpu_api.Graph(bl, 48000)
    g.add_sampleloop("l", 0.5, 0.0, sb.get_index("a"))
    g.add_sampleloop("m", 0.4, 0.0, sb.get_index("b"))
    g.add_sum("bus", 1.0, 0.0)
    g.add_reverb("r", 1.0, 0.0, 1.0, *SMALL)
    assert g.connect("l", "bus") and g.connect("m", "bus") and g.connect("bus", "r")
    built = (sb, fb, g)
    x = render_f32(gpu_api, built, "bus", cs)
    assert (~np.isfinite(x)).sum() == 2 and not np.isfinite(x[5000, 0]) and not np.isfinite(x[7158, 1])
    zeroed = np.where(np.isfinite(x), x, np.float32(0.0))
    k = consts(gpu_api, SR, SMALL)
    ref = lerp1(zeroed, NR.process(zeroed, k)[0])
    assert np.isfinite(ref).all()
    for form in (0, 1):
        g.set_option("debug.reverb_form", form)
        for what, y in (("whole", render_f32(gpu_api, built, "r", cs, max_chunk_frames=1 << 24)), ("chunks", render_f32(gpu_api, built, "r", cs, max_chunk_frames=bl))):
            bad = np.argwhere(~np.isfinite(y)).tolist()
            assert bad == [[5000, 0], [7158, 1]], (form, what, bad)
            ok = np.isfinite(y)
            if form == 0:
                assert np.array_equal(y[ok].view(np.uint32), ref[ok].view(np.uint32)), what
            else:
                assert np.abs(y[ok].astype(np.float64) - ref[ok]).max() <= 2.0 ** -22 * np.abs(ref).max(), what


def test_a_batch_of_vertices_with_different_windows_is_one_merged_launch(gpu_api):
    """Three projects whose reverbs sit on the same level with B = 64, 128 and 256: one k_reverb launch per render, each member
    bitwise its own render."""
    sizes = (0.5, 1.0, 2.0)
    assert [consts(gpu_api, SR, (0.7, 0.3, 1.0, s))["B"] for s in sizes] == [64, 128, 256]
    projects = []
    for i, s in enumerate(sizes):
        p = RP.base_project("noise", seed=i)
        RP.add_reverb(p, "r", "bus", 0.7, 0.3, 1.0, s, wet=[1.0, 0.6, 0.3][i])
        p.set_output("r")
        projects.append(p)
    cs = projects[0].cs
    own = []
    for p in projects:
        sb, fb, g = p.build(gpu_api)
        first = g.render_all(sb, fb, cs, 16, want_f32=False)[0]
        fb.set_time(0)
        own.append((first, g.render_all(sb, fb, cs, 16, want_f32=False)[0]))
    assert len({o[0].tobytes() for o in own}) == 3
    batch = gpu_api.Batch()
    for p in projects:
        batch.add(*p.build(gpu_api))
    batch.set_profiling(True)
    for rep in range(2):
        batch.rewind()
        assert batch.render_all(cs, 16) == cs * 1024
        for i in range(3):
            assert np.array_equal(batch.read_pcm(i, cs), own[i][rep]), (rep, i)
    kt = batch.kernel_times()
    assert reverb_names(kt) == REVERB and kt["k_reverb"][1] == 2 and kt["k_reverb_sum"][1] == 2, kt


def test_the_state_block_is_counted_and_goes_with_the_vertices(gpu_api):
    p = RP.base_project("drums")
    RP.add_reverb(p, "r", "bus", *LARGE)
    block = 8 * (16 + sum(NR.lengths(consts(gpu_api, SR, LARGE))))
    assert block > 400000
    sb, fb, g = p.build(gpu_api)
    assert g.set_output("bus")
    g.render_all(sb, fb, p.cs, 16)
    before = g.device_bytes()
    assert g.set_output("r")
    fb.set_time(0)
    g.set_time(0)
    g.render_all(sb, fb, p.cs, 16)
    assert g.device_bytes() - before >= block   # (the block; and perhaps more edge buffers)
    assert g.device_bytes() - before < block + 4 * 8 * (p.cs * p.bl + 4)
    with_block = g.device_bytes()
    gpu_api.lib().td_graph_reset(g.h)
    # (... and the event tables of the vertices that went, a few kilobytes)
    assert block <= with_block - g.device_bytes() < block + (1 << 20), (with_block, g.device_bytes(), before)


def _guard_project(bl=1024, seconds=0.5):
    return TG.gpu_guard_project("add_reverb", "r", HALL, False, wet=0.5, bl=bl, seconds=seconds, notes=TG.SHORT_NOTES)


def test_guard_keeps_the_scan_and_fast_sines_in_front_of_a_reverb(gpu_api):
    """A scanned band-pass chain plus fast sines in front of a reverb, in the front-end's defaults (band_mode 2, sine_mode 2):
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
            print("guard stats in front of a reverb (Hrev %.3g): %s" % (consts(gpu_api, SR, HALL)["Hrev"], st))
            assert st["audits"] >= 1 and st["last_est"] > 0.0, st
    rms = float(np.sqrt(np.mean((outs["guard"].astype(np.float64) - outs["exact"].astype(np.float64)) ** 2)))
    print("guarded scan + fast sines in front of a reverb (wet 0.5): rms %.3g against the exact forms" % rms)
    assert rms <= 1e-6 and np.abs(outs["exact"]).max() > 0.05
    assert "k_band_scan" in names["guard"] and "k_sine_probe" in names["guard"], names["guard"]
    assert "k_band_scan" not in names["exact"] and "k_sine_probe" not in names["exact"], names["exact"]
    for m in names:
        assert [n for n in names[m] if n.startswith("k_reverb")] == REVERB, names[m]


def test_a_guarded_pull_forced_to_run_again_has_the_exact_bytes(gpu_api):
    """Block pulls under the guard with a bound of 0 (every audited render is done again, with the exact kernels): the state block
    each pull entered with is put back in front of the second run, and the frame count with it, so the pulled frames are the exact
    modes' to the bit."""
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


def test_kernel_names_with_and_without_a_reverb(gpu_api):
    for p in (W.drum_project(seconds=0.25), W.config2(seconds=0.25, n_src=8)):
        sb, fb, g = p.build(gpu_api)
        g.set_profiling(1)
        g.render_all(sb, fb, p.cs, 16, want_f32=False)
        names = list(g.kernel_times())
        assert names and not any(n.startswith("k_reverb") for n in names), names
    p = RP.base_project("drums")
    RP.add_reverb(p, "r", "bus", *HALL)
    p.set_output("r")
    sb, fb, g = p.build(gpu_api)
    g.set_profiling(1)
    g.render_all(sb, fb, p.cs, 16, want_f32=False)
    kt = g.kernel_times()
    assert reverb_names(kt) == REVERB and all(kt[n][1] == 1 for n in REVERB), kt
