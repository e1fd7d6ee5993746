"""The four effect vertices that carry a block of device memory from chunk to chunk (tde::Vertex::line) in ONE graph: a drum bus
into a saturator (R = 4), a chorus (20 ms +- 4 ms), a reverb (size 0.5) and a delay of 1 024 frames in series, 0.25 s at 48 kHz,
every one at gain 1, angle 0, wet 1.  The per-kind suites render one kind at a time; here the engine keeps, restarts, backs up and
puts back four blocks of four sizes at once.

The shapes are the smallest that cover both launch forms: the whole render is longer than 4 096 frames (k_sat_sum, k_chorus_sum
first), the chunks and the block pulls are not (one launch), and every line is shorter than the render, so it is read back.  The
delay's D = 1 024 makes ceil(frames / D) <= 16 in every form: one k_delay_apply tile, which has the serial recurrence's bits --
k_delay_local must not appear.  Every comparison is bitwise."""
import os
import sys

import numpy as np
import pytest

from termdaw_amd import workloads as W

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import chorus_projects as CP  # noqa: E402
import eq_projects as EP  # noqa: E402
import np_chorus as NC  # noqa: E402
import np_delay as ND  # noqa: E402
import np_reverb as NR  # noqa: E402
import np_saturator as NS  # noqa: E402
import fx_rig as TG  # noqa: E402

pytestmark = pytest.mark.gpu
SR = 48000
BL = 256
SAT = ("soft", 12.0, 0.2, -3.0, 4)                        # (kind, drive_db, bias, out_db, R)
CHORUS = CP.case(3, (20.0, 4.0, 0.8, 0.25), "sine")     # H = 1 216
REVERB = (0.5, 0.5, 0.5, 0.5)                             # (room, damp, width, size): shortest line 122, B = 64
DELAY = (1024.0 / 48.0, 0.7, 0.35)                        # (time_ms, feedback, cross): D = 1 024
CHAIN = ("sat", "cho", "rev", "dly")
build, render_f32, _pull_all = TG.build, TG.render_f32, TG._pull_all


def add_chain(p, src):
    p.add_saturator("sat", 1.0, 0.0, 1.0, *SAT)
    p.add_chorus("cho", 1.0, 0.0, 1.0, *CHORUS)
    p.add_reverb("rev", 1.0, 0.0, 1.0, *REVERB)
    p.add_delay("dly", 1.0, 0.0, 1.0, *DELAY)
    for a, b in zip((src,) + CHAIN, CHAIN):
        p.connect(a, b)
    p.set_output("dly")


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def profiled(g, render):
    """render() with profiling on: its frames and the names of the launches it took."""
    g.set_profiling(1)
    y = render()
    names = list(g.kernel_times())
    g.set_profiling(0)
    return y, names


@pytest.fixture(scope="module")
def chain(gpu_api):
    """The built project, and its first whole render of the output at the defaults: every block is allocated by it, none is read."""
    p = EP.base_project("drums", bl=BL, seconds=0.25)
    add_chain(p, "bus")
    built = build(gpu_api, p)
    n = p.cs * BL
    assert 4096 < n <= 16 * 1024 and gpu_api.delay_params(SR, *DELAY)[0] == 1024
    whole, names = profiled(built[2], lambda: render_f32(gpu_api, built, "dly", p.cs, max_chunk_frames=1 << 24))
    assert np.abs(whole).max() > 0.05
    for n_ in ("k_sat_sum", "k_sat", "k_chorus_sum", "k_chorus", "k_reverb_sum", "k_reverb", "k_delay_apply"):
        assert n_ in names, names
    assert "k_delay_local" not in names, names
    return p, built, whole


def test_the_chain_has_the_bits_of_the_numpy_twins_in_series(gpu_api, chain):
    p, built, _ = chain
    x = render_f32(gpu_api, built, "bus", p.cs, max_chunk_frames=1 << 24)
    assert np.abs(x).max() > 0.05
    y, names = profiled(built[2], lambda: render_f32(gpu_api, built, "dly", p.cs, **{"debug.reverb_form": 0}))
    built[2].set_option("debug.reverb_form", 1)
    assert "k_delay_local" not in names and "k_delay_apply" in names, names
    kind, drive, bias, out_db, R = SAT
    k = gpu_api.saturator_params(kind, R, drive, bias, out_db)
    s, _ = NS.saturator(x, kind, R, drive, bias, out_db, 1.0, 1.0, 0.0, h=gpu_api.saturator_taps(R), consts=k[:3])   # (64 frames late)
    c, _ = NC.chorus(s, SR, *CHORUS, consts=gpu_api.chorus_params(SR, *CHORUS)[:4])
    r = c + np.float32(1.0) * (NR.process(c, gpu_api.reverb_params(SR, *REVERB))[0] - c)      # the lerp at wet = 1, f32
    D, gs, gc, _ = gpu_api.delay_params(SR, *DELAY)
    want = r + np.float32(1.0) * (ND.delay(r, D, gs, gc, processed=True)[0] - r)
    assert np.isfinite(want).all() and np.abs(want.astype(np.float64) - x).max() > 1e-2
    bad = np.argwhere(y.view(np.uint32) != want.view(np.uint32))
    assert not len(bad), (len(bad), bad[:4].tolist(), [(float(y[i, j]), float(want[i, j])) for i, j in bad[:4]])


def test_whole_chunked_and_pulled_renders_agree_at_every_vertex_of_the_chain(gpu_api, chain):
    p, built, first = chain
    g = built[2]
    for out in CHAIN:
        whole = render_f32(gpu_api, built, out, p.cs, max_chunk_frames=1 << 24)
        chunks, c_names = profiled(g, lambda: render_f32(gpu_api, built, out, p.cs, max_chunk_frames=4096))
        g.set_option("max_chunk_frames", 1 << 24)
        pulls, p_names = profiled(g, lambda: _pull_all(gpu_api, built, out, p.cs))
        assert same_bits(chunks, whole), (out, "chunks", np.argwhere(chunks != whole)[:4].tolist())
        assert same_bits(pulls, whole), (out, "pulls", np.argwhere(pulls != whole)[:4].tolist())
        for names in (c_names, p_names):   # (one launch per kind, and the delay a single tile)
            assert not {"k_sat_sum", "k_chorus_sum", "k_delay_local"} & set(names), (out, names)
        if out == "dly":
            assert same_bits(whole, first)
            assert "k_sat" in p_names and "k_chorus" in p_names and "k_reverb" in p_names and "k_delay_apply" in p_names, p_names


def test_a_set_time_behind_the_pulls_restarts_all_four_blocks(gpu_api, chain):
    """Behind the pulls every block holds the end of the timeline: a set_time(0) restarts all four at once, and no stale word is
    read -- the whole render is the one that allocated them."""
    p, built, first = chain
    sb, fb, g = built
    g.set_option("max_chunk_frames", 1 << 24)
    pulls = _pull_all(gpu_api, built, "dly", p.cs)
    assert same_bits(pulls, first)
    fb.set_time(0)
    g.set_time(0)
    again = g.render_all(sb, fb, p.cs, 16, want_pcm=False)[1]
    assert same_bits(again, first), np.argwhere(again != first)[:4].tolist()


def test_a_guarded_pull_forced_to_run_again_puts_all_four_lines_back(gpu_api):
    """A two-stage band-pass chain and a synth in front of the bus (the per-kind suites' _guard_project), block pulls under the guard
    with a bound of 0: every audited pull is done again with the exact kernels, from the four blocks it entered with."""
    p = W.ProjectScript(SR, 1024)
    p.set_length(0.25)
    p.assets["a"] = W.Asset(W.noise_int16(7, 9000))
    p.load_sample("a", "a", "")
    p.event_files["f"] = np.array([(0.01, 60.0, 0.8), (0.1, 60.0, 0.0), (0.12, 64.0, 0.6), (0.22, 64.0, 0.0)], np.float32)
    p.load_midi_floww("f", "f")
    p.add_sampleloop("s", 0.5, 0.0, "a")
    p.add_bandpass("b1", 1.0, 0.0, 1.0, 300.0, 5000.0, True)
    p.add_bandpass("b2", 1.0, 10.0, 1.0, 200.0, 8000.0, True)
    p.add_synth("y", 0.5, 0.0, "f", 0.4, 0.3, W.HIT_ADSR, 1.0, 0.8, W.NOTE_ADSR, 0.5, W.STD_ADSR)
    p.add_sum("bus", 1.0, 0.0)
    p.connect("s", "b1"); p.connect("b1", "b2"); p.connect("b2", "bus"); p.connect("y", "bus")
    add_chain(p, "bus")
    got = {}
    for mode, (bm, sm, ppb) in (("redo", (2, 2, 0)), ("exact", (0, 1, 200))):
        sb, fb, g = p.build(gpu_api)
        g.set_option("band_mode", bm)
        g.set_option("sine_mode", sm)
        g.set_option("band_guard_ppb", ppb)
        g.set_profiling(1)
        blocks = []
        for _ in range(p.cs):
            l, r = g.render(sb, fb)
            fb.set_time_to_next_block()
            blocks.append(np.stack([l, r], axis=1))
        got[mode] = np.concatenate(blocks)
        names = list(g.kernel_times())
        assert "k_delay_apply" in names and "k_delay_local" not in names, names
        if mode == "redo":
            st = g.band_guard_stats()
            assert st["redos"] >= p.cs - 1, st
    assert np.abs(got["exact"]).max() > 0.05
    assert same_bits(got["redo"], got["exact"]), np.argwhere(got["redo"] != got["exact"])[:4].tolist()
