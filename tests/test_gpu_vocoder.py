"""The vocoder vertex on the device (td_graph_add_vocoder) against its float64 twin (tests/np_vocoder.py, the serial
restatement of the definition in include/termdaw_amd.h), run on the engine's own constants (td_vocoder_params).

The carrier and the key of the vertex under test always come from the engine itself: renders of the same graph with set_output
on the vertices in front, read as f32 -- the oracle-verified part of the graph is not restated here.

Bounds.  wet = 1, gain = 1, angle = 0, per value:  |p' - p| <= 2^-23 |p| + E max|p| on the bank's output p, carried through the
definition's f32 lerp to the vertex' output (fx_rig.assert_close says why it is not asserted on the output as it stands).
The first term is the one f32 rounding of p, which may flip; E covers the float64 re-association of the scans: 8 x what the numpy
emulation of the tiled scans shows over this file's own grid and inputs (tests/vocoder_projects.py E, derived and re-checked on
the CPU by tests/test_vocoder_host.py; far under the cap 2^-28).  With wet in (0, 1), pan and gain: 4 x 2^-23 x max(|dry|, |p|) x
|amplitude| absolute, as for the EQ.  PCM cases: within one word of the twin's quantised value.

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
import np_vocoder as NV  # noqa: E402
import vocoder_projects as VP  # noqa: E402
from fx_rig import assert_close, MIX, mix_bound, _pull_all, _quantise16, REL, render_f32  # noqa: E402

pytestmark = pytest.mark.gpu
VOC_LAUNCHES = ["k_voc_local", "k_voc_carry_z", "k_voc_env", "k_voc_carry_env", "k_voc_apply"]
CASE = (8, 200.0, 4000.0, 4.0, 10.0, 12.0)   # bands, lo, hi, q, response_ms, out_db
CASE16 = (16, 60.0, 12000.0, 8.0, 3.0, 18.0)
CASE4 = (4, 300.0, 3000.0, 2.0, 30.0, 6.0)


def _bits(a):
    return a.view(np.uint32)


def build(api, p, warm=("bus", "kbus")):
    """The built project after one discarded render of each vertex in front: the sample_multi vertices keep voices that are still
    sounding when a render ends, so only from the second render on does every render see the same input."""
    built = p.build(api)
    for v in warm:
        render_f32(api, built, v, p.cs)
    return built


def twin(api, sr, case, x, k, state=None):
    """(p float32, end state) of the serial twin on the engine's constants."""
    v, end = NV.serial(x, k, VP.spec(api, sr, case), state)
    return v.astype(np.float32), end


def close(y, x, p, what):
    return assert_close(y, x, p, what, VP.E)


# ---- the grid ----
@pytest.mark.parametrize("sr", VP.RATES)
@pytest.mark.parametrize("pair", VP.PAIRS, ids=lambda pr: "%s-keyed-by-%s" % pr)
def test_grid_matches_the_twin(gpu_api, sr, pair):
    cases = VP.grid_cases(sr)
    assert len(cases) == 81
    p = VP.base_project(*pair, sr=sr)
    for i, c in enumerate(cases):
        VP.add_vocoder(p, "v%d" % i, "bus", "kbus", c)
    built = build(gpu_api, p)
    x, k = render_f32(gpu_api, built, "bus", p.cs), render_f32(gpu_api, built, "kbus", p.cs)
    assert min(np.abs(x).max(), np.abs(k).max()) > 0.05 and p.cs * p.bl > 5 * NV.TILE
    worst, exact, acts = 0.0, 0, 0
    for B in VP.BANDS:
        idx = [i for i, c in enumerate(cases) if c[0] == B]
        vs, _ = NV.serial(x, k, [VP.spec(gpu_api, sr, cases[i]) for i in idx])   # (the cases of one band count side by side)
        for i, v in zip(idx, vs):
            pw = v.astype(np.float32)
            y = render_f32(gpu_api, built, "v%d" % i, p.cs)
            worst = max(worst, close(y, x, pw, "%s %d %s" % (pair, sr, cases[i])))
            want = x + np.float32(1.0) * (pw - x)
            exact += int(np.array_equal(_bits(y), _bits(want)))
            acts += int(np.abs(pw).max() > 1e-5 and np.abs(want.astype(np.float64) - x).max() > 64.0 * (REL + VP.E) * np.abs(x).max())
    print("grid %s %d: %d cases, worst |y - want| %.3g x the plain bound, %d bit-identical to the twin" % (pair, sr, len(cases), worst, exact))
    assert acts == len(cases), acts
    assert np.array_equal(render_f32(gpu_api, built, "bus", p.cs), x) and np.array_equal(render_f32(gpu_api, built, "kbus", p.cs), k)


# ---- self key, silent key, a tone as key ----
def _forms(api, built, out, cs):
    forms = {"whole": render_f32(api, built, out, cs), "chunks": render_f32(api, built, out, cs, max_chunk_frames=4096)}
    built[2].set_option("max_chunk_frames", 1 << 24)
    forms["pulls"] = _pull_all(api, built, out, cs)
    return forms


@pytest.mark.parametrize("bl", [1024, 64])
def test_self_key_is_the_unkeyed_vertex_bitwise(gpu_api, bl):
    """A vocoder keyed by its own source sums the same terms twice into the same bits: whole (the five launches, k_voc_local's
    keyed form), in chunks and by pulls (the one-launch form, keyed)."""
    p = VP.base_project("drums", "noise", bl=bl)
    VP.add_vocoder(p, "plain", "bus", None, CASE16, wet=0.8, gain=1.3, angle=20.0)
    VP.add_vocoder(p, "self", "bus", "bus", CASE16, wet=0.8, gain=1.3, angle=20.0)
    built = build(gpu_api, p)
    a, b = _forms(gpu_api, built, "plain", p.cs), _forms(gpu_api, built, "self", p.cs)
    x = render_f32(gpu_api, built, "bus", p.cs)
    for form in a:
        assert np.array_equal(_bits(a[form]), _bits(b[form])), form
        assert np.abs(a[form] - x).max() > 1e-3
    g = built[2]
    g.set_profiling(1)
    render_f32(gpu_api, built, "self", p.cs)
    assert [n for n in g.kernel_times() if n.startswith("k_voc")] == VOC_LAUNCHES


def test_a_silent_key_gives_the_dry_lerp_of_zero_exactly(gpu_api):
    p = VP.base_project("drums", "noise")
    p.add_sum("mute", 0.0, 0.0)   # kbus at gain 0: zeros
    p.connect("kbus", "mute")
    p.add_sum("mute2", 1.0, 0.0)  # (a two-input Sum behind it: an edge buffer, not a stage read through)
    p.connect("mute", "mute2"); p.connect("mute", "mute2")
    VP.add_vocoder(p, "v", "bus", "mute2", CASE, wet=0.25)
    built = build(gpu_api, p)
    x = render_f32(gpu_api, built, "bus", p.cs)
    assert not render_f32(gpu_api, built, "mute2", p.cs).any()
    for form, y in _forms(gpu_api, built, "v", p.cs).items():
        assert np.array_equal(_bits(y), _bits(x + np.float32(0.25) * (np.float32(0.0) - x))), form


def test_a_tone_as_key_opens_its_own_band(gpu_api):
    """Non-vacuity: white noise as carrier, a sine at band k's centre as key -- of the rendered output's energy per band (measured
    here from its spectrum, between the geometric means of neighbouring centres) band k's is the largest."""
    sr, kb = 48000, 5
    rows, _, _ = gpu_api.vocoder_params(sr, *CASE16)
    f = [r[0] for r in rows]
    p = W.ProjectScript(sr, 1024)
    p.set_length(0.5)
    p.set_render_samplerate(sr)
    hz = round(f[kb])
    p.assets["n"] = W.Asset(W.noise_int16(3, 20011), sr=sr)
    tone = (12000.0 * np.sin(2.0 * np.pi * hz * np.arange(sr) / sr)).astype(np.int16)   # whole cycles in a second: loops cleanly
    p.assets["t"] = W.Asset(np.stack([tone, tone], axis=1), sr=sr)
    p.load_sample("n", "n", "")
    p.load_sample("t", "t", "")
    p.add_sampleloop("n", 0.5, 0.0, "n")
    p.add_sampleloop("t", 1.0, 0.0, "t")
    p.add_sum("bus", 1.0, 0.0); p.connect("n", "bus"); p.connect("n", "bus")
    p.add_sum("kbus", 1.0, 0.0); p.connect("t", "kbus"); p.connect("t", "kbus")
    VP.add_vocoder(p, "v", "bus", "kbus", CASE16)
    p.set_output("v")
    built = build(gpu_api, p)
    y = render_f32(gpu_api, built, "v", p.cs)[8192:, 0].astype(np.float64)   # (past the follower's rise)
    spec = np.abs(np.fft.rfft(y * np.hanning(len(y)))) ** 2
    fr = np.fft.rfftfreq(len(y), 1.0 / sr)
    edges = [f[0] / np.sqrt(f[1] / f[0])] + [np.sqrt(f[b] * f[b + 1]) for b in range(15)] + [f[15] * np.sqrt(f[15] / f[14])]
    e = np.array([spec[(fr >= edges[b]) & (fr < edges[b + 1])].sum() for b in range(16)])
    print("band energies, relative to band %d: %s" % (kb, np.round(e / e[kb], 4).tolist()))
    assert e.argmax() == kb and (np.delete(e, kb) < e[kb]).all()


# ---- chunks, pulls, restarts ----
@pytest.mark.parametrize("bl", [1024, 64, 2817])
def test_chunked_and_pulled_renders_match_the_twin(gpu_api, bl):
    """0.5 s: whole, in 4 096-frame chunks (bl 2 817: one block each, a partial second tile every time), and by block pulls of
    `bl` frames -- each inside the bound, and each restarted render bitwise the first."""
    p = VP.base_project("noise", "drums", bl=bl)
    VP.add_vocoder(p, "v", "bus", "kbus", CASE16)
    built = build(gpu_api, p)
    n = p.cs * bl
    assert n == {1024: 24576, 64: 24000, 2817: 25353}[bl]   # (12 tiles; 11 tiles and 1 472 frames; 12 tiles and 777 frames)
    x, k = render_f32(gpu_api, built, "bus", p.cs), render_f32(gpu_api, built, "kbus", p.cs)
    pw, end = twin(gpu_api, 48000, CASE16, x, k)
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
    restart = twin(gpu_api, 48000, CASE16, x[4096:8192], k[4096:8192])[0]
    assert np.abs(restart.astype(np.float64) - pw[4096:8192]).max() > 1e-4 * np.abs(pw).max()
    # a set_time in the middle of pulling restarts the state: two pulls, a jump, one pull -- the twin started from zero there
    at = (4000 // bl) * bl
    got = []
    for out in ("v", "bus", "kbus"):
        sb, fb, g = p.build(gpu_api)
        assert g.set_output(out)
        for _ in range(2):
            g.render(sb, fb)
            fb.set_time_to_next_block()
        fb.set_time(at)
        g.set_time(at)
        got.append(np.stack(g.render(sb, fb), axis=1))
    assert np.abs(got[1]).max() > 0.01
    close(got[0], got[1], twin(gpu_api, 48000, CASE16, got[1], got[2])[0], "pull after set_time")


def test_more_than_256_tiles(gpu_api):
    """12 s at 48 kHz of the looped noise keyed by the drums, 16 bands: 576 512 frames, 282 tiles -- both carries fold two tiles
    per lane."""
    p = VP.base_project("noise", "drums", seconds=12.0)
    VP.add_vocoder(p, "v", "bus", "kbus", CASE16)
    built = build(gpu_api, p)
    n = p.cs * p.bl
    assert n == 576512 and (n + NV.TILE - 1) // NV.TILE == 282
    x, k = render_f32(gpu_api, built, "bus", p.cs), render_f32(gpu_api, built, "kbus", p.cs)
    close(render_f32(gpu_api, built, "v", p.cs), x, twin(gpu_api, 48000, CASE16, x, k)[0], "282 tiles")


# ---- the mix ----
@pytest.mark.parametrize("wet,gain,angle", MIX + [(1.0, 1.7, -75.0)])
def test_wet_pan_and_gain(gpu_api, wet, gain, angle):
    p = VP.base_project("drums", "noise")
    VP.add_vocoder(p, "v", "bus", "kbus", CASE, wet=wet, gain=gain, angle=angle)
    built = build(gpu_api, p)
    x, k = render_f32(gpu_api, built, "bus", p.cs), render_f32(gpu_api, built, "kbus", p.cs)
    y = render_f32(gpu_api, built, "v", p.cs)
    sp = VP.spec(gpu_api, 48000, CASE)
    want, _ = NV.process(x, k, sp, wet=wet, gain=gain, angle=angle)
    proc = NV.serial(x, k, sp)[0].astype(np.float32)
    lim = mix_bound(x, proc, gain, angle)
    err = np.abs(y.astype(np.float64) - want.astype(np.float64))
    print("wet %g gain %g angle %g: worst error / bound %.3g" % (wet, gain, angle, float(np.max(err / lim))))
    assert (err <= lim).all(), (float(np.max(err / lim)), np.argwhere(err > lim)[:4].tolist())
    assert np.abs(want - x).max() > 1e-3 * wet   # (the vertex does something, in proportion to the mix)


def test_dry_ignores_its_key_and_is_a_sum_launch(gpu_api):
    p = VP.base_project("drums", "noise")
    VP.add_vocoder(p, "dry", "bus", "kbus", CASE, wet=0.0)
    VP.add_vocoder(p, "almost", "bus", "kbus", CASE, wet=0.00009)
    VP.add_vocoder(p, "wet", "bus", "kbus", CASE)
    built = build(gpu_api, p)
    x = render_f32(gpu_api, built, "bus", p.cs)
    for name in ("dry", "almost"):
        y = render_f32(gpu_api, built, name, p.cs)
        assert np.array_equal(y, x), (name, np.argwhere(y != x)[:4].tolist())
    g = built[2]
    g.set_profiling(1)
    render_f32(gpu_api, built, "dry", p.cs)
    names = list(g.kernel_times())
    assert not any(n.startswith("k_voc") for n in names) and "k_sum" in names, names   # wet < 0.0001: a plain sum launch
    render_f32(gpu_api, built, "wet", p.cs)
    assert [n for n in g.kernel_times() if n.startswith("k_voc")] == VOC_LAUNCHES
    # a chunk of one tile is k_voc_apply alone
    q = VP.base_project("drums", "noise", seconds=0.04)
    VP.add_vocoder(q, "v", "bus", "kbus", CASE)
    assert q.cs * q.bl == NV.TILE
    sb, fb, g = q.build(gpu_api)
    g.set_output("v")
    g.set_profiling(1)
    g.render_all(sb, fb, q.cs, 16, want_f32=False)
    assert [n for n in g.kernel_times() if n.startswith("k_voc")] == ["k_voc_apply"]


def test_projects_without_a_vocoder_launch_no_vocoder_kernel(gpu_api):
    fx_rig.projects_without_the_kind_launch_no_kernel_of_it(gpu_api, "k_voc")


# ---- key sources ----
def _xk(api, built, p, src, keys):
    x = render_f32(api, built, src, p.cs)
    k = np.float32(0.0) + render_f32(api, built, keys[0], p.cs)   # sum_inputs (extensions.rs:310-319), f32, in connect_key() order
    for name in keys[1:]:
        k = k + render_f32(api, built, name, p.cs)
    return x, k


def test_key_source_an_adsr_vertex_that_would_be_read_through(gpu_api):
    """`env` has one input and one input consumer, the two-input Sum `mix`: without the key edge `mix` evaluates it itself and its
    frames never exist."""
    p = VP.base_project("noise", "drums")
    p.event_files["f"] = np.array([(0.01, 60.0, 0.9), (0.12, 60.0, 0.0), (0.2, 62.0, 0.7), (0.4, 62.0, 0.0)], np.float32)
    p.load_midi_floww("f", "f")
    p.add_adsr("env", 1.0, 0.0, 1.0, "f", False, True, -1, [0.01, 0.1, 0.8, 0.1, 0.2, 0.01])
    p.connect("kbus", "env")
    p.add_sum("mix", 1.0, 0.0); p.connect("env", "mix"); p.connect("bus", "mix")
    VP.add_vocoder(p, "v", "mix", "env", CASE)
    built = build(gpu_api, p)
    x, k = _xk(gpu_api, built, p, "mix", ["env"])
    assert np.abs(k).max() > 0.05
    close(render_f32(gpu_api, built, "v", p.cs), x, twin(gpu_api, 48000, CASE, x, k)[0], "adsr key")


def test_key_sources_another_effects_output_twice_and_a_stage(gpu_api):
    """Two key edges from an EQ's output (summed twice) and one from a single-input Sum stage, read through (term kind 4)."""
    p = VP.base_project("noise", "drums")
    p.add_eq("e", 1.0, 0.0, 1.0, "peak", 900.0, 2.5, 9.0); p.connect("kbus", "e")
    p.add_sum("stage", 0.5, -45.0); p.connect("kbus", "stage")
    p.add_vocoder("v", 1.0, 0.0, 1.0, *CASE4)
    p.connect("bus", "v")
    for key in ("e", "stage", "e"):
        p.connect_key(key, "v")
    built = build(gpu_api, p)
    x, k = _xk(gpu_api, built, p, "bus", ["e", "stage", "e"])
    for form, y in _forms(gpu_api, built, "v", p.cs).items():
        close(y, x, twin(gpu_api, 48000, CASE4, x, k)[0], "eq + stage + eq as key, %s" % form)


def test_key_source_inside_a_band_pass_chain_and_stems(gpu_api):
    """band_mode 1: kbus -> b1 -> b2 -> b3 would be ONE chain launch and b2's frames would never exist; the key edge makes the
    chain materialise b2.  The output sits behind both the vocoder and b3; the vocoder and its key source are read as stems."""
    p = VP.base_project("noise", "drums")
    for i, (lo, hi) in enumerate(((100.0, 9000.0), (150.0, 8000.0), (200.0, 7000.0))):
        p.add_bandpass("b%d" % (i + 1), 1.0, 0.0, 1.0, lo, hi, True)
        p.connect("kbus" if i == 0 else "b%d" % i, "b%d" % (i + 1))
    VP.add_vocoder(p, "v", "bus", "b2", CASE)
    p.add_sum("mix", 1.0, 0.0); p.connect("v", "mix"); p.connect("b3", "mix")
    built = build(gpu_api, p)
    sb, fb, g = built
    g.set_option("band_mode", 1)
    x, k = _xk(gpu_api, built, p, "bus", ["b2"])
    assert np.abs(k).max() > 0.05
    pw = twin(gpu_api, 48000, CASE, x, k)[0]
    want = x + np.float32(1.0) * (pw - x)
    g.set_output("mix")
    g.set_stems(["v", "b2"])
    fb.set_time(0)
    g.set_time(0)
    g.set_profiling(1)
    g.render_all(sb, fb, p.cs, 16)
    assert "k_band_scan" in list(g.kernel_times())
    assert np.abs(g.read_stem_pcm(0).astype(np.int64) - _quantise16(want)).max() <= 1
    assert np.abs(g.read_stem_pcm(1).astype(np.int64) - _quantise16(k)).max() <= 1
    assert np.abs(_quantise16(want) - _quantise16(x)).max() > 30
    g.set_stems([])


# ---- the guard modes ----
def _guard_project(where):
    p = W.ProjectScript(48000, 1024)
    p.set_length(1.0)
    p.assets["a"] = W.Asset(W.noise_int16(7, 9000))
    p.assets["a2"] = W.Asset(W.noise_int16(8, 9001))
    p.load_sample("a", "a", "")
    p.load_sample("a2", "a2", "")
    p.event_files["f"] = np.array([(0.01, 60.0, 0.8), (0.4, 60.0, 0.0), (0.5, 64.0, 0.6), (0.9, 64.0, 0.0)], np.float32)
    p.load_midi_floww("f", "f")
    p.add_sampleloop("s", 0.5, 0.0, "a")
    p.add_sampleloop("s2", 0.5, 0.0, "a2")
    p.add_bandpass("b1", 1.0, 0.0, 1.0, 300.0, 5000.0, True)
    p.add_bandpass("b2", 1.0, 10.0, 1.0, 200.0, 8000.0, True)
    p.add_synth("y", 0.5, 0.0, "f", 0.4, 0.3, W.HIT_ADSR, 1.0, 0.8, W.NOTE_ADSR, 0.5, W.STD_ADSR)
    p.add_sum("bus", 1.0, 0.0)
    p.add_vocoder("v", 1.0, 0.0, 1.0, *CASE)
    if where == "downstream":   # loop -> vocoder (keyed by a loop) -> band-pass chain; the synth joins behind the vocoder
        p.connect("s", "v"); p.connect_key("s2", "v"); p.connect("v", "b1"); p.connect("b1", "b2"); p.connect("b2", "bus"); p.connect("y", "bus")
        p.set_output("bus")
    elif where == "input":      # band-pass chain and synth -> bus -> vocoder, keyed by a loop
        p.connect("s", "b1"); p.connect("b1", "b2"); p.connect("b2", "bus"); p.connect("y", "bus"); p.connect("bus", "v"); p.connect_key("s2", "v")
        p.set_output("v")
    else:                       # loop -> vocoder, keyed by band-pass chain and synth -> bus
        p.connect("s", "b1"); p.connect("b1", "b2"); p.connect("b2", "bus"); p.connect("y", "bus"); p.connect("s2", "v"); p.connect_key("bus", "v")
        p.set_output("v")
    return p


def test_guard_keeps_the_scan_and_fast_sines_downstream_of_a_vocoder(gpu_api):
    fx_rig.guard_keeps_the_scan_and_fast_sines_downstream(gpu_api, _guard_project("downstream"), "vocoder", "k_voc", VOC_LAUNCHES)


@pytest.mark.parametrize("where", ["input", "key"])
def test_guard_renders_the_exact_forms_upstream_of_a_vocoder(gpu_api, where):
    fx_rig.guard_renders_the_exact_forms_upstream(gpu_api, _guard_project(where), floor=1e-3)


# ---- batches ----
def test_batch_members_are_bitwise_their_own_renders(gpu_api):
    """Eight projects, each with a keyed and an unkeyed vocoder in ONE level (and band counts that differ across the batch): the
    merged launches give every member the words of its own render."""
    projects = []
    cases = VP.grid_cases(48000)
    for i in range(8):
        p = VP.base_project(*VP.PAIRS[i % 3], seconds=1.0)
        VP.add_vocoder(p, "vk", "bus", "kbus", cases[(13 * i + 5) % len(cases)], wet=[1.0, 0.6][i % 2], gain=[1.0, 0.7][(i // 4) % 2])
        VP.add_vocoder(p, "vu", "bus", None, cases[(29 * i + 1) % len(cases)])
        p.add_sum("mix", 0.5, 0.0); p.connect("vk", "mix"); p.connect("vu", "mix")
        if i % 4 == 2:   # in front of a Normalize output
            p.add_normalize("out", 1.0, 0.0)
            p.connect("mix", "out")
            p.set_output("out")
        else:
            p.set_output("mix")
        projects.append(p)
    fx_rig.batch_matches_own_renders(gpu_api, projects)


# ---- the front end ----
def test_front_end_renders_the_vocoder_project(gpu_api, tmp_path):
    mem = fx_rig.front_end_renders(gpu_api, tmp_path, W.vocoder_project(seconds=1.0), 'add_vocoder("voc",', 'connect_key("drums","voc")')
    # ... and the key is really in the path: the chord sounds where the drums do -- dry, the same project is the plain chord
    fx_rig.front_end_words_differ(gpu_api, tmp_path, W.vocoder_project(seconds=1.0, wet=0.0), mem)


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
def test_random_vocoder_projects(gpu_api, seed):
    p = VP.random_vocoder_project(seed)
    p.sine_mode = 1   # (the reference's sine: every render of a vertex gives the same bits whatever the output is)
    out = p.output_vertex
    whole = _fresh(gpu_api, p, out)
    assert np.array_equal(_bits(whole), _bits(_fresh(gpu_api, p, out))), seed
    # the first vocoder that is not dry against the twin on the engine's own x and k, whole, in chunks and by pulls
    wets = [c for c in p.calls["add_vocoder"] if c[3] >= 0.0001]
    if not wets:
        return
    args = wets[0]
    v, gain, angle, wet, case = args[0], args[1], args[2], args[3], tuple(args[4:])
    ins = [a for a, b in p.calls["connect"] if b == v]
    built = p.build(gpu_api)
    g = built[2]
    keys = [a for a, b in p.calls["connect_key"] if b == v and g.connect_key(a, v)]   # (an edge that closes a loop is refused, here as in build())
    built = p.build(gpu_api)

    def total(names):
        s = np.zeros((p.cs * p.bl, 2), np.float32)
        for nm in names:
            s = s + _fresh(gpu_api, p, nm)
        return s
    x, k = total(ins), (total(keys) if keys else None)
    sp = VP.spec(gpu_api, 48000, case)
    want, _ = NV.process(x, k, sp, wet=wet, gain=gain, angle=angle)
    proc = NV.serial(x, k, sp)[0].astype(np.float32)
    with np.errstate(invalid="ignore"):
        lim = mix_bound(x, proc, gain, angle)
    for form in ("whole", "chunks", "pulls"):
        y = _fresh(gpu_api, p, v, form)
        err = np.abs(y.astype(np.float64) - want.astype(np.float64))
        print("seed %d: %s keyed by %s, %s: worst error / bound %.3g" % (seed, v, keys, form, float(np.nanmax(err / lim))))
        assert (err <= lim).all(), (seed, v, form, float(np.nanmax(err / lim)), np.argwhere(~(err <= lim))[:4].tolist())
