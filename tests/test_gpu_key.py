"""Key edges on the device (include/termdaw_amd.h td_graph_connect_key): a compressor or gate vertex that takes its
level from the sum of its key sources, against tests/np_key.py -- the two vertices' twins composed -- on the input x and the key k
the engine itself renders at the vertices in front.

The bounds are the two vertices' own and are not derived again: the gate's fx_rig.assert_close with gate_projects.E (the env
sequence of a gate keyed by `gated` is that of the unkeyed gate on `gated`, which E was derived on), the compressor's
fx_rig.assert_close_f32, fx_rig.mix_bound where wet, pan or gain are in play, one word for PCM.  Shapes: 0.5 s
(24 576 frames at 48 kHz, 12 tiles of 2 048), 4 096-frame chunks, block pulls of 1 024 and 64 frames."""
import os
import subprocess
import sys
import wave

import numpy as np
import pytest

from termdaw_amd import workloads as W

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gate_projects as GP  # noqa: E402
import key_projects as KP  # noqa: E402
import np_key as NK  # noqa: E402
from fx_rig import MIX, assert_close, assert_close_f32, build, mix_bound, _pull_all, _quantise16, render_f32, _write_project  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ("gate", "comp")


def _bits(a):
    return a.view(np.uint32)


def _add(p, kind, name, src, key, case=None, **kw):
    if kind == "gate":
        KP.add_gate(p, name, src, key, case or KP.GATE_CASE, **kw)
    else:
        KP.add_comp(p, name, src, key, case or KP.COMP_CASE, **kw)


def _twin(api, kind, sr, case, x, k, **kw):
    """The keyed twin's output (wet / gain / angle in kw) and the processed signal p."""
    if kind == "gate":
        c = api.gate_params(sr, *case)
        return NK.gate(x, k, c, **kw)[0], NK.gate(x, k, c, processed=True)[0]
    return NK.compressor(x, k, sr, *case, **kw)[0], NK.compressor(x, k, sr, *case, processed=True)[0]


def _close(api, kind, sr, case, y, x, k, what):
    """wet 1, no pan, no gain: the vertex' own bound."""
    want, p = _twin(api, kind, sr, case, x, k)
    if kind == "gate":
        assert_close(y, x, p, what, GP.E)
    else:
        assert_close_f32(y, want, what)
    return want


def _forms(api, built, out, cs):
    """Whole, in 4 096-frame chunks, by block pulls: each twice."""
    f = {"whole": [render_f32(api, built, out, cs) for _ in range(2)],
         "chunks": [render_f32(api, built, out, cs, max_chunk_frames=4096) for _ in range(2)]}
    built[2].set_option("max_chunk_frames", 1 << 24)
    f["pulls"] = [_pull_all(api, built, out, cs) for _ in range(2)]
    return f


# ---- 1. a vertex keyed by its own input is the unkeyed vertex ----
@pytest.mark.parametrize("bl", [1024, 64])
@pytest.mark.parametrize("kind", KINDS)
def test_self_key_is_the_unkeyed_vertex_bitwise(gpu_api, kind, bl):
    p = GP.base_project("gated", bl=bl)
    _add(p, kind, "plain", "bus", [])
    _add(p, kind, "keyed", "bus", "bus")
    built = build(gpu_api, p)
    x = render_f32(gpu_api, built, "bus", p.cs)
    plain, keyed = _forms(gpu_api, built, "plain", p.cs), _forms(gpu_api, built, "keyed", p.cs)
    for form in plain:
        for a, b in zip(plain[form], keyed[form]):
            assert np.array_equal(_bits(a), _bits(b)), (kind, bl, form)
        assert np.abs(plain[form][0] - x).max() > 1e-3   # (the vertex acts)


# ---- 2. ducking against the twin ----
def _ducking(api, kind, via, sr=48000, bl=1024, cases=None):
    p, key = KP.ducking_project(via, sr=sr, bl=bl)
    cases = cases or [KP.GATE_CASE if kind == "gate" else KP.COMP_CASE]
    for i, c in enumerate(cases):
        _add(p, kind, "v%d" % i, "bus", key, c)
    built = build(api, p)
    return p, built, render_f32(api, built, "bus", p.cs), render_f32(api, built, key, p.cs), cases


@pytest.mark.parametrize("via", KP.VIAS)
@pytest.mark.parametrize("kind", KINDS)
def test_ducking_grid_matches_the_twin(gpu_api, kind, via):
    p, built, x, k, cases = _ducking(gpu_api, kind, via, cases=KP.gate_grid() if kind == "gate" else KP.comp_grid())
    assert len(cases) == (12 if kind == "gate" else 6) and p.cs * p.bl == 24576
    assert np.abs(x).max() > 0.05 and np.abs(k).max() > 0.2 and not np.array_equal(x, k)
    for i, c in enumerate(cases):
        forms = _forms(gpu_api, built, "v%d" % i, p.cs)
        for name, (a, b) in forms.items():
            want = _close(gpu_api, kind, 48000, c, a, x, k, "%s %s %s %s" % (kind, via, c, name))
            assert np.array_equal(_bits(a), _bits(b)), (name, c)   # a restarted render is bitwise the first
        # ... and the key is what decides: the unkeyed twin on x is somewhere else
        unkeyed = _twin(gpu_api, kind, 48000, c, x, x)[0]
        assert np.abs(unkeyed.astype(np.float64) - want).max() > 1e-3, c


@pytest.mark.parametrize("sr", [44100, 96000])
@pytest.mark.parametrize("via", KP.VIAS)
@pytest.mark.parametrize("kind", KINDS)
def test_ducking_base_case_at_other_rates(gpu_api, kind, via, sr):
    p, built, x, k, cases = _ducking(gpu_api, kind, via, sr=sr)
    for name, (a, b) in _forms(gpu_api, built, "v0", p.cs).items():
        _close(gpu_api, kind, sr, cases[0], a, x, k, "%s %s %d %s" % (kind, via, sr, name))
        assert np.array_equal(_bits(a), _bits(b)), name


@pytest.mark.parametrize("kind", KINDS)
def test_ducking_by_pulls_of_64_and_a_set_time_in_between(gpu_api, kind):
    bl = 64
    p, built, x, k, cases = _ducking(gpu_api, kind, "keybus", bl=bl)
    a, b = [_pull_all(gpu_api, built, "v0", p.cs) for _ in range(2)]
    want = _close(gpu_api, kind, 48000, cases[0], a, x, k, "%s pulls of 64" % kind)
    assert np.array_equal(_bits(a), _bits(b))
    # the state really crosses the pulls: restarted at frame 4 096 the twin is far away
    cut = _twin(gpu_api, kind, 48000, cases[0], x[4096:8192], k[4096:8192])[0]
    assert np.abs(cut.astype(np.float64) - want[4096:8192]).max() > 1e-3
    # a set_time in the middle of pulling restarts the state as it does without a key: two pulls, a jump, one pull
    at = (4000 // bl) * bl
    got = {}
    for out in ("v0", "bus", "keybus"):
        sb, fb, g = p.build(gpu_api)
        assert g.set_output(out)
        for _ in range(2):
            g.render(sb, fb)
            fb.set_time_to_next_block()
        fb.set_time(at)
        g.set_time(at)
        got[out] = np.stack(g.render(sb, fb), axis=1)
    assert np.abs(got["keybus"]).max() > 0.01
    _close(gpu_api, kind, 48000, cases[0], got["v0"], got["bus"], got["keybus"], "%s pull after set_time" % kind)


# ---- 3. topology ----
def _topology_base():
    """The ducking project with a few more places to take keys and inputs from: `bus` (a two-input Sum, materialised), `key` (the
    gated loop, inlined), `stage` (a single-input Sum over bus: read through), `deep` (three Sums behind key), `in2` (two Sums
    behind bus)."""
    p, _ = KP.ducking_project("direct")
    p.add_sum("stage", 0.5, -45.0)
    p.connect("bus", "stage")
    p.add_sum("d1", 1.0, 0.0); p.connect("key", "d1"); p.connect("n", "d1")
    p.add_sum("d2", 0.9, 10.0); p.connect("d1", "d2"); p.connect("m", "d2")
    p.add_sum("deep", 1.0, 0.0); p.connect("d2", "deep"); p.connect("key", "deep")
    p.add_sum("in1", 1.0, 0.0); p.connect("bus", "in1"); p.connect("key", "in1")
    p.add_sum("in2", 0.7, 0.0); p.connect("in1", "in2"); p.connect("n", "in2")
    return p


def _keys_and_input(api, built, p, src, keys):
    x = render_f32(api, built, src, p.cs) if src else np.zeros((p.cs * p.bl, 2), np.float32)
    return x, NK.key_sum([render_f32(api, built, k, p.cs) for k in keys])


TOPOLOGIES = {
    "key three levels deeper than the input": ("n", ["deep"]),
    "key shallower than the input": ("in2", ["key"]),
    "two key edges": ("bus", ["key", "stage"]),
    "the same key edge twice": ("bus", ["key", "key"]),
    "key source a single-input Sum stage": ("in2", ["stage"]),
    "key source also an input of the same vertex": ("deep", ["deep"]),
}


@pytest.mark.parametrize("shape", sorted(TOPOLOGIES))
@pytest.mark.parametrize("kind", KINDS)
def test_topology_matches_the_twin(gpu_api, kind, shape):
    src, keys = TOPOLOGIES[shape]
    p = _topology_base()
    _add(p, kind, "v", src, keys)
    if "also an input" in shape:   # ... and of another vertex
        p.add_sum("other", 1.0, 0.0); p.connect("deep", "other"); p.connect("n", "other")
    built = build(gpu_api, p)
    x, k = _keys_and_input(gpu_api, built, p, src, keys)
    case = KP.GATE_CASE if kind == "gate" else KP.COMP_CASE
    for form, (a, b) in _forms(gpu_api, built, "v", p.cs).items():
        want = _close(gpu_api, kind, 48000, case, a, x, k, "%s, %s, %s" % (shape, kind, form))
        assert np.array_equal(_bits(a), _bits(b))
    assert np.abs(want - x).max() > 1e-3


@pytest.mark.parametrize("kind", KINDS)
def test_key_source_an_adsr_vertex_that_would_be_read_through(gpu_api, kind):
    """`env` has one input and one input consumer, the two-input Sum `mix`: without the key edge `mix` evaluates it itself and its
    frames never exist."""
    p, _ = KP.ducking_project("keybus")
    p.event_files["f"] = np.array([(0.01, 60.0, 0.9), (0.12, 60.0, 0.0), (0.2, 62.0, 0.7), (0.4, 62.0, 0.0)], np.float32)
    p.load_midi_floww("f", "f")
    p.add_adsr("env", 1.0, 0.0, 1.0, "f", False, True, -1, [0.01, 0.1, 0.8, 0.1, 0.2, 0.01])
    p.connect("keybus", "env")
    p.add_sum("mix", 1.0, 0.0); p.connect("env", "mix"); p.connect("bus", "mix")
    _add(p, kind, "v", "mix", "env")
    built = build(gpu_api, p)
    x, k = _keys_and_input(gpu_api, built, p, "mix", ["env"])
    assert np.abs(k).max() > 0.05
    y = render_f32(gpu_api, built, "v", p.cs)
    _close(gpu_api, kind, 48000, KP.GATE_CASE if kind == "gate" else KP.COMP_CASE, y, x, k, "adsr key, %s" % kind)


@pytest.mark.parametrize("kind", KINDS)
def test_key_source_another_compressors_output(gpu_api, kind):
    p, key = KP.ducking_project("keybus")
    KP.add_comp(p, "c0", key, [], (-26.0, 2.0, 5.0, 50.0, 6.0, 3.0))
    _add(p, kind, "v", "bus", "c0")
    built = build(gpu_api, p)
    x, k = _keys_and_input(gpu_api, built, p, "bus", ["c0"])
    y = render_f32(gpu_api, built, "v", p.cs)
    _close(gpu_api, kind, 48000, KP.GATE_CASE if kind == "gate" else KP.COMP_CASE, y, x, k, "compressor as the key, %s" % kind)


@pytest.mark.parametrize("kind", KINDS)
def test_key_source_inside_a_band_pass_chain(gpu_api, kind):
    """band_mode 1: key -> b1 -> b2 -> b3 would be ONE chain launch and b2's frames would never exist; the key edge makes the
    chain materialise b2.  The output sits behind both the keyed vertex and b3; the keyed vertex is read as a stem."""
    p, _ = KP.ducking_project("direct")
    for i, (lo, hi) in enumerate(((100.0, 9000.0), (150.0, 8000.0), (200.0, 7000.0))):
        p.add_bandpass("b%d" % (i + 1), 1.0, 0.0, 1.0, lo, hi, True)
        p.connect("key" if i == 0 else "b%d" % i, "b%d" % (i + 1))
    _add(p, kind, "v", "bus", "b2")
    p.add_sum("mix", 1.0, 0.0); p.connect("v", "mix"); p.connect("b3", "mix")
    built = build(gpu_api, p)
    sb, fb, g = built
    g.set_option("band_mode", 1)
    x, k = _keys_and_input(gpu_api, built, p, "bus", ["b2"])
    assert np.abs(k).max() > 0.05
    want = _twin(gpu_api, kind, 48000, KP.GATE_CASE if kind == "gate" else KP.COMP_CASE, x, k)[0]
    g.set_output("mix")
    g.set_stems(["v"])
    fb.set_time(0)
    g.set_time(0)
    g.set_profiling(1)
    g.render_all(sb, fb, p.cs, 16)
    assert "k_band_scan" in list(g.kernel_times())
    assert np.abs(g.read_stem_pcm(0).astype(np.int64) - _quantise16(want)).max() <= 1
    assert np.abs(_quantise16(want) - _quantise16(x)).max() > 30
    g.set_stems([])


@pytest.mark.parametrize("kind", KINDS)
def test_a_keyed_vertex_without_inputs_processes_silence(gpu_api, kind):
    p, key = KP.ducking_project("direct")
    _add(p, kind, "v", None, key)
    p.add_sum("post", 1.0, 0.0); p.connect("v", "post"); p.connect("v", "post")
    built = build(gpu_api, p)
    y = render_f32(gpu_api, built, "post", p.cs)
    assert y.shape == (p.cs * p.bl, 2) and not y.any()


@pytest.mark.parametrize("kind", KINDS)
def test_a_dry_keyed_vertex_is_bitwise_the_dry_unkeyed_one(gpu_api, kind):
    p, key = KP.ducking_project("keybus")
    _add(p, kind, "plain", "bus", [], wet=0.0, gain=0.7, angle=20.0)
    _add(p, kind, "keyed", "bus", key, wet=0.00009, gain=0.7, angle=20.0)
    built = build(gpu_api, p)
    a, b = render_f32(gpu_api, built, "plain", p.cs), render_f32(gpu_api, built, "keyed", p.cs)
    assert np.array_equal(_bits(a), _bits(b)) and np.abs(a).max() > 0.05
    g = built[2]
    g.set_profiling(1)
    render_f32(gpu_api, built, "keyed", p.cs)
    assert not any(n.startswith(("k_gate", "k_comp")) for n in g.kernel_times())


@pytest.mark.parametrize("wet,gain,angle", MIX[:3])
@pytest.mark.parametrize("kind", KINDS)
def test_wet_pan_and_gain(gpu_api, kind, wet, gain, angle):
    p, key = KP.ducking_project("keybus")
    _add(p, kind, "v", "bus", key, wet=wet, gain=gain, angle=angle)
    built = build(gpu_api, p)
    x, k = _keys_and_input(gpu_api, built, p, "bus", [key])
    y = render_f32(gpu_api, built, "v", p.cs)
    want, proc = _twin(gpu_api, kind, 48000, KP.GATE_CASE if kind == "gate" else KP.COMP_CASE, x, k, wet=wet, gain=gain, angle=angle)
    lim = mix_bound(x, proc, gain, angle)
    err = np.abs(y.astype(np.float64) - want.astype(np.float64))
    print("%s wet %g gain %g angle %g: worst error / bound %.3g" % (kind, wet, gain, angle, float(np.max(err / lim))))
    assert (err <= lim).all(), (float(np.max(err / lim)), np.argwhere(err > lim)[:4].tolist())


# ---- 4. stems ----
@pytest.mark.parametrize("kind", KINDS)
def test_key_source_and_keyed_vertex_as_stems(gpu_api, kind):
    p, key = KP.ducking_project("keybus")
    _add(p, kind, "v", "bus", key)
    p.add_sum("post", 0.5, 10.0); p.connect("v", "post"); p.connect("bus", "post")
    built = build(gpu_api, p)
    sb, fb, g = built
    alone = {}
    for name in (key, "v"):
        g.set_output(name)
        fb.set_time(0); g.set_time(0)
        alone[name] = g.render_all(sb, fb, p.cs, 16, want_f32=False)[0]
    g.set_output("post")
    g.set_stems([key, "v"])
    fb.set_time(0); g.set_time(0)
    g.render_all(sb, fb, p.cs, 16)
    assert np.array_equal(g.read_stem_pcm(0), alone[key]) and np.array_equal(g.read_stem_pcm(1), alone["v"])
    assert np.abs(alone["v"].astype(np.int64)).max() > 1000
    g.set_stems([])


# ---- 5. the guard modes ----
@pytest.mark.parametrize("kind", KINDS)
def test_guard_modes_render_the_exact_forms_upstream_of_a_key(gpu_api, kind):
    p, _ = KP.ducking_project("direct", seconds=1.0)
    p.event_files["f"] = np.array([(0.01, 60.0, 0.8), (0.4, 60.0, 0.0), (0.5, 64.0, 0.6), (0.9, 64.0, 0.0)], np.float32)
    p.load_midi_floww("f", "f")
    p.add_bandpass("b1", 1.0, 0.0, 1.0, 300.0, 5000.0, True)
    p.add_bandpass("b2", 1.0, 10.0, 1.0, 200.0, 8000.0, True)
    p.add_synth("y", 0.5, 0.0, "f", 0.4, 0.3, W.HIT_ADSR, 1.0, 0.8, W.NOTE_ADSR, 0.5, W.STD_ADSR)
    p.add_sum("kb", 1.0, 0.0)
    p.connect("key", "b1"); p.connect("b1", "b2"); p.connect("b2", "kb"); p.connect("y", "kb")
    _add(p, kind, "v", "bus", "kb")
    p.set_output("v")
    outs, names = {}, {}
    for mode, (bm, sm) in (("guard", (2, 2)), ("exact", (0, 1))):
        sb, fb, g = p.build(gpu_api)
        g.set_option("band_mode", bm)
        g.set_option("sine_mode", sm)
        g.set_profiling(1)
        outs[mode] = g.render_all(sb, fb, p.cs, 16, want_pcm=False)[1]
        names[mode] = list(g.kernel_times())
    assert np.array_equal(_bits(outs["guard"]), _bits(outs["exact"])) and np.abs(outs["exact"]).max() > 0.05
    assert "k_band_scan" not in names["guard"] and "k_sine_probe" not in names["guard"], names["guard"]
    assert any(n in names["guard"] for n in ("k_band_pass", "k_band_spec")), names["guard"]


# ---- 6. a batch ----
def test_batch_members_are_bitwise_their_own_renders(gpu_api):
    projects = []
    for i in range(4):
        p, key = KP.ducking_project(KP.VIAS[i % 2])
        kind = KINDS[(i // 2) % 2]
        _add(p, kind, "v", "bus", key, (KP.gate_grid() if kind == "gate" else KP.comp_grid())[3 * i % 6], wet=[1.0, 0.6][i % 2])
        if i == 3:   # an unkeyed one beside it: both instantiations in one level
            _add(p, kind, "u", "bus", [])
            p.add_sum("out", 1.0, 0.0); p.connect("v", "out"); p.connect("u", "out")
            p.set_output("out")
        else:
            p.set_output("v")
        projects.append(p)
    cs = projects[0].cs
    own = []
    for p in projects:
        sb, fb, g = p.build(gpu_api)
        own.append(g.render_all(sb, fb, cs, 16, want_f32=False)[0])
    assert len({o.tobytes() for o in own}) == 4
    batch = gpu_api.Batch()
    for p in projects:
        batch.add(*p.build(gpu_api))
    for rep in range(2):
        batch.rewind()
        assert batch.render_all(cs, 16) == cs * 1024
        for i in range(4):
            assert np.array_equal(batch.read_pcm(i, cs), own[i]), (rep, i)


# ---- 7. the front end ----
def test_front_end_renders_a_ducked_bus(gpu_api, tmp_path):
    p, key = KP.ducking_project("keybus")
    KP.add_comp(p, "duck", "bus", key)
    KP.add_gate(p, "v", "duck", key)
    p.set_output("v")
    d = str(tmp_path / "proj")
    _write_project(p, d)
    assert "connect_key(" in open(os.path.join(d, "project.lua")).read()
    out = str(tmp_path / "m.wav")
    r = subprocess.run([sys.executable, "-m", "termdaw_amd", d, "-o", out], env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    with wave.open(out, "rb") as w:
        words = np.frombuffer(w.readframes(w.getnframes()), np.int16).reshape(-1, 2)
    pcm = p.render(gpu_api)[0]
    assert words.shape == pcm.shape and np.array_equal(words, pcm) and np.abs(pcm).max() > 1000
    # ... and the key edges are really in the path: without them the words differ
    q, _ = KP.ducking_project("keybus")
    KP.add_comp(q, "duck", "bus", [])
    KP.add_gate(q, "v", "duck", [])
    q.set_output("v")
    assert not np.array_equal(q.render(gpu_api)[0], pcm)


# ---- 8. random projects ----
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
def test_random_key_projects(gpu_api, seed):
    p = KP.random_key_project(seed)
    p.sine_mode = 1   # (the reference's sine: every render of a vertex gives the same bits whatever the output is)
    out = p.output_vertex
    whole, chunks, pulls = (_fresh(gpu_api, p, out, form) for form in ("whole", "chunks", "pulls"))
    assert np.array_equal(_bits(whole), _bits(_fresh(gpu_api, p, out))), seed
    assert np.array_equal(_bits(whole), _bits(chunks)) and np.array_equal(_bits(whole), _bits(pulls)), seed
    # the last keyed vertex against the twin on the engine's own x and k
    v = p.keyed[-1]
    kind = "comp" if seed % 2 else "gate"
    args = [c for c in p.calls["add_compressor" if kind == "comp" else "add_gate"] if c[0] == v][-1]
    gain, angle, wet, case = args[1], args[2], args[3], tuple(args[4:])
    ins = [a for a, b in p.calls["connect"] if b == v]
    keys = [a for a, b in p.calls["connect_key"] if b == v]
    x = NK.key_sum([_fresh(gpu_api, p, a) for a in ins])
    k = NK.key_sum([_fresh(gpu_api, p, a) for a in keys])
    y = _fresh(gpu_api, p, v)
    want, proc = _twin(gpu_api, kind, 48000, case, x, k, wet=wet, gain=gain, angle=angle)
    lim = mix_bound(x, proc, gain, angle)
    err = np.abs(y.astype(np.float64) - want.astype(np.float64))
    print("seed %d: %s %s keyed by %s, worst error / bound %.3g" % (seed, kind, v, keys, float(np.nanmax(err / lim))))
    assert (err <= lim).all(), (seed, v, float(np.nanmax(err / lim)), np.argwhere(~(err <= lim))[:4].tolist())
