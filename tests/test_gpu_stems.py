"""Stems (td_graph_set_stems): named vertices rendered to PCM of their own by the same render as the output.

The oracle is the reference's own semantics: stem X of a render is what the same graph renders, through the same sequence
of renders, with set_output(X) -- graph.rs:98-108 visits only what reaches the output (quirk Q12), so everything upstream
of X is the same function of time and of its own carried state either way.  In the exact modes (a bare graph's defaults,
band_mode 0 / sine_mode 1) that is byte for byte."""
import os
import subprocess
import sys

import numpy as np
import pytest

from termdaw_amd import workloads as W

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from fx_rig import _write_project  # noqa: E402
from test_gpu_fuzz import random_project  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _vertex_names(p):
    names = []
    for kind, calls in p.calls.items():
        if kind.startswith("add_"):
            names += [c[0] for c in calls]
    return names


def _exact_build(p, backend):
    p.sine_mode = 1
    built = p.build(backend)
    if hasattr(built[2], "set_option"):
        built[2].set_option("band_mode", 0)
        built[2].set_option("sine_mode", 1)
    return built


def _sequence(p, built, bd, stems=()):
    """plain, scanned, continued renders (tests/test_gpu_fuzz.py): [(pcm, f32, [stem pcm], [stem peak])]"""
    sb, fb, g = built
    out = []
    for scan in (False, True, False):
        if scan:
            g.true_normalize_scan(sb, fb, p.cs)
        pcm, f = g.render_all(sb, fb, p.cs, bd)
        sp = [g.read_stem_pcm(i) for i in range(len(stems))]
        pk = [g.stem_peak(i) for i in range(len(stems))]
        out.append((pcm, f, sp, pk))
    return out


def _oracle_stem(p, oracle, stem, bd):
    ob = p.build(oracle)
    ob[2].set_output(stem)
    return _sequence(p, ob, bd)


def _peak(f):
    a = np.abs(f.astype(np.float32))
    return float("nan") if np.isnan(a).any() else float(a.max()) if a.size else 0.0


def _check_project(p, gpu_api, oracle, stems, bd, label):
    gb = _exact_build(p, gpu_api)
    gb[2].set_stems(stems)
    got = _sequence(p, gb, bd, stems)
    plain = _sequence(p, _exact_build(p, gpu_api), bd)
    for k, (g_, m_) in enumerate(zip(got, plain)):
        assert np.array_equal(g_[0], m_[0]), "%s: the master differs from a render without stems (render %d)" % (label, k)
    for i, s in enumerate(stems):
        want = _oracle_stem(p, oracle, s, bd)
        for k in range(3):
            assert np.array_equal(got[k][2][i], want[k][0]), "%s: stem %s differs from set_output(%s) (render %d, %d bits)" % (label, s, s, k, bd)
            pk, wp = got[k][3][i], _peak(want[k][1])
            assert (np.isnan(pk) and np.isnan(wp)) or pk == wp, "%s: stem %s peak %r, oracle %r" % (label, s, pk, wp)


def _stems_of(p, seed):
    rng = np.random.default_rng(10_000 + seed)
    names = _vertex_names(p)
    return [str(x) for x in rng.choice(names, size=min(len(names), int(rng.integers(1, 5))), replace=False)]


@pytest.mark.parametrize("seed", range(44))
def test_random_project_stems_are_set_output_renders(gpu_api, oracle, seed):
    p = random_project(seed)
    try:
        p.build(oracle)
    except (RuntimeError, KeyError):
        return
    stems = _stems_of(p, seed)
    _check_project(p, gpu_api, oracle, stems, 16, "seed %d" % seed)
    _check_project(p, gpu_api, oracle, stems, 32, "seed %d" % seed)
    if seed % 8 == 0:
        _check_project(p, gpu_api, oracle, stems, 8, "seed %d" % seed)
        _check_project(p, gpu_api, oracle, stems, 24, "seed %d" % seed)


@pytest.mark.parametrize("which", ["drum", "synth", "config3", "config4"])
def test_named_project_stems(gpu_api, oracle, which):
    p = {"drum": lambda: W.drum_project(seconds=1.0),
         "synth": lambda: W.synth_project(seconds=0.5),
         "config3": lambda: W.config3(seconds=1.0),
         "config4": lambda: W.config4(seconds=0.5, depth=12)}[which]()
    names = _vertex_names(p)
    stems = names[:1] + names[len(names) // 2:len(names) // 2 + 1] + names[-1:]
    stems = list(dict.fromkeys(stems))
    _check_project(p, gpu_api, oracle, stems, 16, which)


def test_chunked_and_resampled_stems(gpu_api, oracle):
    p = W.drum_project(seconds=1.0)
    stems = _vertex_names(p)[:3]
    one = _exact_build(p, gpu_api)
    one[2].set_stems(stems)
    many = _exact_build(p, gpu_api)
    many[2].set_option("max_chunk_frames", 4096)
    many[2].set_stems(stems)
    a, b = _sequence(p, one, 16, stems), _sequence(p, many, 16, stems)
    for k in range(3):
        assert np.array_equal(a[k][0], b[k][0])
        for i in range(len(stems)):
            assert np.array_equal(a[k][2][i], b[k][2][i]), "chunked stem %s differs (render %d)" % (stems[i], k)
            assert a[k][3][i] == b[k][3][i]
    # psr > render_sr: each stem through the same resampler as the output
    gb = _exact_build(p, gpu_api)
    gb[2].set_stems(stems)
    gb[2].render_all_resampled(gb[0], gb[1], p.cs, 16, 48000, 44100)
    for i, s in enumerate(stems):
        ob = p.build(oracle)
        ob[2].set_output(s)
        op, of = ob[2].render_all_resampled(ob[0], ob[1], p.cs, 16, 48000, 44100)
        assert np.array_equal(gb[2].read_stem_pcm(i), op), "resampled stem %s" % s


def test_guarded_defaults_keep_stems_exact(gpu_api, oracle):
    p = W.synth_project(seconds=0.5)
    stem = p.calls["add_bandpass"][0][0]   # (synth and debug_sine upstream of it)
    gb = p.build(gpu_api)
    gb[2].set_option("band_mode", 2)
    gb[2].set_option("sine_mode", 2)
    gb[2].set_stems([stem])
    pcm, f = gb[2].render_all(gb[0], gb[1], p.cs, 16)
    ob = p.build(oracle)
    ob[2].set_output(stem)
    sp, _ = ob[2].render_all(ob[0], ob[1], p.cs, 16)
    assert np.array_equal(gb[2].read_stem_pcm(0), sp), "guarded stem %s is not the exact render" % stem
    mp, mf = p.render(oracle)
    rms = float(np.sqrt(np.mean((f.astype(np.float64) - mf.astype(np.float64)) ** 2)))
    assert rms <= 1e-6, rms


def test_nan_stem_reports_nan_peak(gpu_api, oracle):
    for seed in range(200):
        p = random_project(seed)
        try:
            ob = p.build(oracle)
        except (RuntimeError, KeyError):
            continue
        for s in _vertex_names(p):
            ob[2].set_output(s)
            _, f = ob[2].render_all(ob[0], ob[1], p.cs, 16)
            if np.isnan(f).any():
                gb = _exact_build(p, gpu_api)
                gb[2].set_stems([s])
                gb[2].render_all(gb[0], gb[1], p.cs, 16)
                assert np.isnan(gb[2].stem_peak(0))
                return
            ob = p.build(oracle)
    pytest.fail("no NaN-producing vertex in the seeds searched")


def _launches(g):
    return {k: v[1] for k, v in g.kernel_times().items()}


def test_loop_stems_do_not_unfuse_the_headline_launch(gpu_api, oracle):
    p = W.config2(seconds=2.0)
    loops = [c[0] for c in p.calls["add_sampleloop"]]
    base = p.build(gpu_api)
    base[2].set_profiling(1)
    base_pcm, _ = base[2].render_all(base[0], base[1], p.cs, 16)
    want = _launches(base[2])
    assert want.get("k_sum"), want
    for stems in (loops[:1], loops):
        gb = p.build(gpu_api)
        gb[2].set_profiling(1)
        gb[2].set_stems(stems)
        pcm, _ = gb[2].render_all(gb[0], gb[1], p.cs, 16)
        got = _launches(gb[2])
        assert got.pop("k_stems") == 1, got
        assert got == want, (got, want)
        assert np.array_equal(pcm, base_pcm)
        for i in (0, len(stems) - 1):
            ob = p.build(oracle)
            ob[2].set_output(stems[i])
            op, _ = ob[2].render_all(ob[0], ob[1], p.cs, 16)
            assert np.array_equal(gb[2].read_stem_pcm(i), op), stems[i]


def test_zero_stems_is_free(gpu_api):
    p = W.drum_project(seconds=1.0)
    a = p.build(gpu_api)
    a[2].set_profiling(1)
    pa, _ = a[2].render_all(a[0], a[1], p.cs, 16)
    b = p.build(gpu_api)
    b[2].set_stems(_vertex_names(p)[:2])
    b[2].set_stems([])
    b[2].set_profiling(1)
    pb, _ = b[2].render_all(b[0], b[1], p.cs, 16)
    assert _launches(a[2]) == _launches(b[2])
    assert np.array_equal(pa, pb)


def test_front_end_writes_stem_files(gpu_api, tmp_path):
    p = W.drum_project(seconds=1.0)
    names = _vertex_names(p)
    a, b = names[0], names[len(names) // 2]
    d = str(tmp_path / "proj")
    _write_project(p, d)
    m = str(tmp_path / "m.wav")
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-m", "termdaw_amd", d, "--exact-bandpass", "--exact-sine", "-o", m, "--stem", a, "--stem", b],
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    assert "stem %s:" % a in r.stdout and "stem %s:" % b in r.stdout
    for s in (a, b):
        ref = str(tmp_path / ("ref_%s.wav" % s))
        st = gpu_api.State(open_dir=d)
        st.set_option("band_mode", 0)
        st.set_option("sine_mode", 1)
        assert st.refresh()
        st.g.set_output(s)
        st.render(ref)
        with open(ref, "rb") as f1, open(str(tmp_path / ("m.%s.wav" % s)), "rb") as f2:
            assert f1.read() == f2.read(), "stem file %s" % s
    bad = str(tmp_path / "bad.wav")
    r = subprocess.run([sys.executable, "-m", "termdaw_amd", d, "-o", bad, "--stem", "no_such_vertex"],
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode != 0
    assert not any(f.startswith("bad") for f in os.listdir(str(tmp_path)))


# ---- stems downstream of the output, and stems whose branch only a scan can normalise ----
def _loops_project(seconds=0.5):
    p = W.ProjectScript(48000, 1024)
    p.set_length(seconds)
    for k in range(3):
        nm = "a%d" % k
        p.assets[nm] = W.Asset(W.noise_int16(77 + k, 20000 + 977 * k))
        p.load_sample(nm, nm, "")
        p.add_sampleloop("l%d" % k, 0.5 + 0.25 * k, -30.0 + 30.0 * k, nm)
    return p


def _downstream_project():
    """3 loops -> Normalize `n` (the output) -> Sum `post` (gain, pan): a stem fed by the output."""
    p = _loops_project()
    p.add_normalize("n", 1.0, 0.0)
    for k in range(3):
        p.connect("l%d" % k, "n")
    p.add_sum("post", 0.5, 20.0)
    p.connect("n", "post")
    p.set_output("n")
    return p


def _side_project():
    """3 loops -> Sum `mix` (the output); 2 of them -> Normalize `side`, which only a stem reaches."""
    p = _loops_project()
    p.add_sum("mix", 1.0, 0.0)
    p.add_normalize("side", 0.8, 0.0)
    for k in range(3):
        p.connect("l%d" % k, "mix")
    p.connect("l0", "side")
    p.connect("l2", "side")
    p.set_output("mix")
    return p


@pytest.mark.parametrize("normalize", ["single_pass", "two_pass"])
def test_stem_downstream_of_a_normalize_output_without_f32(gpu_api, oracle, normalize):
    """The output's f32 frames are kept (and its check is not deferred) when a stem reads them, whatever "output_f32" says."""
    p = _downstream_project()
    gb = _exact_build(p, gpu_api)
    gb[2].set_option("output_f32", 0)
    if normalize == "two_pass":
        gb[2].set_option("debug.spec_normalize", 0)
    gb[2].set_stems(["post"])
    sb, fb, g = gb
    plain = _sequence(p, _exact_build(p, gpu_api), 16)
    want = _oracle_stem(p, oracle, "post", 16)
    for k, scan in enumerate((False, True, False)):
        if scan:
            g.true_normalize_scan(sb, fb, p.cs)
        pcm, _ = g.render_all(sb, fb, p.cs, 16, want_f32=False)
        assert np.array_equal(pcm, plain[k][0]), "master, render %d" % k
        assert np.array_equal(g.read_stem_pcm(0), want[k][0]), "stem post fed by the output, render %d" % k


def test_guarded_stem_downstream_of_the_output_is_exact(gpu_api, oracle):
    p = W.synth_project(seconds=0.5)
    out = p.output_vertex
    p.add_sum("post", 0.5, 0.0)
    p.connect(out, "post")
    gb = p.build(gpu_api)
    gb[2].set_option("band_mode", 2)
    gb[2].set_option("sine_mode", 2)
    gb[2].set_stems(["post"])
    pcm, _ = gb[2].render_all(gb[0], gb[1], p.cs, 16)
    ob = p.build(oracle)
    ob[2].set_output("post")
    sp, _ = ob[2].render_all(ob[0], ob[1], p.cs, 16)
    assert np.array_equal(gb[2].read_stem_pcm(0), sp), "a stem downstream of the output is not the exact render"
    mp, _ = p.render(oracle)
    assert np.array_equal(pcm, mp), "everything upstream of the stem -- the output's whole graph -- takes the exact kernels"


def _cli(d, out, stems, scan=False):
    env = dict(os.environ, PYTHONPATH=ROOT)
    cmd = [sys.executable, "-m", "termdaw_amd", d, "--exact-bandpass", "--exact-sine", "-o", out] + (["--scan"] if scan else [])
    for s in stems:
        cmd += ["--stem", s]
    return subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)


def _state_render_as_output(gpu_api, d, vertex, path, scan=False):
    st = gpu_api.State(open_dir=d)
    st.set_option("band_mode", 0)
    st.set_option("sine_mode", 1)
    assert st.refresh()
    st.g.set_output(vertex)
    if scan:
        st.scan_exact()
    st.render(path)
    with open(path, "rb") as f:
        return f.read()


@pytest.mark.parametrize("scan", [False, True])
def test_front_end_stem_fed_by_a_normalize_output(gpu_api, tmp_path, scan):
    d = str(tmp_path / "proj")
    _write_project(_downstream_project(), d)
    r = _cli(d, str(tmp_path / "m.wav"), ["post"], scan=scan)
    assert r.returncode == 0, r.stderr
    want = _state_render_as_output(gpu_api, d, "post", str(tmp_path / "ref.wav"), scan=scan)
    with open(str(tmp_path / "m.post.wav"), "rb") as f:
        assert f.read() == want


def test_front_end_scan_covers_a_stem_only_normalize(gpu_api, tmp_path):
    d = str(tmp_path / "proj")
    _write_project(_side_project(), d)
    r = _cli(d, str(tmp_path / "m.wav"), ["side"], scan=True)
    assert r.returncode == 0, r.stderr
    want = _state_render_as_output(gpu_api, d, "side", str(tmp_path / "ref.wav"), scan=True)
    with open(str(tmp_path / "m.side.wav"), "rb") as f:
        assert f.read() == want, "the scan did not cover the stem's Normalize vertex"
    # ... and the unscanned render of the same stem differs: the scan is what the comparison pins
    unscanned = _state_render_as_output(gpu_api, d, "side", str(tmp_path / "ref0.wav"), scan=False)
    assert unscanned != want


def test_front_end_rejects_a_repeated_stem(gpu_api, tmp_path):
    d = str(tmp_path / "proj")
    _write_project(_side_project(), d)
    r = _cli(d, str(tmp_path / "m.wav"), ["side", "side"])
    assert r.returncode == 1 and "Traceback" not in r.stderr and "twice" in r.stderr, r.stderr
    assert not os.path.exists(str(tmp_path / "m.wav"))


def test_stem_peak_of_a_stem_not_rendered_raises(gpu_api):
    p = _side_project()
    gb = _exact_build(p, gpu_api)
    gb[2].set_stems(["side"])
    with pytest.raises(gpu_api.TermdawError):
        gb[2].stem_peak(0)
    gb[2].render_all(gb[0], gb[1], p.cs, 16)
    assert gb[2].stem_peak(0) > 0.0
    gb[2].set_stems(["side"])   # (a new list: nothing of it rendered yet)
    with pytest.raises(gpu_api.TermdawError):
        gb[2].stem_peak(0)
