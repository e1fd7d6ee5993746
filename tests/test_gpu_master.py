"""Loudness mastering on the device (td_graph_master, td_batch_master, td_master_f32, td_state_set_master).

The twin is this file's float64 numpy restatement of the definition in include/termdaw_amd.h: the window W and the release
coefficient a from their formulas, the detector correlated with the FIR td_loudness_filters hands out, the hold with
scipy.ndimage.maximum_filter1d, the release as a cumulative max in the log domain, the smoothing as a cumsum, all at the gain
and internal ceiling the call reports.  Loudness and true peak of the results are measured again with test_gpu_loudness's
reference meter."""
import os
import subprocess
import sys
import wave

import numpy as np
import pytest
from scipy.ndimage import maximum_filter1d

from termdaw_amd import workloads as W

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_loudness import reference  # noqa: E402
from fx_rig import _write_project  # noqa: E402
from test_gpu_stems import _loops_project  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def gain_curve(api, x, sr, g, cp, lookahead_ms=5.0, release_ms=100.0):
    """G[n] of one pass at gain g under the internal ceiling cp over x (frames, 2), scaled to [-1, 1)."""
    n = x.shape[0]
    Wn = max(1, int(np.floor(lookahead_ms * sr / 1000.0 + 0.5)))
    a = np.exp(-1.0 / (release_ms * sr / 1000.0))
    _, _, fir = api.loudness_filters(sr)
    xf = np.asarray(x, np.float32).astype(np.float64)
    pad = np.concatenate([np.zeros((5, 2)), xf, np.zeros((6, 2))])
    p = np.abs(xf).max(axis=1)
    for ph in range(1, fir.shape[0]):
        pts = np.maximum(*[np.abs(np.correlate(pad[:, c], fir[ph].astype(np.float64), "valid")) for c in range(2)])
        p = np.maximum(p, pts)
        p[1:] = np.maximum(p[1:], pts[:-1])
    q = maximum_filter1d(np.concatenate([p, np.zeros(Wn)]), size=Wn, mode="constant", cval=0.0, origin=-(Wn // 2))[:n]
    with np.errstate(divide="ignore"):
        h = np.where(q > 0, np.minimum(1.0, cp / (g * np.where(q > 0, q, 1.0))), 1.0)
        k = np.arange(n, dtype=np.float64)
        la = np.log(a)
        w = np.maximum.accumulate(np.log(1.0 - h) - k * la)
    u = np.exp(w + k * la)
    e = np.concatenate([np.full(Wn - 1, 1.0 - u[0]), 1.0 - u])   # (before frame 0: e[0], the limiter settled on the opening peak)
    cs = np.concatenate([[0.0], np.cumsum(e)])
    return (cs[Wn:Wn + n] - cs[:n]) / Wn


def twin_words(api, pcm, bits, sr, rep, **kw):
    scale = float(2 ** (bits - 1))
    G = gain_curve(api, pcm / scale, sr, rep["gain"], rep["ceiling"], **kw)
    y = np.trunc(pcm.astype(np.float64) * rep["gain"] * G[:, None])
    return np.clip(y, -scale, scale - 1), G


def check_ceiling(api, words, bits, sr, rep, C):
    scale = float(2 ** (bits - 1))
    c = 10.0 ** (C / 20.0)
    assert np.abs(words.astype(np.int64)).max() <= c * scale + 1
    assert words.min() >= -scale and words.max() <= scale - 1
    ref, _ = reference(api, words / scale, sr)
    assert rep["true_peak"] <= C and ref["true_peak"] <= C + 1e-3, (rep["true_peak"], ref["true_peak"])
    return ref


def _bits(rep):
    return np.array([rep[k] for k in sorted(rep)], np.float64).view(np.uint64)


def _clicks(sr, seconds=3.0, seed=0):
    rng = np.random.default_rng(seed)
    t = np.arange(int(sr * seconds)) / sr
    env = (np.sin(2 * np.pi * 1.5 * t) > 0).astype(np.float64)
    x = 0.25 * np.sin(2 * np.pi * 440.0 * t) * env
    x = np.stack([x, 0.8 * x], axis=1)
    for i in rng.integers(0, len(t), 40):
        x[i] += rng.uniform(-0.9, 0.9, 2)
    return x.astype(np.float32)


@pytest.mark.parametrize("sr,kind", [(44100, "clicks"), (48000, "noise"), (96000, "clicks"), (48000, "clicks")])
def test_f32_matches_the_twin(gpu_api, sr, kind):
    x = _clicks(sr) if kind == "clicks" else (0.3 * np.random.default_rng(1).standard_normal((sr * 3, 2))).astype(np.float32)
    y, rep = gpu_api.master_f32(x, sr, -12.0, -1.0)
    G = gain_curve(gpu_api, x, sr, rep["gain"], rep["ceiling"])
    want = x.astype(np.float64) * rep["gain"] * G[:, None]
    assert np.abs(y - want).max() <= 2e-6, np.abs(y - want).max()
    assert abs(rep["min_gain"] - G.min()) <= 1e-6, (rep["min_gain"], G.min())
    assert rep["true_peak"] <= -1.0 and (kind != "clicks" or rep["min_gain"] < 1.0), rep
    ref, _ = reference(gpu_api, y, sr)
    assert ref["true_peak"] <= -1.0 + 1e-3
    if rep["met"]:
        assert abs(ref["integrated"] - (-12.0)) <= 0.1 + 0.005


# Lookahead / release over their ranges: W = 1 (0.1 ms at 8 kHz), W = 2049 and 4097 (a W - 1 that is a multiple of the
# 2048-frame tile: the smoothing's window then starts exactly on a tile), W = 4800 and 9600 (the detector's branch for a window
# longer than a tile), and the shortest and longest release.
EDGES = [(8000, 0.1, 100.0), (48000, 42.6875, 100.0), (48000, 4097 / 48.0, 100.0), (48000, 100.0, 10000.0), (44100, 5.0, 1.0),
         (96000, 100.0, 1.0), (48000, 0.1, 10000.0)]


@pytest.mark.parametrize("sr,lookahead,release", EDGES)
def test_f32_window_and_release_edges_match_the_twin(gpu_api, sr, lookahead, release):
    x = _clicks(sr, seed=sr)
    y, rep = gpu_api.master_f32(x, sr, -12.0, -1.0, lookahead, release)
    G = gain_curve(gpu_api, x, sr, rep["gain"], rep["ceiling"], lookahead, release)
    want = x.astype(np.float64) * rep["gain"] * G[:, None]
    assert np.abs(y - want).max() <= 2e-6, (np.abs(y - want).max(), int(np.argmax(np.abs(y - want).max(axis=1))))
    assert abs(rep["min_gain"] - G.min()) <= 1e-6, (rep["min_gain"], G.min())
    assert rep["true_peak"] <= -1.0 and rep["min_gain"] < 1.0, rep
    y2, rep2 = gpu_api.master_f32(x, sr, -12.0, -1.0, lookahead, release)
    assert np.array_equal(y.view(np.uint32), y2.view(np.uint32)) and np.array_equal(_bits(rep), _bits(rep2))


def test_quiet_signal_needs_no_limiting(gpu_api):
    p = W.config2(seconds=10.0)
    sb, fb, g = p.build(gpu_api)
    pcm, _ = g.render_all(sb, fb, p.cs, 16)
    rep = g.master(-30.0, -1.0)
    assert rep["min_gain"] == 1.0 and rep["passes"] == 1 and rep["met"], rep
    assert abs(rep["integrated"] - (-30.0)) <= 0.1
    want = np.clip(np.trunc(pcm.astype(np.float64) * rep["gain"]), -32768, 32767)
    assert np.array_equal(g.read_pcm().astype(np.float64), want)
    x = _clicks(48000) * 0.01
    y, r = gpu_api.master_f32(x, 48000, -40.0, -1.0)
    assert r["min_gain"] == 1.0 and r["passes"] == 1
    assert np.array_equal(y, (x.astype(np.float64) * r["gain"]).astype(np.float32))


def _render(api, p, bits, resample=None):
    sb, fb, g = p.build(api)
    if resample:
        pcm, _ = g.render_all_resampled(sb, fb, p.cs, bits, 48000, resample)
    else:
        pcm, _ = g.render_all(sb, fb, p.cs, bits)
    return sb, fb, g, pcm


@pytest.mark.parametrize("case", ["config2", "drum8", "drum16", "drum24", "drum32", "resampled"])
def test_renders_match_the_twin(gpu_api, case):
    if case == "config2":
        p, bits, rs = W.config2(seconds=10.0), 16, None
    elif case == "resampled":
        p, bits, rs = W.drum_project(seconds=3.0), 16, 44100
    else:
        p, bits, rs = W.drum_project(seconds=3.0), int(case[4:]), None
    sb, fb, g, pcm = _render(gpu_api, p, bits, rs)
    sr = rs or 48000
    rep = g.master(-14.0, -1.0)
    got = g.read_pcm()
    want, G = twin_words(gpu_api, pcm, bits, sr, rep)
    d = np.abs(got.astype(np.float64) - want)
    if bits <= 16:
        assert d.max() <= 1 and np.mean(d > 0) <= 1e-3, (d.max(), np.mean(d > 0))
    else:
        assert d.max() / 2 ** (bits - 1) <= 2e-6, d.max()
    assert abs(rep["min_gain"] - G.min()) <= 1e-6
    ref = check_ceiling(gpu_api, got, bits, sr, rep, -1.0)
    if rep["met"]:
        assert abs(ref["integrated"] - (-14.0)) <= 0.1 + 0.005, (ref["integrated"], rep)
    assert rep["sr"] == sr and rep["frames"] == pcm.shape[0]


def test_unreachable_target_keeps_the_ceiling(gpu_api):
    p = W.config2(seconds=10.0)
    sb, fb, g, pcm = _render(gpu_api, p, 16)
    rep = g.master(-6.0, -1.0)
    assert not rep["met"] and rep["passes"] >= 4, rep
    check_ceiling(gpu_api, g.read_pcm(), 16, 48000, rep, -1.0)


def test_report_calls_and_renders(gpu_api):
    p = W.config2(seconds=3.0)
    sb, fb, g, pcm = _render(gpu_api, p, 16)
    rep = g.master(-14.0)
    loud = g.loudness()[0]
    assert np.array_equal(np.array([loud[k] for k in gpu_api.LOUDNESS_FIELDS], np.float64).view(np.uint64),
                          np.array([rep[k] for k in gpu_api.LOUDNESS_FIELDS], np.float64).view(np.uint64))
    g.master(-14.0)
    r20 = g.master(-20.0)
    w20 = g.read_pcm()
    # a fresh graph mastered to -20 alone: the same words and report
    sb2, fb2, g2, pcm2 = _render(gpu_api, p, 16)
    assert np.array_equal(pcm, pcm2)
    alone = g2.master(-20.0)
    assert np.array_equal(g2.read_pcm(), w20) and np.array_equal(_bits(alone), _bits(r20))
    # a new render drops the kept words: a 24-bit render mastered, then a 32-bit one (the same bytes per frame, other words)
    # masters to what a fresh graph's 32-bit render does -- kept 24-bit words would give another report
    g.reset_normalize_vertices(); fb.set_time(0); g.set_time(0)
    g.render_all(sb, fb, p.cs, 24)
    r24 = g.master(-20.0)
    g.reset_normalize_vertices(); fb.set_time(0); g.set_time(0)
    pcm32, _ = g.render_all(sb, fb, p.cs, 32)
    r32 = g.master(-20.0)
    sb4, fb4, g4, pcm32b = _render(gpu_api, p, 32)
    assert np.array_equal(pcm32, pcm32b)
    fresh = g4.master(-20.0)
    assert np.array_equal(_bits(r32), _bits(fresh)) and not np.array_equal(_bits(r32), _bits(r24))
    assert np.array_equal(g.read_pcm(pcm32.shape[0], 32), g4.read_pcm(pcm32.shape[0], 32))
    # async equals sync: an asynchronous 16-bit render after the 32-bit one masters to the 16-bit render's words and report
    g.reset_normalize_vertices(); fb.set_time(0); g.set_time(0)
    g.render_all_async(sb, fb, p.cs, 16)
    assert np.array_equal(_bits(g.master(-20.0)), _bits(r20)) and np.array_equal(g.read_pcm(pcm.shape[0], 16), w20)


def test_batch_equals_each_graph(gpu_api):
    projects = [W.config2(seconds=2.0, n_src=8, seed_offset=k) for k in range(8)]
    built = [p.build(gpu_api) for p in projects]
    b = gpu_api.Batch()
    for sb, fb, g in built:
        b.add(sb, fb, g)
    b.render_all(projects[0].cs, 16)
    rows = b.master(-16.0, -1.5)
    words = [g.read_pcm(r["frames"], 16) for (_, _, g), r in zip(built, rows)]
    assert len({round(r["input_integrated"], 3) for r in rows}) > 1
    for i, (sb, fb, g) in enumerate(built):
        own = g.master(-16.0, -1.5)
        assert np.array_equal(_bits(own), _bits(rows[i])), (i, own, rows[i])
        assert np.array_equal(g.read_pcm(rows[i]["frames"], 16), words[i])


def test_no_master_call_changes_no_render(gpu_api):
    p = W.config2(seconds=2.0)
    sb, fb, g = p.build(gpu_api)

    def render():
        g.reset_normalize_vertices(); fb.set_time(0); g.set_time(0)
        g.set_profiling(True)
        pcm, f = g.render_all(sb, fb, p.cs, 16)
        fams = set(g.kernel_times())
        g.set_profiling(False)
        return pcm, f, fams
    pcm0, f0, fams0 = render()
    g.master(-14.0)
    pcm1, f1, fams1 = render()
    assert fams0 == fams1 and not [f for f in fams1 if f.startswith("k_master")], (fams0, fams1)
    assert np.array_equal(pcm0, pcm1) and np.array_equal(f0.view(np.uint32), f1.view(np.uint32))
    g.set_profiling(True)
    g.master(-14.0)
    fams = set(g.kernel_times())
    g.set_profiling(False)
    assert {"k_master_detect", "k_master_scan", "k_master_carry", "k_master_apply", "k_loudness"} <= fams, fams


def test_silence_has_nothing_to_master(gpu_api):
    with pytest.raises(gpu_api.TermdawError, match="nothing to master"):
        gpu_api.master_f32(np.zeros((48000, 2), np.float32), 48000, -14.0)


# ---- the State and the CLI ----
def _cli(d, out, *extra):
    env = dict(os.environ, PYTHONPATH=ROOT)
    return subprocess.run([sys.executable, "-m", "termdaw_amd", d, "-o", out] + list(extra), env=env, capture_output=True, text=True,
                          timeout=600)


def _wav(path):
    with wave.open(path, "rb") as w:
        assert w.getsampwidth() == 2 and w.getnchannels() == 2
        return np.frombuffer(w.readframes(w.getnframes()), "<i2").reshape(-1, 2), w.getframerate()


def _project(tmp_path):
    p = _loops_project(seconds=3.0)
    p.add_sum("mix", 1.0, 0.0)
    for k in range(3):
        p.connect("l%d" % k, "mix")
    p.set_output("mix")
    d = str(tmp_path / "proj")
    _write_project(p, d)
    return d


def test_state_masters_its_renders(gpu_api, tmp_path):
    d = _project(tmp_path)
    s = gpu_api.State(open_dir=d)
    assert s.refresh()
    plain = s.render_to_memory()
    assert s.master_report() is None
    s.set_master(-16.0, -1.0)
    got = s.render_to_memory()
    rep = s.master_report()
    assert np.array_equal(got, s.g.read_pcm(rep["frames"], s.bd)) and rep["passes"] >= 1
    g2 = gpu_api.State(open_dir=d)
    assert g2.refresh()
    assert np.array_equal(g2.render_to_memory(), plain)
    s.set_master(None)
    assert np.array_equal(s.render_to_memory(), plain) and s.master_report() is None


def test_cli_master(gpu_api, tmp_path):
    d = _project(tmp_path)
    plain = str(tmp_path / "plain.wav")
    r = _cli(d, plain, "--stem", "l1")
    assert r.returncode == 0, r.stderr
    m = str(tmp_path / "m.wav")
    r = _cli(d, m, "--master", "-16:-1", "--stem", "l1", "--loudness")
    assert r.returncode == 0, r.stderr
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("master ")]
    assert len(lines) == 1 and lines[0].startswith("master %s: I " % m) and "passes" in lines[0], r.stdout
    pcm, sr = _wav(m)
    s = gpu_api.State(open_dir=d)
    assert s.refresh()
    s.set_master(-16.0)
    assert np.array_equal(s.render_to_memory(), pcm)
    ref, _ = reference(gpu_api, pcm / 32768.0, sr)
    assert abs(ref["integrated"] - (-16.0)) <= 0.1 + 0.005 and ref["true_peak"] <= -1.0 + 1e-3, ref
    loud = [ln for ln in r.stdout.splitlines() if ln.startswith("loudness %s:" % m)]
    assert len(loud) == 1 and abs(float(loud[0].split()[3]) - ref["integrated"]) < 0.051, (loud, ref)
    # stems are written unmastered; a run without --master writes the same bytes as before
    with open(str(tmp_path / "m.l1.wav"), "rb") as a, open(str(tmp_path / "plain.l1.wav"), "rb") as b:
        assert a.read() == b.read()
    again = str(tmp_path / "again.wav")
    assert _cli(d, again, "--stem", "l1").returncode == 0
    with open(plain, "rb") as a, open(again, "rb") as b:
        assert a.read() == b.read()
