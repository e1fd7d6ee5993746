"""The loudness meter on the device (td_graph_loudness, td_batch_loudness, td_loudness_f32).

The reference is this file's own float64 restatement of ITU-R BS.1770-4 / EBU Tech 3341 / 3342 in numpy and scipy: lfilter
for the K-weighting, whole hops of round(rate / 10) frames, 400 ms blocks and 3 s windows at a step of one hop, the two gates,
the loudness range's percentiles, and the true peak as a polyphase restatement with the FIR td_loudness_filters hands out.
The termdaw reference has no loudness meter: there is nothing of its to compare with."""
import os
import subprocess
import sys
import wave

import numpy as np
import pytest
from scipy.signal import lfilter

from termdaw_amd import workloads as W

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from fx_rig import _write_project  # noqa: E402
from test_gpu_stems import _downstream_project, _loops_project  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LU, DB = 0.005, 0.001


def _lufs(p):
    with np.errstate(divide="ignore"):
        return -0.691 + 10.0 * np.log10(p)


def reference(api, x, sr):
    """BS.1770-4 / Tech 3341 / 3342 in float64 over x (frames, 2), already scaled to [-1, 1)."""
    x = np.asarray(x, np.float64)
    (sb, sa), (hb, ha), fir = api.loudness_filters(sr)
    y = lfilter(hb, ha, lfilter(sb, sa, x, axis=0), axis=0)
    H = int(round(sr / 10.0))
    nh = x.shape[0] // H
    z = (y[:nh * H] ** 2).reshape(nh, H, 2).mean(axis=1).sum(axis=1)
    P = np.array([z[j:j + 4].mean() for j in range(nh - 3)])
    mom = _lufs(P)
    integrated = -np.inf
    g = P[mom > -70.0]
    if g.size:
        rel = _lufs(g.mean()) - 10.0
        g = P[(mom > -70.0) & (mom > rel)]
        if g.size:
            integrated = float(_lufs(g.mean()))
    S = np.array([z[k:k + 30].mean() for k in range(nh - 29)])
    st = _lufs(S)
    lra = 0.0
    g = S[st > -70.0]
    if g.size:
        rel = _lufs(g.mean()) - 20.0
        v = np.sort(st[(st > -70.0) & (st > rel)])
        if v.size:
            n = v.size - 1
            lra = float(v[int(np.floor(n * 0.95 + 0.5))] - v[int(np.floor(n * 0.10 + 0.5))])
    xf = x.astype(np.float32).astype(np.float64)   # (the meter interpolates f32 samples)
    pad = np.concatenate([np.zeros((5, 2)), xf, np.zeros((6, 2))])
    tp = np.abs(xf).max() if xf.size else 0.0
    for p in range(1, fir.shape[0]):
        f = fir[p].astype(np.float64)
        for c in range(2):
            yp = np.correlate(pad[:, c], f, "valid")
            tp = max(tp, float(np.abs(yp).max()))
    with np.errstate(divide="ignore"):
        sp = 20.0 * np.log10(np.abs(xf).max()) if xf.size else -np.inf
        tpd = 20.0 * np.log10(tp)
    return {"integrated": integrated, "momentary_max": float(mom.max()) if mom.size else -np.inf,
            "short_term_max": float(st.max()) if st.size else -np.inf, "lra": lra, "true_peak": float(tpd),
            "sample_peak": float(sp), "frames": x.shape[0], "sr": sr}, mom


def _close(a, b, tol):
    if np.isinf(a) or np.isinf(b):
        return a == b
    return abs(a - b) <= tol


def check(api, got, x, sr, mom=None, label=""):
    want, wmom = reference(api, x, sr)
    for k in ("integrated", "momentary_max", "short_term_max", "lra"):
        assert _close(got[k], want[k], LU), (label, k, got[k], want[k])
    for k in ("true_peak", "sample_peak"):
        assert _close(got[k], want[k], DB), (label, k, got[k], want[k])
    assert got["frames"] == want["frames"] and got["sr"] == sr, (label, got, want)
    if mom is not None:
        assert mom.shape == wmom.shape, (label, mom.shape, wmom.shape)
        keep = wmom > -70.0
        assert np.all(np.abs(mom[keep] - wmom[keep]) <= LU), (label, np.abs(mom[keep] - wmom[keep]).max())
    return want


def _sine(level_db, seconds, sr=48000, hz=1000.0, phase=0.0):
    n = int(round(seconds * sr))
    s = (10.0 ** (level_db / 20.0)) * np.sin(2.0 * np.pi * hz * np.arange(n) / sr + phase)
    return np.stack([s, s], axis=1).astype(np.float32)


def _seq(parts, sr=48000):
    return np.concatenate([_sine(db, sec, sr) for db, sec in parts])


# ---- EBU Tech 3341 / 3342 test signals (stereo 1 kHz sines), through td_loudness_f32 ----
TECH3341 = {1: ([(-23, 20)], -23.0), 2: ([(-33, 20)], -33.0), 3: ([(-36, 10), (-23, 60), (-36, 10)], -23.0),
            4: ([(-72, 10), (-36, 10), (-23, 60), (-36, 10), (-72, 10)], -23.0), 5: ([(-26, 20), (-20, 20.1), (-26, 20)], -23.0)}
TECH3342 = {1: ([(-20, 20), (-30, 20)], 10.0), 2: ([(-20, 20), (-15, 20)], 5.0), 3: ([(-40, 20), (-20, 20)], 20.0),
            4: ([(-50, 20), (-35, 20), (-20, 20), (-35, 20), (-50, 20)], 15.0)}


@pytest.mark.parametrize("case", sorted(TECH3341))
def test_tech3341_integrated(gpu_api, case):
    parts, want = TECH3341[case]
    x = _seq(parts)
    got = gpu_api.loudness_f32(x, 48000)
    assert abs(got["integrated"] - want) <= 0.1, (case, got)
    check(gpu_api, got, x, 48000, label="3341 case %d" % case)


@pytest.mark.parametrize("case", sorted(TECH3342))
def test_tech3342_loudness_range(gpu_api, case):
    parts, want = TECH3342[case]
    x = _seq(parts)
    got = gpu_api.loudness_f32(x, 48000)
    assert abs(got["lra"] - want) <= 1.0, (case, got)
    check(gpu_api, got, x, 48000, label="3342 case %d" % case)


def test_true_peak_between_samples(gpu_api):
    """A sine at fs/4 with a 45 degree phase: every sample sits 3 dB under the crest, which the 4x interpolator finds."""
    x = _sine(-6.0, 2.0, hz=12000.0, phase=np.pi / 4)
    got = gpu_api.loudness_f32(x, 48000)
    assert abs(got["sample_peak"] - (-9.0103)) < 0.001, got
    assert abs(got["true_peak"] - (-6.0)) <= 0.2 and got["true_peak"] >= got["sample_peak"], got
    check(gpu_api, got, x, 48000, label="fs/4")


@pytest.mark.parametrize("sr", [44100, 96000, 192000])
def test_other_rates(gpu_api, sr):
    rng = np.random.default_rng(sr)
    x = (0.2 * rng.standard_normal((int(sr * 3.3), 2))).astype(np.float32)
    check(gpu_api, gpu_api.loudness_f32(x, sr), x, sr, label="noise %d" % sr)


# ---- real renders ----
def _scaled(pcm, bits):
    return pcm.astype(np.float64) / float(2 ** (bits - 1))


def test_config2_bare_graph(gpu_api):
    p = W.config2(seconds=10.0)
    sb, fb, g = p.build(gpu_api)
    pcm, _ = g.render_all(sb, fb, p.cs, 16)
    rows = g.loudness()
    assert len(rows) == 1
    m1 = g.momentary(0)
    check(gpu_api, rows[0], _scaled(pcm, 16), 48000, m1, "config2")
    again = g.loudness()
    assert np.array_equal(_bits(rows), _bits(again)), "two calls differ"
    assert np.array_equal(m1.view(np.uint64), g.momentary(0).view(np.uint64))


def test_config3_through_the_state(gpu_api, tmp_path):
    d = str(tmp_path / "c3")
    _write_project(W.config3(seconds=6.0), d)
    s = gpu_api.State(open_dir=d)
    assert s.refresh()
    pcm = s.render_to_memory()
    g = s.g
    rows = g.loudness()
    check(gpu_api, rows[0], _scaled(pcm, s.bd), s.render_sr, g.momentary(0), "config3 state")


def test_resampled_render(gpu_api):
    p = W.drum_project(seconds=3.0)
    sb, fb, g = p.build(gpu_api)
    pcm, _ = g.render_all_resampled(sb, fb, p.cs, 16, 48000, 44100)
    rows = g.loudness()
    assert rows[0]["sr"] == 44100 and rows[0]["frames"] == pcm.shape[0]
    check(gpu_api, rows[0], _scaled(pcm, 16), 44100, g.momentary(0), "resampled")


@pytest.mark.parametrize("bits", [8, 24, 32])
def test_sink_bit_depths(gpu_api, bits):
    p = W.drum_project(seconds=2.0)
    sb, fb, g = p.build(gpu_api)
    pcm, _ = g.render_all(sb, fb, p.cs, bits)
    check(gpu_api, g.loudness()[0], _scaled(pcm, bits), 48000, g.momentary(0), "%d-bit" % bits)


def test_stem_after_a_normalize_output(gpu_api):
    p = _downstream_project()
    p.set_length(2.0)
    sb, fb, g = p.build(gpu_api)
    g.set_stems(["post", "n"])
    pcm, _ = g.render_all(sb, fb, p.cs, 16)
    rows = g.loudness()
    assert len(rows) == 3
    check(gpu_api, rows[0], _scaled(pcm, 16), 48000, g.momentary(0), "output")
    check(gpu_api, rows[1], _scaled(g.read_stem_pcm(0), 16), 48000, g.momentary(1), "stem post")
    # a stem naming the output is the output, bit for bit
    assert np.array_equal(np.array(list(rows[2].values())).view(np.uint64), np.array(list(rows[0].values())).view(np.uint64))
    assert np.array_equal(g.momentary(2).view(np.uint64), g.momentary(0).view(np.uint64))
    only = g.loudness(stems=False)
    assert len(only) == 1 and only[0] == rows[0]
    with pytest.raises(gpu_api.TermdawError, match="signals asked for"):
        import ctypes as C
        out = (C.c_double * 32)()
        if not gpu_api.lib().td_graph_loudness(g.h, out, 4):
            raise gpu_api.TermdawError(gpu_api.last_error())


def _bits(rows):
    return np.array([[r[k] for k in sorted(r)] for r in rows], np.float64).view(np.uint64)


def test_batch_equals_each_graph(gpu_api):
    projects = [W.config2(seconds=2.0, n_src=8, seed_offset=k) for k in range(8)]
    b = gpu_api.Batch()
    built = [p.build(gpu_api) for p in projects]
    for sb, fb, g in built:
        b.add(sb, fb, g)
    b.render_all(projects[0].cs, 16)
    rows = b.loudness()
    assert len(rows) == 8
    for i, (sb, fb, g) in enumerate(built):
        own = g.loudness()
        assert np.array_equal(_bits(rows[i:i + 1]), _bits(own)), (i, rows[i], own[0])
    assert len({r["integrated"] for r in rows}) > 1


def test_async_equals_sync(gpu_api):
    p = W.config2(seconds=3.0)
    sb, fb, g = p.build(gpu_api)
    g.render_all(sb, fb, p.cs, 16)
    sync = g.loudness()
    g.reset_normalize_vertices(); fb.set_time(0); g.set_time(0)
    g.render_all_async(sb, fb, p.cs, 16)
    assert np.array_equal(_bits(g.loudness()), _bits(sync))


def test_loudness_call_changes_no_render(gpu_api):
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
    pcm1, f1, fams1 = render()
    g.loudness()
    pcm2, f2, fams2 = render()
    assert fams0 == fams1 == fams2 and "k_loudness" not in fams2, (fams0, fams2)
    assert np.array_equal(pcm0, pcm2) and np.array_equal(f0.view(np.uint32), f2.view(np.uint32))


# ---- edge cases ----
def test_silence(gpu_api):
    r = gpu_api.loudness_f32(np.zeros((48000 * 2, 2), np.float32), 48000)
    for k in ("integrated", "momentary_max", "short_term_max", "true_peak", "sample_peak"):
        assert r[k] == -np.inf, (k, r)
    assert r["lra"] == 0.0 and r["frames"] == 96000


def test_shorter_than_a_block(gpu_api):
    x = _sine(-20.0, 0.3)
    r = gpu_api.loudness_f32(x, 48000)
    assert r["integrated"] == -np.inf and r["momentary_max"] == -np.inf and r["lra"] == 0.0, r
    assert np.isfinite(r["true_peak"]) and np.isfinite(r["sample_peak"]), r
    check(gpu_api, r, x, 48000, label="short")


def test_nan_frame(gpu_api):
    x = _sine(-20.0, 2.0)
    x[50000, 1] = np.nan
    r = gpu_api.loudness_f32(x, 48000)
    for k in ("integrated", "momentary_max", "short_term_max", "lra", "true_peak", "sample_peak"):
        assert np.isnan(r[k]), (k, r)


def test_no_whole_render(gpu_api):
    p = W.drum_project(seconds=1.0)
    sb, fb, g = p.build(gpu_api)
    with pytest.raises(gpu_api.TermdawError, match="no whole render"):
        g.loudness()
    b = gpu_api.Batch()
    b.add(sb, fb, g)
    with pytest.raises(gpu_api.TermdawError, match="no whole render"):
        b.loudness()


# ---- the CLI ----
def _cli(d, out, *extra):
    env = dict(os.environ, PYTHONPATH=ROOT)
    return subprocess.run([sys.executable, "-m", "termdaw_amd", d, "-o", out] + list(extra), env=env, capture_output=True, text=True,
                          timeout=600)


def _wav(path):
    with wave.open(path, "rb") as w:
        assert w.getsampwidth() == 2 and w.getnchannels() == 2
        return np.frombuffer(w.readframes(w.getnframes()), "<i2").reshape(-1, 2), w.getframerate()


def test_cli_prints_loudness_lines(gpu_api, tmp_path):
    p = _loops_project(seconds=2.0)
    p.add_sum("mix", 1.0, 0.0)
    for k in range(3):
        p.connect("l%d" % k, "mix")
    p.set_output("mix")
    d = str(tmp_path / "proj")
    _write_project(p, d)
    m = str(tmp_path / "m.wav")
    r = _cli(d, m, "--loudness", "--stem", "l1")
    assert r.returncode == 0, r.stderr
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("loudness ")]
    assert len(lines) == 2 and lines[0].startswith("loudness %s: I " % m) and lines[1].startswith("loudness %s.l1.wav: I " % m[:-4])
    for ln, path in zip(lines, (m, str(tmp_path / "m.l1.wav"))):
        pcm, sr = _wav(path)
        want, _ = reference(gpu_api, pcm / 32768.0, sr)
        tok = ln.split()
        assert abs(float(tok[tok.index("I") + 1]) - want["integrated"]) < 0.051, (ln, want)
        assert abs(float(tok[tok.index("dBTP") - 1]) - want["true_peak"]) < 0.051, (ln, want)
        for f in ("LRA", "M max", "S max", "dBFS"):
            assert f in ln
    r = _cli(d, str(tmp_path / "q.wav"))
    assert r.returncode == 0 and not [ln for ln in r.stdout.splitlines() if ln.startswith("loudness ")], r.stdout
