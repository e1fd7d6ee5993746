"""The loudness meter on the host, no GPU (include/termdaw_amd.h td_graph_loudness): the K-weighting
coefficients and the true-peak FIR td_loudness_filters hands out -- BS.1770-4's published 48 kHz table, the bilinear forms
restated in numpy at other rates, the phase rule, phase 0 the unit impulse -- the device entry points failing loudly without a
render or a GPU, and the host engine measuring random projects with stems under AddressSanitizer / UBSan (tests/asan_loudness.cpp
against tests/mock_hip.cpp + tests/mock_stems.cpp + tests/mock_loudness.cpp, built like tests/test_stems_host.py)."""
import multiprocessing
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import fx_rig  # noqa: E402


def kweight_numpy(fs):
    """BS.1770-4's two stages at rate fs: the bilinear forms of the issue, restated."""
    f0, G, Q = 1681.974450955533, 3.999843853973347, 0.7071752369554196
    K = np.tan(np.pi * f0 / fs)
    Vh = 10.0 ** (G / 20.0)
    Vb = Vh ** 0.4996667741545416
    a0 = 1.0 + K / Q + K * K
    shelf = (np.array([Vh + Vb * K / Q + K * K, 2.0 * (K * K - Vh), Vh - Vb * K / Q + K * K]) / a0,
             np.array([1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]))
    f0, Q = 38.13547087602444, 0.5003270373238773
    K = np.tan(np.pi * f0 / fs)
    a0 = 1.0 + K / Q + K * K
    hp = (np.array([1.0, -2.0, 1.0]), np.array([1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]))
    return shelf, hp


def test_filters_match_the_bs1770_table(api):
    (sb, sa), (hb, ha), fir = api.loudness_filters(48000)
    np.testing.assert_allclose(sb, [1.53512485958697, -2.69169618940638, 1.19839281085285], rtol=0, atol=1e-12)
    np.testing.assert_allclose(sa, [1.0, -1.69065929318241, 0.73248077421585], rtol=0, atol=1e-12)
    np.testing.assert_array_equal(hb, [1.0, -2.0, 1.0])
    np.testing.assert_allclose(ha, [1.0, -1.99004745483398, 0.99007225036621], rtol=0, atol=1e-12)
    assert fir.shape == (4, 12)


@pytest.mark.parametrize("sr", [44100, 96000, 8000, 192000])
def test_filters_match_the_formulas(api, sr):
    (sb, sa), (hb, ha), _ = api.loudness_filters(sr)
    (nsb, nsa), (nhb, nha) = kweight_numpy(sr)
    for got, want in ((sb, nsb), (sa, nsa), (hb, nhb), (ha, nha)):
        np.testing.assert_allclose(got, want, rtol=0, atol=1e-13)


@pytest.mark.parametrize("sr,phases", [(8000, 4), (44100, 4), (48000, 4), (95999, 4), (96000, 2), (176400, 2), (191999, 2),
                                       (192000, 1), (384000, 1)])
def test_fir_phases_and_identity(api, sr, phases):
    _, _, fir = api.loudness_filters(sr)
    assert fir.shape == (phases, 12)
    unit = np.zeros(12, np.float32)
    unit[5] = 1.0
    assert np.array_equal(fir[0], unit), fir[0]
    for p in range(1, phases):   # an interpolator: the taps of every phase sum to about 1, the largest on the nearest sample
        assert abs(float(fir[p].sum()) - 1.0) < 0.02 and int(np.argmax(fir[p])) == (5 if 2 * p <= phases else 6), (p, fir[p])
    if phases == 4:   # (phases 1 and 3 mirror each other about the point half-way)
        np.testing.assert_allclose(fir[1], fir[3][::-1], rtol=0, atol=1e-7)


def test_filters_reject_bad_arguments(api):
    import ctypes as C
    with pytest.raises(api.TermdawError, match="positive"):
        api.loudness_filters(0)
    kw = (C.c_double * 10)()
    fir = np.zeros(8, np.float32)
    ph, taps = C.c_size_t(0), C.c_size_t(0)
    assert api.lib().td_loudness_filters(48000, kw, fir.ctypes.data_as(C.POINTER(C.c_float)), 8, C.byref(ph), C.byref(taps)) == 0
    assert "48 floats" in api.last_error() and ph.value == 4 and taps.value == 12


def test_graph_entry_points_fail_without_a_render(api):
    g = api.Graph(64, 48000)
    g.add_sum("a", 1.0, 0.0)
    g.set_output("a")
    with pytest.raises(api.TermdawError, match="no whole render"):
        g.loudness()
    with pytest.raises(api.TermdawError, match="not measured"):
        g.momentary(0)
    assert api.lib().td_graph_momentary(g.h, 0, None, 0) == 0 and "no such signal" in api.last_error()


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="only meaningful on a box without a GPU")
def test_device_meter_fails_without_a_gpu(api):
    assert api.device_count() == 0
    with pytest.raises(api.TermdawError, match="no HIP device"):
        api.loudness_f32(np.zeros((48000, 2), np.float32), 48000)


def _write_projects(args):
    base, seeds = args
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import test_gpu_fuzz as F
    out = []
    for seed in seeds:
        p = F.random_project(seed, allow_sinf=True)
        rng = np.random.default_rng(70_000 + seed)
        names = sorted({c[0] for k, cs in p.calls.items() if k.startswith("add_") for c in cs})
        stems = [str(x) for x in rng.choice(names, size=min(len(names), int(rng.integers(1, 4))), replace=False)]
        d = os.path.join(base, "s%d" % seed)
        lua = p.to_lua(os.path.join(d, "assets"))
        with open(os.path.join(d, "project.lua"), "w") as f:
            f.write(lua)
        with open(os.path.join(d, "meta.txt"), "w") as f:
            f.write(str(p.bl))
        with open(os.path.join(d, "stems.txt"), "w") as f:
            f.write("\n".join(stems) + "\n")
        out.append(d)
    return out


@pytest.mark.skipif(shutil.which("g++") is None or not os.path.exists("/opt/rocm/include/hip/hip_runtime_api.h"), reason="needs g++ and the HIP headers")
def test_loudness_under_sanitizers(tmp_path, tmp_path_factory):
    exe = fx_rig.asan_exe(tmp_path_factory, "asan_loudness", ["mock_stems.cpp", "mock_loudness.cpp", "asan_loudness.cpp"])
    n = int(os.environ.get("TD_ASAN_LOUD_SEEDS", "48"))
    workers = max(1, min(8, os.cpu_count() or 1))
    env = dict(os.environ, **fx_rig.ENV)
    seeds = list(range(n))
    base = str(tmp_path / "p")
    with multiprocessing.Pool(workers) as pool:
        lists = pool.map(_write_projects, [(base, seeds[i::workers]) for i in range(workers) if seeds[i::workers]])
    procs = [subprocess.Popen([exe] + lst, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for lst in lists]
    measured = signals = 0
    for p in procs:
        out, err = p.communicate(timeout=1800)
        assert p.returncode == 0, (out[-800:], err[-4000:])
        assert "asan_loudness done" in out
        measured += int(out.split(" measurements")[0].split()[-1])
        signals += int(out.split(" signals")[0].split("(")[-1])
    assert measured >= n * 2 and signals > measured, (measured, signals)
    print("asan_loudness: %d projects, %d measurements, %d signals clean" % (n, measured, signals))
