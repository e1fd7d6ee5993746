"""The compressor vertex on the host, no GPU (include/termdaw_amd.h td_graph_add_compressor): parameter ranges
rejected with messages that name the parameter, through the C ABI and through the Lua front-end; the canonical dump line; known
answers of the float64 twin (tests/np_compressor.py) that can be derived by hand; the host engine on random projects with
compressor vertices under AddressSanitizer / UBSan (tests/asan_comp.cpp against tests/mock_hip.cpp + tests/mock_comp.cpp, whose
mock launches check every descriptor's bounds, tiling, carry slots and launch order); and the guard rule -- upstream of a
compressor the exact forms, downstream of it the scan -- read from the launch families the mock build reports."""
import math
import multiprocessing
import os
import subprocess
import sys

import numpy as np
import pytest

from termdaw_amd import workloads as W

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import comp_projects as CP  # noqa: E402
import fx_rig  # noqa: E402
import np_compressor as NC  # noqa: E402
from fx_rig import ENV, _families  # noqa: E402

GOOD = dict(threshold_db=-18.0, ratio=4.0, attack_ms=5.0, release_ms=100.0, knee_db=6.0, makeup_db=0.0)
RANGES = dict(threshold_db=(-80.0, 0.0), ratio=(1.0, 1000.0), attack_ms=(0.0, 1000.0), release_ms=(1.0, 10000.0), knee_db=(0.0, 40.0),
              makeup_db=(-40.0, 40.0))
ORDER = ["threshold_db", "ratio", "attack_ms", "release_ms", "knee_db", "makeup_db"]
BAD = [(k, v) for k, (lo, hi) in RANGES.items() for v in (np.nextafter(np.float32(lo), np.float32(-1e9)), np.nextafter(np.float32(hi), np.float32(1e9)),
                                                           float("nan"), float("inf"), float("-inf"))]


def _args(**kw):
    return fx_rig._args(GOOD, ORDER, as_float=True, **kw)


@pytest.mark.parametrize("name,value", BAD)
def test_out_of_range_parameters_are_rejected_by_name(api, name, value):
    fx_rig.out_of_range_is_rejected_by_name(api, 48000, lambda g, *a: g.add_compressor("c", 1.0, 0.0, 1.0, *a), None, _args(**{name: value}), name)


def test_range_ends_are_accepted(api):
    fx_rig.range_ends_are_accepted(api, 48000, lambda g, *a: g.add_compressor(*a), "c", RANGES, ORDER, _args())


def _lua(line):
    return fx_rig._lua(line, "c")


@pytest.mark.parametrize("name,value", [(k, v) for k, v in BAD if math.isfinite(v)])
def test_lua_rejects_the_same_ranges(api, name, value):
    fx_rig.lua_rejects_the_same_ranges(api, 48000, "add_compressor", _args(**{name: value}), name)


def test_lua_accepts_and_dumps_the_canonical_line(api):
    s = api.State("", 48000, 64)
    assert s.refresh(_lua('add_compressor("c", 0.5, -30, 1, -18, 4, 0, 100.5, 6, 3);')), api.last_error()
    dump = s.dump_calls()
    band = api.State("", 48000, 64)
    assert band.refresh('add_sum("in", 1.0, 0.0);\nadd_bandpass("b", 0.5, -30, 1, 100.5, 4, true);\nconnect("in", "b");\nset_output("b");\n'), api.last_error()
    # the numbers print as add_bandpass prints the same values
    nums = band.dump_calls().split('add_bandpass("b",')[1].split(")")[0].split(",")   # 0.5, -30, 1, 100.5, 4, true
    half, m30, one, x1005, four = nums[:5]
    line = [ln for ln in dump.splitlines() if ln.startswith("add_compressor(")]
    assert len(line) == 1
    args = line[0][len("add_compressor("):-1].split(",")
    assert args[0] == '"c"' and args[1] == half and args[2] == m30 and args[3] == one and args[5] == four and args[7] == x1005, line
    assert len(args) == 10 and " " not in line[0]
    # add_lv2fx stays parsed and dropped
    s2 = api.State("", 48000, 64)
    assert s2.refresh('add_sum("i", 1.0, 0.0);\nadd_sum("a", 1.0, 0.0);\nconnect("i", "a");\nadd_lv2fx("fx", 1.0, 0.0, 1.0, "comp");\nset_output("a");\n'), api.last_error()
    assert 'add_lv2fx("fx"' in s2.dump_calls()


def test_project_script_records_and_writes_the_call(tmp_path):
    p = W.ProjectScript(48000, 64)
    p.add_sum("in", 1.0, 0.0)
    p.add_compressor("c", 1.0, 0.0, 1.0, -18.0, 4.0, 5.0, 100.0, 6.0, 0.0)
    p.connect("in", "c")
    p.set_output("c")
    assert p.calls["add_compressor"] == [("c", 1.0, 0.0, 1.0, -18.0, 4.0, 5.0, 100.0, 6.0, 0.0)]
    assert 'add_compressor("c", 1.0, 0.0, 1.0, -18.0, 4.0, 5.0, 100.0, 6.0, 0.0);' in p.to_lua(str(tmp_path))


# ---- the twin's known answers ----
def _const(level_db, n, sign=1.0):
    a = np.float32(10.0 ** (level_db / 20.0))
    return np.stack([np.full(n, sign * a, np.float32), np.full(n, np.float32(0.25) * a, np.float32)], axis=1)


def test_twin_settles_at_the_static_curve():
    """-6 dBFS against T = -18, R = 4, hard knee: 12 dB over, d = 0.75 x 12 = 9 dB, output at -15 dBFS."""
    x = _const(-6.0, 48000)
    y, (y1, yL) = NC.compress(x, 48000, -18.0, 4.0, 5.0, 100.0, 0.0, 0.0)
    level = 20.0 * math.log10(float(np.float32(10.0 ** (-6.0 / 20.0))))
    d = 0.75 * (level + 18.0)
    assert abs(d - 9.0) < 1e-6 and y1 == d and abs(yL - d) < 1e-9
    assert abs(20.0 * math.log10(abs(float(y[-1, 0]))) - (-15.0)) < 1e-5
    assert abs(float(y[-1, 1]) / float(y[-1, 0]) - 0.25) < 1e-6   # stereo-linked: one gain for both channels


def test_twin_below_threshold_is_the_makeup_gain_exactly():
    x = (np.random.default_rng(3).uniform(-1, 1, (4000, 2)) * 10.0 ** (-40.0 / 20.0)).astype(np.float32)
    for M in (0.0, 6.0, -12.5):
        p, st = NC.compress(x, 44100, -30.0, 8.0, 1.0, 50.0, 0.0, M, processed=True)
        G = 10.0 ** (float(np.float32(M)) / 20.0)
        assert np.array_equal(p, (x.astype(np.float64) * G).astype(np.float32)) and st == (0.0, 0.0)
    y, _ = NC.compress(x, 44100, -30.0, 8.0, 1.0, 50.0, 0.0, 0.0)
    assert np.array_equal(y.view(np.uint32), x.view(np.uint32))   # G = 1: l + 1 (l - l) = l


def test_twin_knee_is_continuous_at_both_ends():
    T, R, Wk = -20.0, 4.0, 10.0
    for o, want in ((-Wk / 2, 0.0), (Wk / 2, 0.75 * Wk / 2)):
        for eps in (-1e-9, 0.0, 1e-9):
            s = 10.0 ** ((T + o + eps) / 20.0)
            # (float64 levels: the f32 grid is too coarse to sit 1e-9 dB from the knee's end)
            x = np.array([[s, 0.0]], np.float64)
            xs = np.maximum(np.abs(x[:, 0]), np.abs(x[:, 1]))
            oo = 20.0 * np.log10(xs) - T
            slope = 1.0 - 1.0 / R
            if 2 * oo[0] < -Wk:
                d = 0.0
            elif 2 * abs(oo[0]) <= Wk:
                d = slope * (oo[0] + Wk / 2) ** 2 / (2 * Wk)
            else:
                d = slope * oo[0]
            assert abs(d - want) < 1e-8, (o, eps, d, want)
    # ... and the twin's own branches on f32 levels either side of each end agree with the two formulas to the grid's step
    lv = np.array([T - Wk / 2 - 0.01, T - Wk / 2 + 0.01, T + Wk / 2 - 0.01, T + Wk / 2 + 0.01])
    x = np.stack([10.0 ** (lv / 20.0), np.zeros(4)], axis=1).astype(np.float32)
    d = NC.wanted_reduction(x, T, R, Wk)
    assert d[0] == 0.0 and 0.0 < d[1] < 1e-5 and abs(d[2] - 0.75 * Wk / 2) < 0.01 and abs(d[3] - 0.75 * Wk / 2) < 0.01 and d[2] < d[3]
    # hard knee: exactly at the threshold nothing is wanted
    assert NC.wanted_reduction(np.array([[1.0, 0.0]], np.float32), 0.0, 4.0, 0.0)[0] == 0.0


def test_twin_attack_zero_follows_the_release_stage():
    x = (np.random.default_rng(5).standard_normal((3000, 2)) * 0.4).astype(np.float32)
    d = NC.wanted_reduction(x, -24.0, 3.0, 4.0)
    aR, aA = NC.coefficients(48000, 0.0, 20.0)
    assert aA == 0.0
    yL, (y1, yl) = NC.detector(d, aR, aA)
    y1s, v = np.empty(len(d)), 0.0
    for n in range(len(d)):
        v = max(d[n], aR * v)
        y1s[n] = v
    assert np.array_equal(yL, y1s) and y1 == yl == y1s[-1]


def test_twin_ignores_non_finite_frames_in_the_state():
    x = _const(-6.0, 600)
    x[100] = [np.nan, 0.5]
    x[200] = [0.1, np.inf]
    x[300] = [0.0, -0.0]
    d = NC.wanted_reduction(x, -18.0, 4.0, 0.0)
    assert d[100] == 0.0 and d[200] == 0.0 and d[300] == 0.0 and d[99] > 8.9
    y, st = NC.compress(x, 48000, -18.0, 4.0, 1.0, 100.0, 0.0, 0.0)
    assert np.isnan(y[100, 0]) and np.isfinite(y[100, 1]) and np.isfinite(y[101]).all() and np.isfinite(st).all()


@pytest.mark.parametrize("cut", [1, 777, 2048, 4999])
def test_twin_split_anywhere_is_the_one_piece_result(cut):
    x = (np.random.default_rng(cut).standard_normal((5000, 2)) * 0.5).astype(np.float32)
    kw = dict(threshold_db=-20.0, ratio=6.0, attack_ms=3.0, release_ms=80.0, knee_db=8.0, makeup_db=2.0, wet=0.7, gain=0.5, angle=30.0)
    whole, end = NC.compress(x, 48000, **kw)
    a, st = NC.compress(x[:cut], 48000, **kw)
    b, end2 = NC.compress(x[cut:], 48000, state=st, **kw)
    assert np.array_equal(np.concatenate([a, b]).view(np.uint32), whole.view(np.uint32)) and end == end2


# ---- the host engine under sanitizers ----
@pytest.fixture(scope="module")
def asan_exe(tmp_path_factory):
    return fx_rig.asan_exe(tmp_path_factory, "asan_comp", ["mock_comp.cpp", "asan_comp.cpp"])


def test_compressor_projects_under_sanitizers(asan_exe, tmp_path):
    n = int(os.environ.get("TD_ASAN_COMP_SEEDS", "32"))
    workers = max(1, min(8, os.cpu_count() or 1))
    seeds = list(range(n))
    base = str(tmp_path / "p")
    with multiprocessing.Pool(workers) as pool:
        lists = pool.map(CP.write_projects, [(base, seeds[i::workers]) for i in range(workers) if seeds[i::workers]])
    procs = [subprocess.Popen([asan_exe] + lst, env=dict(os.environ, **ENV), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for lst in lists]
    launches = vertices = carried = fresh = 0
    for p in procs:
        out, err = p.communicate(timeout=1800)
        assert p.returncode == 0, (out[-800:], err[-4000:])
        tail = out.split("asan_comp done:")[1]
        launches += int(tail.split("k_comp launches ")[1].split()[0])
        vertices += int(tail.split("(")[1].split()[0])
        fresh += int(tail.split(" entered fresh")[0].split()[-1])
        carried += int(tail.split(" entered with carried state")[0].split()[-1])
    # every project holds a compressor vertex; multi-chunk renders and block pulls enter with carried state
    assert launches >= n and vertices >= launches and fresh > 0 and carried > 0, (launches, vertices, fresh, carried)
    print("asan_comp: %d projects, %d launches, %d vertices (%d fresh, %d carried) clean" % (n, launches, vertices, fresh, carried))


def _guard_project(shape):
    return fx_rig.guard_project(shape, lambda p, name, dry: p.add_compressor(name, 1.0, 0.0, 1.0, -30.0, 4.0, 1.0, 100.0, 6.0, 0.0))


def test_guard_modes_keep_the_exact_forms_upstream_of_a_compressor(asan_exe, tmp_path):
    """band_mode 2 / sine_mode 2 (the driver's profiled render): the launch families each shape went through."""
    fams = _families(asan_exe, tmp_path, {s: _guard_project(s) for s in ("band_up", "band_down", "band_both", "sine_up", "sine_free")})
    exact = ("k_band_pass", "k_band_spec")
    up, down, both = fams["band_up"], fams["band_down"], fams["band_both"]
    assert "k_band_scan" not in up and any(k in up for k in exact), up
    assert "k_band_scan" in down and not any(k in down for k in exact), down
    assert "k_band_scan" in both and any(k in both for k in exact), both
    for f in (up, down, both):
        assert all(f.get(k) == 1 for k in ("k_comp_detect", "k_comp_carry_y1", "k_comp_env", "k_comp_carry_yl", "k_comp_apply")), f
    sup, sfree = fams["sine_up"], fams["sine_free"]
    assert "k_sine_probe" not in sup and "k_synth" in sup, sup
    assert "k_sine_probe" in sfree or "k_sources" in sfree or "k_synth" in sfree, sfree
    assert ("k_sine_probe" in sfree), sfree
    assert not any(k.startswith("k_comp") for k in sfree), sfree
