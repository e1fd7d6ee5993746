"""The parametric EQ vertex on the host, no GPU (include/termdaw_amd.h td_graph_add_eq): td_eq_coefficients
against the cookbook formulas and against facts of the response; Hmax against a dense grid; the float64 twin
(tests/np_eq.py) against the FFT of the same coefficients; parameter ranges rejected with messages that name the parameter,
through the C ABI and through the Lua front-end; the canonical dump line; the derivation of the GPU test's bound constant E
from the numpy emulation of the tiled scan; the host engine on random projects with EQ vertices under AddressSanitizer / UBSan
(tests/asan_eq.cpp against tests/mock_hip.cpp + tests/mock_eq.cpp, whose mock launches check every descriptor's bounds, tiling,
carry words, matrix powers and launch order); and the guard rule and the launch lists, read from the launch families and the
path gains the mock build reports."""
import math
import multiprocessing
import os
import subprocess
import sys

import numpy as np
import pytest

from termdaw_amd import workloads as W

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import eq_projects as EP  # noqa: E402
import fx_rig  # noqa: E402
import np_eq as NE  # noqa: E402
from fx_rig import ENV, driver_report, PARENT_LAUNCHES, _families, oracle_input  # noqa: E402


def coeffs(api, kind, sr, f, q, g):
    b, a, hmax = api.eq_coefficients(kind, sr, f, q, g)
    return np.concatenate([b, a[1:]]), hmax


PARAM_GRID = [(kind, sr, f, q, g) for sr in (8000, 44100, 48000, 96000, 192000) for kind in NE.KINDS
              for f in (10.0, 20.0, 100.0, 1000.0, 0.25 * sr, 0.45 * sr) for q in (0.1, 0.5, 0.707, 3.0, 20.0)
              for g in ((-24.0, -3.0, 0.0, 6.0, 24.0) if kind in NE.HAS_GAIN else (0.0,))]


def test_coefficients_are_the_cookbook_formulas(api):
    """Within 4 ulp of float64 over a parameter grid: the same operations, so only libm's last bits can differ."""
    worst = 0.0
    for kind, sr, f, q, g in PARAM_GRID:
        c, _ = coeffs(api, kind, sr, f, q, g)
        want = NE.cookbook(kind, sr, f, q, g)
        ulps = np.abs(c - want) / np.spacing(np.abs(want))
        worst = max(worst, float(ulps.max()))
        assert (ulps <= 4.0).all(), (kind, sr, f, q, g, c, want)
        assert abs(c[4]) < 1.0 and abs(c[3]) < 1.0 + c[4]   # the stability triangle
    print("td_eq_coefficients vs the cookbook: worst %.2f ulp over %d cases" % (worst, len(PARAM_GRID)))
    # the kinds without gain ignore gain_db, NaN included
    for kind in ("lowpass", "highpass", "bandpass", "notch"):
        assert np.array_equal(coeffs(api, kind, 48000, 1000.0, 1.0, 0.0)[0], coeffs(api, kind, 48000, 1000.0, 1.0, float("nan"))[0])
        assert np.array_equal(coeffs(api, kind, 48000, 1000.0, 1.0, 0.0)[0], coeffs(api, kind, 48000, 1000.0, 1.0, 99.0)[0])


# (Tolerances: the five coefficients are rounded to float64, and near z = 1 the denominator 1 + a1 + a2 = 4 sin^2(w0 / 2) is
# as small as 1e-7 -- 10 Hz at 96 kHz -- so a response there is known to 2^-52 / 1e-7 = 2e-9 relative, 2e-8 dB; 1e-6 dB leaves
# room for that and is far below anything a wrong formula would give.)
def _db(x):
    return 20.0 * math.log10(abs(x))


@pytest.mark.parametrize("sr", [44100, 48000, 96000])
def test_response_facts(api, sr):
    for f, q in ((100.0, 0.707), (1000.0, 3.0), (10.0, 20.0), (0.45 * sr, 0.1), (5000.0, 20.0)):
        w0 = 2.0 * math.pi * float(np.float32(f)) / sr
        for g in (-24.0, -3.0, 6.0, 24.0):
            c, _ = coeffs(api, "peak", sr, f, q, g)
            assert abs(_db(NE.response(c, w0)) - g) < 1e-6, ("peak", f, q, g)   # |H| at f0 is gain_db
            for kind, w in (("lowshelf", 0.0), ("highshelf", math.pi)):
                c, _ = coeffs(api, kind, sr, f, q, g)
                assert abs(_db(NE.response(c, w)) - g) < 1e-6, (kind, f, q, g)   # the shelf's own end sits at gain_db
                assert abs(_db(NE.response(c, math.pi - w))) < 1e-6, (kind, f, q, g)   # ... and the other end at 0 dB
        c, _ = coeffs(api, "bandpass", sr, f, q, 0.0)
        assert abs(_db(NE.response(c, w0))) < 1e-6 and abs(NE.response(c, 0.0)) < 1e-9 and abs(NE.response(c, math.pi)) < 1e-9
        c, _ = coeffs(api, "notch", sr, f, q, 0.0)
        # (the zero sits at w0 exactly; evaluated in float64 near z = 1 what is left is rounding over |1 + a1 z^-1 + a2 z^-2|)
        assert abs(NE.response(c, w0)) < 1e-6 and abs(_db(NE.response(c, 0.0))) < 1e-6 and abs(_db(NE.response(c, math.pi))) < 1e-6
        c, _ = coeffs(api, "lowpass", sr, f, q, 0.0)
        assert abs(_db(NE.response(c, 0.0))) < 1e-6 and abs(NE.response(c, math.pi)) < 1e-12
        assert abs(abs(NE.response(c, w0)) - float(np.float32(q))) < 1e-6 * max(1.0, q)   # |H(w0)| = Q
        c, _ = coeffs(api, "highpass", sr, f, q, 0.0)
        assert abs(_db(NE.response(c, math.pi))) < 1e-6 and abs(NE.response(c, 0.0)) < 1e-12


def dense_grid(sr):
    """65 536 frequencies in [0, pi]: 32 768 evenly spaced (1.5 Hz apart at 96 kHz) and 32 768 spaced by a constant ratio from
    1 Hz up (ratio 1.0003).  The narrowest peak of the range, Q = 20, is within 0.1 % of its top over a relative width of
    sqrt(0.002) / 2Q = 1.1e-3 of its centre: the even part resolves that from 1.4 kHz up, the ratio part everywhere below."""
    return np.concatenate([np.linspace(0.0, math.pi, 32768), np.geomspace(2.0 * math.pi / sr, math.pi, 32768)])


def test_hmax_bounds_the_response_on_a_dense_grid(api):
    worst_lo, worst_hi = 9.0, 0.0
    for sr in (44100, 48000, 96000):
        w = dense_grid(sr)
        z1 = np.exp(-1j * w)
        z2 = z1 * z1
        for kind, f, q, g in EP.grid_cases(sr) + [(k, 3000.0, 1.0, 0.0) for k in NE.KINDS]:
            c, hmax = coeffs(api, kind, sr, f, q, g)
            top = float(np.abs((c[0] + c[1] * z1 + c[2] * z2) / (1.0 + c[3] * z1 + c[4] * z2)).max())
            r = hmax / top
            worst_lo, worst_hi = min(worst_lo, r), max(worst_hi, r)
            assert top * (1.0 - 1e-12) <= hmax <= 1.001 * top, (kind, sr, f, q, g, hmax, top)
    print("Hmax / the grid's maximum: %.12f .. %.6f" % (worst_lo, worst_hi))


@pytest.mark.parametrize("kind,f,q,g", [("peak", 1000.0, 3.0, 12.0), ("lowshelf", 200.0, 0.707, -9.0), ("bandpass", 4000.0, 8.0, 0.0),
                                        ("highpass", 80.0, 0.707, 0.0), ("notch", 2000.0, 20.0, 0.0)])
def test_twin_impulse_response_is_the_fft_of_the_coefficients(api, kind, f, q, g):
    n = 1 << 16   # (every case has rung out far below 1e-16 by then: the circular response is the linear one)
    c, _ = coeffs(api, kind, 48000, f, q, g)
    x = np.zeros((n, 2), np.float32)
    x[0] = (1.0, -0.5)
    h, end = NE.biquad(x, c)
    assert np.abs(end).max() < 1e-30
    H = np.fft.rfft(h[:, 0])
    want = NE.response(c, np.linspace(0.0, math.pi, n // 2 + 1))
    assert np.abs(H - want).max() < 1e-11 * max(1.0, np.abs(want).max())
    assert np.allclose(h[:, 1], -0.5 * h[:, 0], rtol=0, atol=1e-15)   # the channels are independent and the filter linear
    # ... and p of the whole vertex is that, rounded once
    y, _ = NE.eq(x, c, processed=True)
    assert np.array_equal(y, h.astype(np.float32))


def test_twin_split_anywhere_is_the_one_piece_result(api):
    c, _ = coeffs(api, "peak", 48000, 300.0, 5.0, 18.0)
    x = (np.random.default_rng(4).standard_normal((5000, 2)) * 0.5).astype(np.float32)
    kw = dict(wet=0.7, gain=0.5, angle=30.0)
    whole, end = NE.eq(x, c, **kw)
    for cut in (1, 777, 2048, 4999):
        a, st = NE.eq(x[:cut], c, **kw)
        b, end2 = NE.eq(x[cut:], c, state=st, **kw)
        assert np.array_equal(np.concatenate([a, b]).view(np.uint32), whole.view(np.uint32)) and np.array_equal(end, end2)
    dry, st = NE.eq(x, c, wet=0.00009, state=np.ones((2, 2)))
    assert np.array_equal(dry, x) and np.array_equal(st, np.ones((2, 2)))   # wet < 0.0001: untouched, the state stays


def test_twin_keeps_non_finite_frames_out_of_the_state(api):
    c, _ = coeffs(api, "lowshelf", 48000, 500.0, 0.707, 12.0)
    x = (np.random.default_rng(6).standard_normal((600, 2)) * 0.3).astype(np.float32)
    x[100] = [np.nan, 0.5]
    x[200] = [0.1, np.inf]
    y, st = NE.eq(x, c)
    p, _ = NE.eq(x, c, processed=True)
    assert np.isnan(p[100, 0]) and p[200, 1] == np.inf   # the frame's p is the input sample itself ...
    assert np.isnan(y[100, 0]) and np.isfinite(y[100, 1]) and np.isnan(y[200, 1]) and np.isfinite(y[200, 0])   # (inf + 1 (inf - inf))
    assert np.isfinite(np.delete(y, [100, 200], axis=0)).all() and np.isfinite(st).all()
    z = x.copy()
    z[100, 0] = 0.0
    z[200, 1] = 0.0
    assert np.array_equal(np.delete(NE.eq(z, c)[0], [100, 200], axis=0), np.delete(y, [100, 200], axis=0))


# ---- ranges ----
GOOD = dict(kind="peak", freq_hz=1000.0, q=1.0, gain_db=6.0)
RANGES = dict(freq_hz=(10.0, 21600.0), q=(0.1, 20.0), gain_db=(-24.0, 24.0))
BAD = [(k, v) for k, (lo, hi) in RANGES.items() for v in (np.nextafter(np.float32(lo), np.float32(-1e9)), np.nextafter(np.float32(hi), np.float32(1e9)),
                                                           float("nan"), float("inf"), float("-inf"))]


def _args(**kw):
    a = dict(GOOD)
    a.update(kw)
    return [a["kind"], float(a["freq_hz"]), float(a["q"]), float(a["gain_db"])]


@pytest.mark.parametrize("name,value", BAD)
def test_out_of_range_parameters_are_rejected_by_name(api, name, value):
    g = api.Graph(64, 48000)
    with pytest.raises(api.TermdawError, match=name):
        g.add_eq("e", 1.0, 0.0, 1.0, *_args(**{name: value}))
    with pytest.raises(api.TermdawError, match=name):
        k, f, q, gd = _args(**{name: value})
        api.eq_coefficients(k, 48000, f, q, gd)


@pytest.mark.parametrize("kind", [-1, 7, 1 << 20])
def test_out_of_range_kinds_are_rejected_by_name(api, kind):
    g = api.Graph(64, 48000)
    with pytest.raises(api.TermdawError, match="kind"):
        g.add_eq("e", 1.0, 0.0, 1.0, kind, 1000.0, 1.0, 0.0)
    with pytest.raises(api.TermdawError, match="kind"):
        api.eq_coefficients(kind, 48000, 1000.0, 1.0, 0.0)
    with pytest.raises(ValueError, match="kind"):
        g.add_eq("e", 1.0, 0.0, 1.0, "bell", 1000.0, 1.0, 0.0)


def test_range_ends_are_accepted_and_follow_the_rate(api):
    for sr in (8000, 44100, 48000, 96000, 192000):
        g = api.Graph(64, sr)
        g.add_sum("in", 1.0, 0.0)
        top = 0.45 * sr
        assert float(np.float32(top)) == top
        for i, kind in enumerate(NE.KINDS):
            g.add_eq("lo%d" % i, 1.0, 0.0, 1.0, kind, 10.0, 0.1, -24.0)
            g.add_eq("hi%d" % i, 1.0, 0.0, 1.0, i, top, 20.0, 24.0)
            assert g.connect("in", "lo%d" % i) and g.connect("in", "hi%d" % i)
        with pytest.raises(api.TermdawError, match="freq_hz"):
            g.add_eq("over", 1.0, 0.0, 1.0, "peak", float(np.nextafter(np.float32(top), np.float32(1e9))), 1.0, 0.0)
        g.add_eq("nogain", 1.0, 0.0, 1.0, "notch", 50.0, 20.0, float("nan"))   # gain_db is ignored by the kinds without gain
        g.add_eq("wet", 1.0, 0.0, 7.0, *_args())   # (wet is clamped, not rejected: graph.rs:256)
        g.add_eq("dry", 1.0, 0.0, -3.0, *_args())
        assert g.set_output("hi1") and g.check_graph()


def _lua(line):
    return fx_rig._lua(line, "e")


@pytest.mark.parametrize("name,value", [(k, v) for k, v in BAD if math.isfinite(v)])
def test_lua_rejects_the_same_ranges(api, name, value):
    s = api.State("", 48000, 64)
    k, f, q, gd = _args(**{name: value})
    assert not s.refresh(_lua('add_eq("e", 1.0, 0.0, 1.0, "%s", %r, %r, %r);' % (k, f, q, gd)))
    assert name in api.last_error(), api.last_error()
    if not (name == "freq_hz" and value > 100.0):   # (the upper end of freq_hz depends on the rate: known when the graph is built)
        assert "line 2" in api.last_error(), api.last_error()


@pytest.mark.parametrize("kind", ["bell", "Peak", "", "4"])
def test_lua_rejects_unknown_kind_strings(api, kind):
    s = api.State("", 48000, 64)
    assert not s.refresh(_lua('add_eq("e", 1.0, 0.0, 1.0, "%s", 1000.0, 1.0, 0.0);' % kind))
    err = api.last_error()
    assert "kind" in err and "line 2" in err and "lowshelf" in err, err
    assert not s.refresh(_lua('add_eq("e", 1.0, 0.0, 1.0, {}, 1000.0, 1.0, 0.0);')) and "line 2" in api.last_error()


def test_lua_accepts_and_dumps_the_canonical_line(api):
    for kind in NE.KINDS:
        s = api.State("", 48000, 64)
        assert s.refresh(_lua('add_eq("e", 0.5, -30, 1, "%s", 100.5, 4, -18);' % kind)), api.last_error()
        dump = s.dump_calls()
        band = api.State("", 48000, 64)
        assert band.refresh('add_sum("in", 1.0, 0.0);\nadd_bandpass("b", 0.5, -30, 1, 100.5, 4, true);\nconnect("in", "b");\nset_output("b");\n'), api.last_error()
        # the numbers print as add_bandpass prints the same values
        half, m30, one, x1005, four = band.dump_calls().split('add_bandpass("b",')[1].split(")")[0].split(",")[:5]
        line = [ln for ln in dump.splitlines() if ln.startswith("add_eq(")]
        assert len(line) == 1
        args = line[0][len("add_eq("):-1].split(",")
        assert args[:7] == ['"e"', half, m30, one, '"%s"' % kind, x1005, four] and len(args) == 8 and " " not in line[0], line


def test_project_script_records_and_writes_the_call(tmp_path):
    p = W.ProjectScript(48000, 64)
    p.add_sum("in", 1.0, 0.0)
    p.add_eq("e", 1.0, 0.0, 1.0, "highshelf", 8000.0, 0.707, -6.0)
    p.connect("in", "e")
    p.set_output("e")
    assert p.calls["add_eq"] == [("e", 1.0, 0.0, 1.0, "highshelf", 8000.0, 0.707, -6.0)]
    assert 'add_eq("e", 1.0, 0.0, 1.0, "highshelf", 8000.0, 0.707, -6.0);' in p.to_lua(str(tmp_path))


# ---- the bound of tests/test_gpu_eq.py ----


def _emulate(api, sr, cases, want_f64):
    cs = np.array([coeffs(api, kind, sr, f, q, g)[0] for kind, f, q, g in cases])
    worst, worst64, weakest = (0.0, None), 0.0, (9e9, None)
    for kind in EP.INPUTS:
        x = oracle_input(kind, sr)
        assert len(x) > 5 * NE.TILE and np.abs(x).max() > 0.05
        ser, _ = NE.biquad(x, cs)
        peak = np.abs(ser).max(axis=(1, 2))
        r = np.abs(NE.blocked(x, cs) - ser).max(axis=(1, 2)) / peak
        i = int(r.argmax())
        if r[i] > worst[0]:
            worst = (float(r[i]), (cases[i], sr, kind))
        if want_f64:
            r64 = np.abs(NE.blocked(x, cs, power_dtype=np.float64) - ser).max(axis=(1, 2)) / peak
            worst64 = max(worst64, float(r64.max()))
        acts = np.abs(ser - x.astype(np.float64)[None]).max(axis=(1, 2)) / (np.abs(x).max() * (2.0 ** -23 + EP.E))
        j = int(acts.argmin())
        if acts[j] < weakest[0]:
            weakest = (float(acts[j]), (cases[j], sr, kind))
    return worst, worst64, weakest


def test_the_emulated_scan_stays_inside_the_committed_constant(api):
    """E = 8 x the worst max|blocked - serial| / max|serial| of the numpy emulation over the GPU test's own grid and inputs; this
    recomputes that worst figure and fails above E / 8.  Also: with float64-squared powers the same emulation is two orders of
    magnitude outside, and every grid case changes its input by far more than the bound (so the GPU test cannot pass on a
    filter that does nothing).  The same for the 96 kHz cases below the grid and their own constant."""
    worst, worst64, weakest = (0.0, None), 0.0, (9e9, None)
    for sr in EP.RATES:
        w, w64, wk = _emulate(api, sr, EP.grid_cases(sr), True)
        worst, worst64, weakest = max(worst, w, key=lambda t: t[0]), max(worst64, w64), min(weakest, wk, key=lambda t: t[0])
    print("emulated scan: worst %.3g = %.4g x 2^-24 of the peak at %s; float64-squared powers %.3g x 2^-24; the weakest case moves "
          "its input by %.3g bounds (%s)" % (worst[0], worst[0] * 2.0 ** 24, worst[1], worst64 * 2.0 ** 24, weakest[0], weakest[1]))
    assert worst[0] <= EP.E_EMULATED and EP.E == 8.0 * EP.E_EMULATED and EP.E <= 2.0 ** -28
    assert worst64 > 100.0 * EP.E
    assert weakest[0] > 64.0
    low, _, weak_low = _emulate(api, 96000, EP.low_cases(), False)
    print("below the grid (10 and 20 Hz at 96 kHz): worst %.3g = %.4g x 2^-24 of the peak at %s" % (low[0], low[0] * 2.0 ** 24, low[1]))
    assert low[0] <= EP.E_LOW_EMULATED and EP.E_LOW == 8.0 * EP.E_LOW_EMULATED and weak_low[0] > 64.0


# ---- the host engine under sanitizers ----
@pytest.fixture(scope="module")
def asan_exe(tmp_path_factory):
    return fx_rig.asan_exe(tmp_path_factory, "asan_eq", ["mock_guard.cpp", "mock_eq.cpp", "asan_eq.cpp"])


def test_eq_projects_under_sanitizers(asan_exe, tmp_path):
    n = int(os.environ.get("TD_ASAN_EQ_SEEDS", "32"))
    workers = max(1, min(8, os.cpu_count() or 1))
    seeds = list(range(n))
    base = str(tmp_path / "p")
    with multiprocessing.Pool(workers) as pool:
        lists = pool.map(EP.write_projects, [(base, seeds[i::workers]) for i in range(workers) if seeds[i::workers]])
    procs = [subprocess.Popen([asan_exe] + lst, env=dict(os.environ, **ENV), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for lst in lists]
    launches = vertices = carried = fresh = rejected = 0
    for p in procs:
        out, err = p.communicate(timeout=1800)
        assert p.returncode == 0, (out[-800:], err[-4000:])
        tail = out.split("asan_eq done:")[1]
        launches += int(tail.split("k_eq launches ")[1].split()[0])
        vertices += int(tail.split("(")[1].split()[0])
        fresh += int(tail.split(" entered fresh")[0].split()[-1])
        carried += int(tail.split(" entered with carried state")[0].split()[-1])
        rejected += int(tail.split(" rejected refreshes")[0].split()[-1])
    # multi-chunk renders and block pulls enter with carried state; every project is within the ranges
    assert rejected == 0 and launches >= n // 2 and vertices >= launches and fresh > 0 and carried > 0, (rejected, launches, vertices, fresh, carried)
    print("asan_eq: %d projects, %d launches, %d vertices (%d fresh, %d carried) clean" % (n, launches, vertices, fresh, carried))


def _guard_project(shape):
    """(band_plain is the control of the path gain; the dry one has wet < 0.0001: a k_sum launch, gain 1)"""
    return fx_rig.guard_project(shape, lambda p, name, dry: p.add_eq(name, 1.0, 0.0, 0.00009 if dry else 0.75, "peak", 1000.0, 2.0, 12.0), name="e")


EQ_LAUNCHES = ("k_eq_local", "k_eq_carry", "k_eq_apply")


def test_guard_modes_carry_the_estimate_through_an_eq(api, asan_exe, tmp_path):
    """band_mode 2 / sine_mode 2 (the driver's profiled render): upstream of an EQ the scan / fast forms stay, and the guard's
    estimate at the output is the one of the same project without the EQ times (1 - wet) + wet Hmax."""
    shapes = ("band_up", "band_plain", "band_dry", "sine_up", "sine_free")
    fams, gains, _ = driver_report(asan_exe, tmp_path, {s: _guard_project(s) for s in shapes})
    exact = ("k_band_pass", "k_band_spec")
    for s in ("band_up", "band_plain", "band_dry"):
        assert "k_band_scan" in fams[s] and not any(k in fams[s] for k in exact), (s, fams[s])
    assert all(fams["band_up"].get(k) == 1 for k in EQ_LAUNCHES), fams["band_up"]
    assert [k for k in fams["band_up"] if k.startswith("k_eq")] == list(EQ_LAUNCHES), fams["band_up"]
    # wet < 0.0001 compiles to k_sum: the launch list of the project with a Sum in the EQ's place
    assert not any(k.startswith("k_eq") for k in fams["band_dry"]) and list(fams["band_dry"].items()) == list(fams["band_plain"].items()), (fams["band_dry"], fams["band_plain"])
    for s in ("sine_up", "sine_free"):
        assert "k_sine_probe" in fams[s], (s, fams[s])
    assert all(fams["sine_up"].get(k) == 1 for k in EQ_LAUNCHES) and not any(k.startswith("k_eq") for k in fams["sine_free"])
    # the path gain: the driver prints the audit's gain from the band-pass vertex to the output (AuditHead)
    _, hmax = coeffs(api, "peak", 48000, 1000.0, 2.0, 12.0)
    assert abs(hmax - 10.0 ** (12.0 / 20.0)) < 1e-9
    want = (1.0 - 0.75) + 0.75 * hmax
    assert gains["band_plain"]["path"] > 0.0
    assert abs(gains["band_up"]["path"] / gains["band_plain"]["path"] - want) < 1e-6 * want, (gains, want)
    assert abs(gains["band_dry"]["path"] / gains["band_plain"]["path"] - 1.0) < 1e-6, gains


def test_projects_without_an_eq_keep_their_launch_list(asan_exe, tmp_path):
    """The launch lists of drum_project, config 2 and config 4 (families and launch counts of one profiled render under the
    front-end's guard modes) as the parent commit compiled them."""
    projects = {"drums": W.drum_project(seconds=0.5), "config2": W.config2(seconds=0.5, n_src=8), "config4": W.config4(seconds=0.5, depth=6)}
    fams = _families(asan_exe, tmp_path, projects)
    for name in projects:
        got = " ".join("%s=%d" % kv for kv in fams[name].items())
        assert not any(k.startswith("k_eq") for k in fams[name]) and got == PARENT_LAUNCHES[name], (name, got)


# (recorded on the parent commit with its own driver of the same form, tests/asan_comp.cpp, on these project directories)
