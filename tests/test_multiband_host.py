"""The multiband vertex on the host, no GPU (include/termdaw_amd.h td_graph_add_multiband): parameter ranges rejected
with messages that name the parameter, through the C ABI and through the Lua front-end (NaN included); no key edge into a
multiband; td_graph_reset; the canonical dump line; td_multiband_params against numpy's evaluation of the formulas; facts of the
float64 twin (tests/np_multiband.py) that can be derived by hand; the crossover's tiled scans restated in numpy
(np_multiband.blocked: the kernels' tile geometry, the 18-state block operator, its join order) against the serial loop, within
the bound's constant, which this file derives; the host engine on random projects with multiband vertices under AddressSanitizer /
UBSan (a stand-alone program: tests/asan_fx.cpp as it is, against tests/mock_hip.cpp + tests/mock_guard.cpp +
tests/mock_multiband.cpp, whose mock launches check every descriptor); and the guard rule and the launch lists, read from the
launch families the mock build reports."""
import math
import multiprocessing
import os
import subprocess
import sys

import numpy as np
import pytest

from termdaw_amd import workloads as W

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fx_rig  # noqa: E402
import multiband_projects as MP  # noqa: E402
import np_multiband as NM  # noqa: E402
from fx_rig import ENV, PARENT_LAUNCHES, _families, oracle_input  # noqa: E402
SR = 48000

# add_multiband's arguments behind `wet`, flat, as the Lua line has them
ORDER = ["lo_hz", "hi_hz", "thr_lo", "thr_mid", "thr_hi", "ratio_lo", "ratio_mid", "ratio_hi", "attack_ms", "release_ms", "knee_db",
         "makeup_lo", "makeup_mid", "makeup_hi"]
GOOD = dict(lo_hz=200.0, hi_hz=2000.0, thr_lo=-30.0, thr_mid=-24.0, thr_hi=-18.0, ratio_lo=4.0, ratio_mid=2.0, ratio_hi=8.0, attack_ms=5.0,
            release_ms=50.0, knee_db=6.0, makeup_lo=0.0, makeup_mid=3.0, makeup_hi=-3.0)
# the word of the message per parameter, and the ranges
WORD = {k: k for k in ("lo_hz", "hi_hz", "attack_ms", "release_ms", "knee_db")}
WORD.update({"thr_" + b: "threshold_db" for b in ("lo", "mid", "hi")})
WORD.update({"ratio_" + b: "ratio" for b in ("lo", "mid", "hi")})
WORD.update({"makeup_" + b: "makeup_db" for b in ("lo", "mid", "hi")})
RANGES = dict(lo_hz=(40.0, None), hi_hz=(None, 0.45 * SR), attack_ms=(0.0, 1000.0), release_ms=(1.0, 10000.0), knee_db=(0.0, 40.0))
for _b in ("lo", "mid", "hi"):
    RANGES["thr_" + _b] = (-60.0, 0.0)
    RANGES["ratio_" + _b] = (1.0, 1000.0)
    RANGES["makeup_" + _b] = (-40.0, 40.0)
NAN = float("nan")


def _below(v):
    return float(np.nextafter(np.float32(v), np.float32(-1e9)))


def _above(v):
    return float(np.nextafter(np.float32(v), np.float32(1e9)))


BAD = [(k, _below(lo)) for k, (lo, hi) in RANGES.items() if lo is not None] + [(k, _above(hi)) for k, (lo, hi) in RANGES.items() if hi is not None]
BAD += [(k, NAN) for k in RANGES]
BAD += [("hi_hz", _below(400.0)), ("hi_hz", 200.0), ("lo_hz", _above(1000.0)), ("lo_hz", 2000.0)]   # hi_hz >= 2 lo_hz: the message names both


def _flat(**kw):
    a = dict(GOOD)
    a.update(kw)
    return [a[k] for k in ORDER]


def _args(**kw):
    """Graph.add_multiband's arguments behind `wet`: the per-band triples as tuples."""
    f = _flat(**kw)
    return (f[0], f[1], tuple(f[2:5]), tuple(f[5:8]), f[8], f[9], f[10], tuple(f[11:14]))


# ---- ranges, key edges, the Lua line, the project script ----
@pytest.mark.parametrize("name,value", BAD)
def test_out_of_range_parameters_are_rejected_by_name(api, name, value):
    g = api.Graph(64, SR)
    for call in (lambda: g.add_multiband("v", 1.0, 0.0, 1.0, *_args(**{name: value})), lambda: api.multiband_params(SR, *_args(**{name: value}))):
        with pytest.raises(api.TermdawError, match=WORD[name]) as e:
            call()
        assert "multiband:" in str(e.value)


def test_range_ends_are_accepted_and_follow_the_rate(api):
    g = api.Graph(64, SR)
    g.add_sum("in", 1.0, 0.0)
    ends = [_args(lo_hz=40.0, hi_hz=80.0, thr_lo=-60.0, thr_mid=0.0, ratio_lo=1.0, ratio_hi=1000.0, attack_ms=0.0, release_ms=1.0, knee_db=0.0,
                  makeup_lo=-40.0, makeup_hi=40.0),
            _args(lo_hz=0.225 * SR, hi_hz=0.45 * SR, attack_ms=1000.0, release_ms=10000.0, knee_db=40.0),
            _args(lo_hz=40.0, hi_hz=0.45 * SR)]
    for i, c in enumerate(ends):
        g.add_multiband("v%d" % i, 1.0, 0.0, 1.0, *c)
        assert g.connect("in", "v%d" % i)
    g.add_multiband("wet", 1.0, 0.0, 7.0, *_args())   # (wet is clamped, not rejected: graph.rs:256)
    g.add_multiband("dry", 1.0, 0.0, -3.0, *_args())
    assert g.set_output("v1") and g.check_graph()
    for sr in (44100, 96000):   # hi_hz's end is 0.45 of the graph's own rate
        h = api.Graph(64, sr)
        h.add_multiband("p", 1.0, 0.0, 1.0, *_args(hi_hz=0.45 * sr))
        with pytest.raises(api.TermdawError, match="hi_hz"):
            h.add_multiband("q", 1.0, 0.0, 1.0, *_args(hi_hz=_above(0.45 * sr)))


def test_multiband_params_needs_room_and_three_values_per_band(api):
    import ctypes
    out = (ctypes.c_double * 27)()
    f3 = lambda *v: (ctypes.c_float * 3)(*v)   # noqa: E731
    a = (SR, 200.0, 2000.0, f3(-30, -30, -30), f3(4, 4, 4), 5.0, 50.0, 6.0, f3(0, 0, 0), out)
    assert api.lib().td_multiband_params(*a, 27) == 1
    assert api.lib().td_multiband_params(*a, 26) == 0 and "multiband_params" in api.last_error()
    with pytest.raises(ValueError):
        api.multiband_params(SR, 200.0, 2000.0, (-30.0, -30.0), (4, 4, 4), 5.0, 50.0, 6.0, (0, 0, 0))


def test_a_multiband_takes_no_key(api):
    g = api.Graph(64, SR)
    g.add_sum("a", 1.0, 0.0)
    g.add_multiband("m", 1.0, 0.0, 1.0, *_args())
    g.add_compressor("c", 1.0, 0.0, 1.0, -20.0, 4.0, 5.0, 50.0, 6.0, 0.0)
    assert not g.connect_key("a", "m") and api.last_error() == "connect_key: m takes no key input"
    assert g.connect_key("m", "c"), api.last_error()   # any vertex may BE the key
    assert g.connect("a", "m")


def test_reset_clears_multibands(api):
    g = api.Graph(64, SR)
    g.add_sum("a", 1.0, 0.0)
    g.add_multiband("m", 1.0, 0.0, 1.0, *_args())
    assert g.connect("a", "m") and g.connect("m", "a") is False
    api.lib().td_graph_reset(g.h)
    assert not g.connect("a", "m") and "cannot be found" in api.last_error()   # (the vertices are gone)
    g.add_sum("a", 1.0, 0.0)
    g.add_multiband("m", 1.0, 0.0, 1.0, *_args())
    assert g.connect("m", "a"), api.last_error()   # the edge of before is gone: what was a loop then is none now


def _lua(line):
    return fx_rig._lua(line, "g")


def _lit(v):
    if math.isnan(v):
        return "0/0"
    return repr(float(v))


@pytest.mark.parametrize("name,value", BAD)
def test_lua_rejects_the_same_ranges(api, name, value):
    s = api.State("", SR, 64)
    line = 'add_multiband("g", 1.0, 0.0, 1.0, %s);' % ", ".join(_lit(v) for v in _flat(**{name: value}))
    assert not s.refresh(_lua(line))
    assert WORD[name] in api.last_error() and "multiband:" in api.last_error(), api.last_error()


def test_lua_accepts_and_dumps_the_canonical_line(api):
    s = api.State("", SR, 64)
    assert s.refresh(_lua('add_multiband("g", 0.5, -30, 1, 100.5, 4000, -30, -30, 0, 4, 4, 1, 0.5, 50, 4, 0, 0.5, 4);')), api.last_error()
    dump = s.dump_calls()
    band = api.State("", SR, 64)
    assert band.refresh('add_sum("in", 1.0, 0.0);\nadd_bandpass("b", 0.5, -30, 1, 100.5, 4, true);\nconnect("in", "b");\nset_output("b");\n'), api.last_error()
    # the numbers print as add_bandpass prints the same values
    half, m30, one, x1005, four = band.dump_calls().split('add_bandpass("b",')[1].split(")")[0].split(",")[:5]
    line = [ln for ln in dump.splitlines() if ln.startswith("add_multiband(")]
    assert len(line) == 1
    args = line[0][len("add_multiband("):-1].split(",")
    assert args == ['"g"', half, m30, one, x1005, "4000", m30, m30, "0", four, four, one, half, "50", four, "0", half, four], line
    assert " " not in line[0]


def test_project_script_records_writes_and_applies_the_call(api, tmp_path):
    p = W.ProjectScript(SR, 64)
    p.add_sum("in", 1.0, 0.0)
    p.add_multiband("g", 1.0, 0.0, 1.0, 200.0, 2000.0, [-30.0, -24.0, -18.0], (4.0, 2.0, 8.0), 5.0, 50.0, 6.0, (0.0, 3.0, -3.0))
    p.connect("in", "g")
    p.set_output("g")
    assert p.calls["add_multiband"] == [("g", 1.0, 0.0, 1.0, 200.0, 2000.0, (-30.0, -24.0, -18.0), (4.0, 2.0, 8.0), 5.0, 50.0, 6.0, (0.0, 3.0, -3.0))]
    lua = p.to_lua(str(tmp_path))
    assert 'add_multiband("g", 1.0, 0.0, 1.0, 200.0, 2000.0, -30.0, -24.0, -18.0, 4.0, 2.0, 8.0, 5.0, 50.0, 6.0, 0.0, 3.0, -3.0);' in lua
    s = api.State("", SR, 64)
    assert s.refresh(lua), api.last_error()
    q = W.multiband_project(seconds=0.5)
    assert q.output_vertex == "mb" and ("bus", "mb") in q.calls["connect"] and not q.calls["add_normalize"]
    assert 'add_multiband("mb", 1.0, 0.0, 1.0, 200.0, 2000.0, -30.0, -30.0, -30.0, 4.0, 4.0, 4.0, 5.0, 50.0, 6.0, 0.0, 0.0, 0.0);' in q.to_lua(str(tmp_path / "q"))


# ---- td_multiband_params ----
def test_multiband_params_match_the_formulas(api):
    """An independent float64 evaluation of the cookbook forms at Q = sqrt(1/2).  sin, cos and exp come from libm on both sides,
    but only correct rounding would make that a promise: a few ulp of each value, carried through the quotients: 8 ulp, of the
    value or -- for the differences -- of the terms that cancel in it."""
    worst = 0.0
    q = np.sqrt(0.5)
    for sr in MP.RATES + (8000, 192000):
        for lo, hi in MP.crossovers(sr) + ((55.5, 0.31 * sr),):
            for att, rel in MP.TIMES + ((33.3, 777.7),):
                lo32, hi32, att32, rel32 = (float(np.float32(v)) for v in (lo, hi, att, rel))
                sets, aA, aR = api.multiband_params(sr, lo, hi, (-30.0,) * 3, (4.0,) * 3, att, rel, 6.0, (0.0,) * 3)
                want = []
                for f in (lo32, hi32):
                    w0 = 2.0 * np.pi * f / sr
                    cw, alpha = np.cos(w0), np.sin(w0) / (2.0 * q)
                    a0 = 1.0 + alpha
                    omc = 2.0 * np.sin(0.5 * w0) ** 2
                    tail = (-2.0 * cw / a0, (1.0 - alpha) / a0)
                    want.append(((omc / 2.0 / a0, omc / a0, omc / 2.0 / a0) + tail, ((1.0 + cw) / 2.0 / a0, -(1.0 + cw) / a0, (1.0 + cw) / 2.0 / a0) + tail,
                                 ((1.0 - alpha) / a0, -2.0 * cw / a0, 1.0) + tail, 1.0 / a0))
                rows = (want[0][0], want[0][1], want[1][0], want[1][1], want[1][2])   # L1, H1, L2, H2, A2
                scale = (want[0][3], want[0][3], want[1][3], want[1][3], want[1][3])
                for got, w, sc in zip(sets, rows, scale):
                    for j in range(5):
                        # (a1, a2 and the numerators with 1 + cos or 1 - alpha are differences: what is left carries the ulp of
                        # the terms that cancelled, 2 / (1 + alpha) at most)
                        ulps = abs(got[j] - float(w[j])) / np.spacing(max(abs(float(w[j])), 2.0 * sc if j else abs(float(w[j])), 2.0 * sc))
                        worst = max(worst, ulps)
                        assert ulps <= 8.0, (sr, lo, hi, got, w)
                assert sets[4][1] == sets[2][3] and sets[4][0] == sets[2][4] and sets[4][3:] == sets[2][3:]   # A2 shares L2's denominator
                for got, w in ((aA, np.exp(-1.0 / (att32 * sr / 1000.0)) if att32 > 0.0 else 0.0), (aR, np.exp(-1.0 / (rel32 * sr / 1000.0)))):
                    ulps = abs(got - float(w)) / np.spacing(max(abs(float(w)), 1e-300))
                    worst = max(worst, ulps)
                    assert ulps <= 4.0, (sr, att, rel, got, w)
    print("multiband_params: worst disagreement with numpy %.3g ulp" % worst)


# ---- facts of the twin ----
def _spec(api, sr=SR, **kw):
    return MP.spec(api, sr, _args(**kw))


FLAT = dict(thr_lo=0.0, thr_mid=0.0, thr_hi=0.0, ratio_lo=1.0, ratio_mid=1.0, ratio_hi=1.0, makeup_lo=0.0, makeup_mid=0.0, makeup_hi=0.0)


def _x(n=6000, seed=5):
    return np.random.default_rng(seed).uniform(-0.5, 0.5, (n, 2)).astype(np.float32)


@pytest.mark.parametrize("sr", MP.RATES)
def test_twin_with_no_band_working_is_an_all_pass(api, sr):
    """All ratios 1 and makeup 0: G_b = 1 and p = low + mid + high, which A2 on the low band makes an all-pass of x.  | |H| - 1 | from
    a 2^17-frame impulse response, at the narrowest and the widest crossover of the range and at one in between."""
    imp = np.zeros((1 << 17, 2), np.float32)
    imp[0] = (1.0, 1.0)
    worst = 0.0
    specs = [_spec(api, sr, lo_hz=lo, hi_hz=hi, **FLAT) for lo, hi in ((40.0, 80.0), (40.0, 0.45 * sr), (200.0, 2000.0), (0.2 * sr, 0.4 * sr))]
    h, _ = NM.serial(imp, specs)
    for hs in h:
        H = np.fft.rfft(hs[:, 0])
        worst = max(worst, float(np.abs(np.abs(H) - 1.0).max()))
        assert np.array_equal(hs[:, 1], hs[:, 0])
    print("all-pass at %d Hz: | |H| - 1 | <= %.3g" % (sr, worst))
    assert worst <= 1e-9


def test_twin_splits_give_the_one_piece_result_bitwise(api):
    x = _x()
    sp = _spec(api, lo_hz=40.0, hi_hz=80.0, attack_ms=1000.0, release_ms=10000.0)
    whole, end = NM.process(x, sp, wet=0.7, gain=1.7, angle=30.0)
    for cut in (1, 777, 2048, 4999):
        a, st = NM.process(x[:cut], sp, wet=0.7, gain=1.7, angle=30.0)
        b, st = NM.process(x[cut:], sp, wet=0.7, gain=1.7, angle=30.0, state=st)
        assert np.array_equal(np.concatenate([a, b]).view(np.uint32), whole.view(np.uint32)) and np.array_equal(st, end), cut
    dry, st = NM.process(x, sp, wet=0.00009, state=end)
    assert np.array_equal(dry, x) and np.array_equal(st, end)   # dry: a Sum, the state untouched


def test_twin_a_non_finite_frame_stays_out_of_the_state(api):
    x = _x()
    sp = _spec(api)
    want, wend = NM.serial(np.where(np.arange(len(x))[:, None] == 1000, np.float32(0.0), x), sp)
    for bad in ((np.nan, 0.0), (0.0, np.inf), (-np.inf, np.nan)):
        xx = x.copy()
        xx[1000] = bad
        p, end = NM.serial(xx, sp)
        assert np.isfinite(p).all() and np.array_equal(p, want) and np.array_equal(end, wend), bad
    # ... and reaches the output through the dry leg of the lerp only
    xx = x.copy()
    xx[1000, 0] = np.nan
    out, _ = NM.process(xx, sp, wet=0.5)
    assert np.isnan(out[1000, 0]) and np.isfinite(np.delete(out, 1000, axis=0)).all()


def tone_input(n=24576, sr=SR):
    t = np.arange(n) / sr
    v = (0.25 * np.sin(2.0 * np.pi * 100.0 * t) + 0.25 * np.sin(2.0 * np.pi * 8000.0 * t)).astype(np.float32)
    return np.stack([v, v], axis=1)


def test_twin_only_the_high_band_works_on_a_two_tone_input(api):
    """Non-vacuity, measured from the spectrum: 0.25 sin 100 Hz + 0.25 sin 8 kHz through a 400 / 3 000 Hz crossover whose low and
    mid band sit at ratio 1 and whose high band compresses 4:1 above -30 dB -- the 8 kHz line falls, the 100 Hz line stays."""
    x = tone_input()
    p, _ = NM.serial(x, MP.spec(api, SR, MP.TONE_CASE))
    lo_in, hi_in = MP.tone_lines(x)
    lo_out, hi_out = MP.tone_lines(p.astype(np.float32))
    print("100 Hz line moves %.3g dB, 8 kHz line %.3f dB" % (lo_out - lo_in, hi_out - hi_in))
    assert hi_out - hi_in <= -6.0 and abs(lo_out - lo_in) < 0.1


# ---- the tiled scans restated ----
def _emulate(args):
    """One rate and input (a worker of its own: numpy only): the worst max|blocked - serial| / max|serial| of p over the specs and
    its case's index; and, to print, the same figure of the end states (against the largest state word)."""
    x, specs = args
    ser, end = NM.serial(x, specs)
    blk, endb = NM.blocked(x, specs)
    peak = np.abs(ser).max(axis=(1, 2))
    assert (peak > 0.0).all()
    r = np.abs(blk - ser).max(axis=(1, 2)) / peak
    i = int(r.argmax())
    return (float(r[i]), i), float((np.abs(endb - end).max(axis=1) / np.abs(end).max(axis=1)).max())


def test_blocked_scan_stays_inside_the_committed_constant(api):
    """E = 8 x the worst max|blocked - serial| / max|serial| of the numpy emulation over the GPU test's own grid and inputs at
    the three rates; this recomputes that worst figure and fails above E / 8."""
    jobs, what = [], []
    for sr in MP.RATES:
        cases = MP.grid_cases(sr)
        assert len(cases) == 81
        specs = [MP.spec(api, sr, c) for c in cases]
        for kind in MP.INPUTS:
            x = oracle_input(kind, sr)
            assert len(x) > 5 * NM.TILE and np.abs(x).max() > 0.05
            jobs.append((x, specs))
            what.append((cases, sr, kind))
    with multiprocessing.Pool(max(1, min(len(jobs), os.cpu_count() or 1))) as pool:
        results = pool.map(_emulate, jobs)
    worst, states, n = (0.0, None), 0.0, 0
    for (w, st), (cases, sr, kind) in zip(results, what):
        if w[0] > worst[0]:
            worst = (w[0], (cases[w[1]], sr, kind))
        states, n = max(states, st), n + len(cases)
    print("blocked scan: %d cases, worst max|blocked - serial| / max|serial| %.3g at %s (E_EMULATED %.3g, E %.3g = 2^%.1f); end states "
          "within %.3g of their largest word" % (n, worst[0], worst[1], MP.E_EMULATED, MP.E, math.log2(MP.E), states))
    assert n == 3 * 3 * 81 == 729
    assert 0.0 < worst[0] <= MP.E_EMULATED and MP.E == 8 * MP.E_EMULATED and MP.E <= 2 ** -28


def test_blocked_scan_continues_from_a_carried_state(api):
    x = oracle_input("noise", SR)[:9000]
    sp = _spec(api, lo_hz=40.0, hi_hz=80.0, attack_ms=1000.0, release_ms=10000.0)
    v, end = NM.serial(x, sp)
    for cut in (1, 777, 2048, 4999):
        a, st = NM.blocked(x[:cut], sp)
        b, st = NM.blocked(x[cut:], sp, state=st)
        assert np.abs(np.concatenate([a, b]) - v).max() <= MP.E_EMULATED * np.abs(v).max()
        assert np.abs(st - end).max() <= 2.0 ** -28 * np.abs(end).max()


def test_operator_has_the_23_blocks_and_steps_like_the_cascade(api):
    """A z + c x is one frame of the nine biquads; the blocks outside BLOCKS are exactly zero, in every power."""
    sp = _spec(api)
    A = NM.operator(sp["co"])
    mask = np.zeros((18, 18), bool)
    for r, c in NM.BLOCKS:
        mask[2 * r:2 * r + 2, 2 * c:2 * c + 2] = True
    assert int(mask.sum()) == 23 * 4 and not A[~mask].any() and not NM._power(A, 2048)[~mask].any()
    rng = np.random.default_rng(3)
    z0 = rng.uniform(-1, 1, 18)
    co = [[sp["co"][s, i] for i in range(5)] for s in range(5)]
    z = list(z0)
    NM._frame(co, z, 0.37)
    zero = [0.0] * 18
    NM._frame(co, zero, 1.0)
    assert np.allclose(np.array(z), (A.astype(np.float64) @ z0) + 0.37 * np.array(zero), rtol=0, atol=1e-14)


# ---- the host engine under sanitizers ----
@pytest.fixture(scope="module")
def asan_exe(tmp_path_factory):
    return fx_rig.asan_exe(tmp_path_factory, "asan_multiband", ["mock_guard.cpp", "mock_multiband.cpp", "asan_fx.cpp"])


MB_LAUNCHES = ("k_mb_local", "k_mb_carry", "k_mb_detect", "k_mb_carry_y1", "k_mb_env", "k_mb_carry_yl", "k_mb_apply")


def test_random_multiband_projects_hold_one_to_three_multibands():
    wet = 0
    for seed in range(16):
        p = MP.random_multiband_project(seed)
        assert 1 <= len(p.calls["add_multiband"]) <= 3
        wet += sum(1 for c in p.calls["add_multiband"] if c[3] >= 0.0001)
    assert wet >= 12


def test_multiband_projects_under_sanitizers(asan_exe, tmp_path):
    n = int(os.environ.get("TD_ASAN_MULTIBAND_SEEDS", "32"))
    workers = max(1, min(8, os.cpu_count() or 1))
    seeds = list(range(n))
    base = str(tmp_path / "p")
    with multiprocessing.Pool(workers) as pool:
        lists = pool.map(MP.write_projects, [(base, seeds[i::workers]) for i in range(workers) if seeds[i::workers]])
    procs = [subprocess.Popen([asan_exe] + lst, env=dict(os.environ, **ENV), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for lst in lists]
    tot = dict(apply=0, vertices=0, single=0, fresh=0, carried=0, local=0, rejected=0, restarts=0, short=0, env=0)
    for p in procs:
        out, err = p.communicate(timeout=1800)
        assert p.returncode == 0, (out[-800:], err[-4000:])
        tail = out.split("asan_multiband done:")[1]
        tot["apply"] += int(tail.split("k_mb_apply descriptors ")[1].split()[0])
        tot["vertices"] += int(tail.split("(")[1].split()[0])
        tot["single"] += int(tail.split(" one-launch")[0].split()[-1])
        tot["fresh"] += int(tail.split(" entered fresh")[0].split()[-1])
        tot["carried"] += int(tail.split(" entered with the line")[0].split()[-1])
        tot["local"] += int(tail.split(" k_mb_local descriptors")[0].split()[-1])
        tot["env"] += int(tail.split(" k_comp_env descriptors")[0].split()[-1])
        tot["restarts"] += int(tail.split(" restarts checked")[0].split()[-1])
        tot["short"] += int(tail.split(" short chunks")[0].split()[-1])
        tot["rejected"] += int(tail.split(" rejected refreshes")[0].split()[-1])
    # whole renders and 4 096-frame chunks take seven launches, block pulls one; chunks and pulls enter with the line; the band
    # detectors run three descriptors per vertex
    assert tot["rejected"] == 0 and tot["apply"] >= n // 2 and tot["vertices"] == tot["apply"], tot
    assert tot["fresh"] > 0 and tot["carried"] > 0 and tot["single"] > 0 and 0 < tot["local"] < tot["apply"] and tot["env"] == 3 * tot["local"], tot
    assert tot["restarts"] > 0 and tot["short"] > 0, tot
    print("asan_multiband: %d projects clean: %s" % (n, tot))


MB = MP.case(200.0, 2000.0, MP.BAND_SETTINGS[0], 6.0, (5.0, 50.0))


def _guard_project(shape, seconds=0.5):
    """The guard's shapes: `b` / `y` is what the guard would speed up (a band-pass under band_mode 2, a synth under sine_mode 2)."""
    p = W.ProjectScript(SR, 1024)
    p.set_length(seconds)
    p.assets["a"] = W.Asset(W.noise_int16(7, 9000))
    p.load_sample("a", "a", "")
    p.event_files["f"] = np.array([(0.01, 60.0, 0.8), (0.2, 60.0, 0.0), (0.25, 62.0, 0.6)], np.float32)
    p.load_midi_floww("f", "f")
    wet = 0.0 if shape.endswith("_dry") else 1.0
    if shape in ("in_up", "in_dry", "in_plain"):      # loop -> band-pass -> multiband | dry multiband | Sum
        p.add_sampleloop("s", 1.0, 0.0, "a")
        p.add_bandpass("b", 1.0, 0.0, 1.0, 300.0, 5000.0, True)
        if shape == "in_plain":
            p.add_sum("c", 1.0, 0.0)
        else:
            p.add_multiband("c", 1.0, 0.0, wet, *MB)
        p.connect("s", "b"); p.connect("b", "c")
        p.set_output("c")
    elif shape == "down":                            # loop -> multiband -> band-pass
        p.add_sampleloop("s", 1.0, 0.0, "a")
        p.add_multiband("c", 1.0, 0.0, 1.0, *MB)
        p.add_bandpass("b", 1.0, 0.0, 1.0, 300.0, 5000.0, True)
        p.connect("s", "c"); p.connect("c", "b"); p.set_output("b")
    elif shape in ("sine_up", "one_tile", "level"):  # synth -> multiband (one_tile: a render of 2 048 frames)
        p.add_synth("y", 1.0, 0.0, "f", 0.4, 0.3, W.HIT_ADSR, 1.0, 0.8, W.NOTE_ADSR, 0.5, W.STD_ADSR)
        p.add_multiband("c", 1.0, 0.0, 1.0, *MB)
        p.connect("y", "c")
        if shape == "level":     # ... and two more in the same level
            p.add_multiband("c2", 1.0, 0.0, 1.0, *MP.case(40.0, 80.0, MP.BAND_SETTINGS[1], 0.0, (0.0, 1.0)))
            p.add_multiband("c3", 1.0, 0.0, 0.5, *MP.case(1000.0, 21600.0, MP.BAND_SETTINGS[2], 40.0, (1000.0, 10000.0)))
            p.add_sum("m", 1.0, 0.0)
            for v in ("c2", "c3"):
                p.connect("y", v)
            for v in ("c", "c2", "c3"):
                p.connect(v, "m")
        p.set_output("m" if shape == "level" else "c")
    else:                        # synth -> sum: the control
        p.add_synth("y", 1.0, 0.0, "f", 0.4, 0.3, W.HIT_ADSR, 1.0, 0.8, W.NOTE_ADSR, 0.5, W.STD_ADSR)
        p.add_sum("c", 1.0, 0.0)
        p.connect("y", "c"); p.set_output("c")
    return p


def test_guard_modes_keep_the_exact_forms_upstream_of_a_multiband(asan_exe, tmp_path):
    """band_mode 2 / sine_mode 2 (the driver's profiled render): the launch families each shape went through."""
    shapes = ("in_up", "in_dry", "in_plain", "down", "sine_up", "sine_free", "level")
    projects = {s: _guard_project(s) for s in shapes}
    projects["one_tile"] = _guard_project("one_tile", seconds=0.04)
    assert projects["one_tile"].cs * 1024 == NM.TILE
    fams = _families(asan_exe, tmp_path, projects)
    exact = ("k_band_pass", "k_band_spec")
    # upstream of a multiband that is not dry: the exact forms
    f = fams["in_up"]
    assert "k_band_scan" not in f and any(k in f for k in exact), f
    assert [(k, v) for k, v in f.items() if k.startswith("k_mb")] == [(k, 1) for k in MB_LAUNCHES], f   # (and in this order)
    # downstream of it the guard is free
    down = fams["down"]
    assert "k_band_scan" in down and not any(k in down for k in exact), down
    # wet < 0.0001 compiles to k_sum and changes nothing upstream: the launch list of the project with a Sum in its place
    assert not any(k.startswith("k_mb") for k in fams["in_dry"]) and "k_band_scan" in fams["in_dry"], fams["in_dry"]
    assert fams["in_dry"] == fams["in_plain"], (fams["in_dry"], fams["in_plain"])
    sup, sfree = fams["sine_up"], fams["sine_free"]
    assert "k_sine_probe" not in sup and "k_synth" in sup, sup
    assert "k_sine_probe" in sfree and not any(k.startswith("k_mb") for k in sfree), sfree
    # a chunk of one tile is k_mb_apply alone; three vertices in one level take each step once
    assert [(k, v) for k, v in fams["one_tile"].items() if k.startswith("k_mb")] == [("k_mb_apply", 1)], fams["one_tile"]
    assert [(k, v) for k, v in fams["level"].items() if k.startswith("k_mb")] == [(k, 1) for k in MB_LAUNCHES], fams["level"]


def test_projects_without_a_multiband_keep_their_launch_list(asan_exe, tmp_path):
    projects = {"drums": W.drum_project(seconds=0.5), "config2": W.config2(seconds=0.5, n_src=8), "config4": W.config4(seconds=0.5, depth=6)}
    fams = _families(asan_exe, tmp_path, projects)
    for name in projects:
        got = " ".join("%s=%d" % kv for kv in fams[name].items())
        assert not any(k.startswith("k_mb") for k in fams[name]) and got == PARENT_LAUNCHES[name], (name, got)
