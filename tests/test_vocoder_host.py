"""The vocoder vertex on the host, no GPU (include/termdaw_amd.h td_graph_add_vocoder): parameter ranges rejected
with messages that name the parameter, through the C ABI and through the Lua front-end (NaN and the infinities included); key
edges into a vocoder (and still none into an EQ), loops over both kinds of edge, td_graph_reset; the canonical dump line;
td_vocoder_params against numpy's evaluation of the formulas; facts of the float64 twin (tests/np_vocoder.py) that can be derived
by hand; the tiled scans restated in numpy (np_vocoder.blocked, the kernels' tile geometry and join order) against the serial
loop, within the bound's constant, which this file derives; the host engine on random projects with vocoder vertices under
AddressSanitizer / UBSan (a stand-alone program: tests/asan_fx.cpp as it is, against tests/mock_hip.cpp + tests/mock_guard.cpp +
tests/mock_vocoder.cpp, whose mock launches check every descriptor); and the guard rule and the launch lists, read from the launch
families the mock build reports."""
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
import np_vocoder as NV  # noqa: E402
import vocoder_projects as VP  # noqa: E402
from fx_rig import ENV, PARENT_LAUNCHES, _families, oracle_input  # noqa: E402
SR = 48000

GOOD = dict(bands=8, lo_hz=200.0, hi_hz=4000.0, q=4.0, response_ms=10.0, out_db=12.0)
ORDER = ["bands", "lo_hz", "hi_hz", "q", "response_ms", "out_db"]
RANGES = dict(lo_hz=(40.0, None), hi_hz=(None, 0.45 * SR), q=(0.5, 20.0), response_ms=(0.1, 1000.0), out_db=(-24.0, 48.0))
NON_FINITE = (float("nan"), float("inf"), float("-inf"))


def _below(v):
    return float(np.nextafter(np.float32(v), np.float32(-1e9)))


def _above(v):
    return float(np.nextafter(np.float32(v), np.float32(1e9)))


BAD = [(k, _below(lo)) for k, (lo, hi) in RANGES.items() if lo is not None] + [(k, _above(hi)) for k, (lo, hi) in RANGES.items() if hi is not None]
BAD += [(k, v) for k in RANGES for v in NON_FINITE]
BAD += [("bands", v) for v in (0, 1, 2, 3, 5, 12, 15, 17, 32, -4)]
BAD += [("lo_hz", 4000.0), ("lo_hz", 4000.5), ("hi_hz", 200.0), ("hi_hz", 199.5)]   # lo_hz < hi_hz: the message names both


def _args(**kw):
    return fx_rig._args(GOOD, ORDER, **kw)


# ---- ranges, key edges, the Lua line, the project script ----
@pytest.mark.parametrize("name,value", BAD)
def test_out_of_range_parameters_are_rejected_by_name(api, name, value):
    fx_rig.out_of_range_is_rejected_by_name(api, SR, lambda g, *a: g.add_vocoder("v", 1.0, 0.0, 1.0, *a), api.vocoder_params, _args(**{name: value}), name)


def test_range_ends_are_accepted_and_follow_the_rate(api):
    g = api.Graph(64, SR)
    g.add_sum("in", 1.0, 0.0)
    ends = [(4, 40.0, 0.45 * SR, 0.5, 0.1, -24.0), (16, 40.0, _above(40.0), 20.0, 1000.0, 48.0), (8, _below(0.45 * SR), 0.45 * SR, 4.0, 10.0, 0.0)]
    for i, c in enumerate(ends):
        g.add_vocoder("v%d" % i, 1.0, 0.0, 1.0, *c)
        assert g.connect("in", "v%d" % i)
    g.add_vocoder("wet", 1.0, 0.0, 7.0, *_args())   # (wet is clamped, not rejected: graph.rs:256)
    g.add_vocoder("dry", 1.0, 0.0, -3.0, *_args())
    assert g.set_output("v1") and g.check_graph()
    for sr in (44100, 96000):   # hi_hz's end is 0.45 of the graph's own rate
        h = api.Graph(64, sr)
        h.add_vocoder("p", 1.0, 0.0, 1.0, *_args(hi_hz=0.45 * sr))
        with pytest.raises(api.TermdawError, match="hi_hz"):
            h.add_vocoder("q", 1.0, 0.0, 1.0, *_args(hi_hz=_above(0.45 * sr)))


def test_vocoder_params_needs_room_for_every_band(api):
    import ctypes
    out = (ctypes.c_double * 98)()
    assert api.lib().td_vocoder_params(SR, 16, 200.0, 4000.0, 4.0, 10.0, 0.0, out, 98) == 1
    assert api.lib().td_vocoder_params(SR, 16, 200.0, 4000.0, 4.0, 10.0, 0.0, out, 97) == 0 and "vocoder_params" in api.last_error()
    assert api.lib().td_vocoder_params(SR, 4, 200.0, 4000.0, 4.0, 10.0, 0.0, out, 26) == 1


def _keyed_graph(api):
    g = api.Graph(64, SR)
    g.add_sum("a", 1.0, 0.0)
    g.add_sum("b", 1.0, 0.0)
    g.add_vocoder("v", 1.0, 0.0, 1.0, *_args())
    g.add_eq("eq", 1.0, 0.0, 1.0, "peak", 900.0, 2.5, 9.0)
    return g


def test_a_vocoder_takes_a_key_and_an_eq_still_does_not(api):
    g = _keyed_graph(api)
    assert g.connect_key("a", "v") and g.connect_key("b", "v") and g.connect_key("a", "v"), api.last_error()   # (a duplicate is an edge of its own)
    assert g.connect_key("eq", "v"), api.last_error()   # any vertex may BE the key
    assert not g.connect_key("a", "eq") and api.last_error() == "connect_key: eq takes no key input"
    assert not g.connect_key("a", "b") and api.last_error() == "connect_key: b takes no key input"
    assert not g.connect_key("nope", "v") and "cannot be found" in api.last_error()


def test_loops_are_found_over_input_and_key_edges_together(api):
    g = _keyed_graph(api)
    assert g.connect("v", "a")   # v -> a (input); a -> v as a key would close the loop
    assert not g.connect_key("a", "v") and api.last_error() == "connect_key: edge would close a loop"
    assert not g.connect_key("v", "v") and "connect_key" in api.last_error()
    assert g.connect_key("b", "v")   # b -> v (key); v -> b as an input would close the loop
    assert not g.connect("v", "b") and api.last_error() == "connect: edge would close a loop"
    assert g.connect("a", "eq") and not g.connect_key("eq", "v") and api.last_error() == "connect_key: edge would close a loop"


def test_reset_clears_vocoders_and_their_key_edges(api):
    g = _keyed_graph(api)
    assert g.connect("v", "a") and not g.connect_key("a", "v") and g.connect_key("b", "v")
    api.lib().td_graph_reset(g.h)
    assert not g.connect_key("b", "v") and "cannot be found" in api.last_error()   # (the vertex is gone)
    g.add_sum("a", 1.0, 0.0)
    g.add_sum("b", 1.0, 0.0)
    g.add_vocoder("v", 1.0, 0.0, 1.0, *_args())
    # the edges of before are gone: what was a loop then is none now, in either kind
    assert g.connect_key("a", "v"), api.last_error()
    assert g.connect("v", "b"), api.last_error()


def _lua(line):
    return fx_rig._lua(line, "g", key="k")


def _lit(v):
    if isinstance(v, int):
        return str(v)
    if math.isnan(v):
        return "0/0"
    if math.isinf(v):
        return "1/0" if v > 0 else "-1/0"
    return repr(float(v))


@pytest.mark.parametrize("name,value", BAD)
def test_lua_rejects_the_same_ranges(api, name, value):
    s = api.State("", SR, 64)
    line = 'add_vocoder("g", 1.0, 0.0, 1.0, %s);' % ", ".join(_lit(v) for v in _args(**{name: value}))
    assert not s.refresh(_lua(line))
    assert name in api.last_error(), api.last_error()


def test_lua_accepts_and_dumps_the_canonical_line(api):
    s = api.State("", SR, 64)
    assert s.refresh(_lua('add_vocoder("g", 0.5, -30, 1, 4, 100.5, 4000, 4, 0.5, 0.5);')), api.last_error()
    dump = s.dump_calls()
    band = api.State("", SR, 64)
    assert band.refresh('add_sum("in", 1.0, 0.0);\nadd_bandpass("b", 0.5, -30, 1, 100.5, 4, true);\nconnect("in", "b");\nset_output("b");\n'), api.last_error()
    # the numbers print as add_bandpass prints the same values
    half, m30, one, x1005, four = band.dump_calls().split('add_bandpass("b",')[1].split(")")[0].split(",")[:5]
    line = [ln for ln in dump.splitlines() if ln.startswith("add_vocoder(")]
    assert len(line) == 1
    args = line[0][len("add_vocoder("):-1].split(",")
    assert args[0] == '"g"' and args[1] == half and args[2] == m30 and args[3] == one and args[4] == "4" and args[5] == x1005, line
    assert args[7] == four and args[8] == half and args[9] == half and len(args) == 10 and " " not in line[0]
    assert 'connect_key("k","g")' in dump


def test_project_script_records_writes_and_applies_the_call(api, tmp_path):
    p = W.ProjectScript(SR, 64)
    p.add_sum("in", 1.0, 0.0)
    p.add_sum("k", 1.0, 0.0)
    p.add_vocoder("g", 1.0, 0.0, 1.0, 8, 200.0, 4000.0, 4.0, 10.0, 12.0)
    p.connect("in", "g")
    p.connect_key("k", "g")
    p.set_output("g")
    assert p.calls["add_vocoder"] == [("g", 1.0, 0.0, 1.0, 8, 200.0, 4000.0, 4.0, 10.0, 12.0)]
    lua = p.to_lua(str(tmp_path))
    assert 'add_vocoder("g", 1.0, 0.0, 1.0, 8, 200.0, 4000.0, 4.0, 10.0, 12.0);' in lua
    s = api.State("", SR, 64)
    assert s.refresh(lua), api.last_error()
    assert W.vocoder_project(seconds=0.5).calls["add_vocoder"][0][4] == 16


# ---- td_vocoder_params ----
def test_vocoder_params_match_the_formulas(api):
    """An independent float64 evaluation: f_b by numpy's power, the cookbook band-pass by np_eq.cookbook's formulas at f_b (here
    without the rounding of the frequency to float32 that the EQ vertex' parameter has), a and g by exp and power.  pow, sin, cos
    and exp come from libm on both sides, but only correct rounding would make that a promise: a few ulp of each value, carried
    through the quotients: 8 ulp, of the value or -- for the two differences a1 and a2 -- of the terms that cancel in it."""
    worst = 0.0
    for sr in VP.RATES + (8000, 192000):
        for c in VP.grid_cases(sr) + [(8, 55.5, 0.31 * sr, 3.3, 33.3, -7.7)]:
            if c[2] > 0.45 * sr:
                continue
            B, lo, hi, q, ms, db = c[0], *(float(np.float32(v)) for v in c[1:])
            rows, a, g = api.vocoder_params(sr, *c)
            assert len(rows) == B
            for b, row in enumerate(rows):
                f = lo * np.power(hi / lo, b / (B - 1.0))
                w0 = 2.0 * np.pi * f / sr
                alpha = np.sin(w0) / (2.0 * q)
                want = (f, alpha / (1.0 + alpha), 0.0, -alpha / (1.0 + alpha), -2.0 * np.cos(w0) / (1.0 + alpha), (1.0 - alpha) / (1.0 + alpha))
                # (a1 and a2 are differences: near w0 = pi / 2 the cosine, near alpha = 1 the numerator 1 - alpha cancel, and what is
                # left carries the ulp of the terms that cancelled, 2 / (1 + alpha) and 1 / (1 + alpha))
                scales = (f, want[1], 1.0, want[1], 2.0 / (1.0 + alpha), 1.0 / (1.0 + alpha))
                for got, w, sc in zip(row, want, scales):
                    ulps = abs(got - float(w)) / np.spacing(max(abs(float(w)), float(sc)))
                    worst = max(worst, ulps)
                    assert ulps <= 8.0, (sr, c, b, row, want)
                assert row[2] == 0.0 and row[3] == -row[1]
            assert rows[0][0] == lo and abs(rows[-1][0] - hi) <= 4 * np.spacing(hi)
            for got, w in ((a, np.exp(-1.0 / (ms * sr / 1000.0))), (g, np.power(10.0, db / 20.0))):
                ulps = abs(got - float(w)) / np.spacing(abs(float(w)))
                worst = max(worst, ulps)
                assert ulps <= 4.0, (sr, c, got, w)
    print("vocoder_params: worst disagreement with numpy %.3g ulp" % worst)


# ---- facts of the twin ----
def _spec(api, **kw):
    return NV.spec(api.vocoder_params(SR, *_args(**kw)))


def _xk(n=6000, seed=5):
    rng = np.random.default_rng(seed)
    x = rng.uniform(-0.5, 0.5, (n, 2)).astype(np.float32)
    k = np.zeros((n, 2), np.float32)
    k[500:3500] = (rng.uniform(-0.5, 0.5, (3000, 2)) * np.hanning(3000)[:, None]).astype(np.float32)
    return x, k


def test_twin_key_equal_to_the_input_is_the_unkeyed_result_bitwise(api):
    x, _ = _xk()
    for bands in (4, 8, 16):
        sp = _spec(api, bands=bands)
        a, ea = NV.process(x, x.copy(), sp, wet=0.7, gain=1.7, angle=30.0)
        b, eb = NV.process(x, None, sp, wet=0.7, gain=1.7, angle=30.0)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) and np.array_equal(ea, eb)


def test_twin_splits_give_the_one_piece_result_bitwise(api):
    x, k = _xk()
    sp = _spec(api, bands=16, q=20.0, response_ms=1000.0)
    whole, end = NV.process(x, k, sp, wet=0.7, gain=1.7, angle=30.0)
    for cut in (1, 777, 2048, 4999):
        a, st = NV.process(x[:cut], k[:cut], sp, wet=0.7, gain=1.7, angle=30.0)
        b, st = NV.process(x[cut:], k[cut:], sp, wet=0.7, gain=1.7, angle=30.0, state=st)
        assert np.array_equal(np.concatenate([a, b]).view(np.uint32), whole.view(np.uint32)) and np.array_equal(st, end), cut


def test_twin_a_silent_modulator_gives_exactly_zero(api):
    x, k = _xk()
    p, end = NV.serial(x, np.zeros_like(k), _spec(api))
    assert not p.any() and not end[:, 4:].any() and end[:, :4].any()   # (the carrier's filters run all the same)
    out, _ = NV.process(x, np.zeros_like(k), _spec(api), wet=0.25)
    assert np.array_equal(out, x + np.float32(0.25) * (np.float32(0.0) - x))   # the dry lerp of zero


def test_twin_a_non_finite_modulator_frame_stays_out_of_the_state(api):
    x, k = _xk()
    sp = _spec(api)
    want, wend = NV.serial(x, np.where(np.arange(len(k))[:, None] == 1000, np.float32(0.0), k), sp)
    for bad in ((np.nan, 0.1), (0.1, np.inf), (-np.inf, np.nan)):
        kk = k.copy()
        kk[1000] = bad
        p, end = NV.serial(x, kk, sp)
        assert np.isfinite(p).all() and np.array_equal(p, want) and np.array_equal(end, wend), bad
    # ... whereas a non-finite CARRIER sample enters its filter as 0 and reaches the output through the dry leg of the lerp only
    xx = x.copy()
    xx[1000, 0] = np.nan
    p, _ = NV.serial(xx, k, sp)
    assert np.isfinite(p).all()
    out, _ = NV.process(xx, k, sp, wet=0.5)
    assert np.isnan(out[1000, 0]) and np.isfinite(np.delete(out, 1000, axis=0)).all()


def test_twin_a_key_tone_opens_its_own_band(api):
    """White-noise carrier, a sine at band 2's centre as key: band 2's follower is the largest by far."""
    rng = np.random.default_rng(9)
    n = 12000
    sp = _spec(api, bands=8, q=8.0)
    tone = (0.5 * np.sin(2.0 * np.pi * sp["f"][2] * np.arange(n) / SR)).astype(np.float32)
    _, end = NV.serial(rng.uniform(-0.5, 0.5, (n, 2)).astype(np.float32), np.stack([tone, tone], axis=1), sp)
    e = end[:, 6]
    assert e.argmax() == 2 and e[2] > 4.0 * np.delete(e, 2).max(), e


# ---- the tiled scans restated ----
def _emulate(args):
    """One rate and pair of inputs (a worker of its own: numpy only): the worst max|blocked - serial| / max|serial| of p over the
    specs and its case's index; and, to print, the same figure of the end states (against the largest state word: the biquads'
    (s1, s2) cancel in y near z = 1 and are conditioned worse than p, which is what the bound is on)."""
    x, k, specs = args
    worst, states = (0.0, -1), 0.0
    for B in VP.BANDS:
        idx = [i for i, s in enumerate(specs) if s["B"] == B]
        ser, end = NV.serial(x, k, [specs[i] for i in idx])
        for j, i in enumerate(idx):
            blk, endb = NV.blocked(x, k, specs[i])
            worst = max(worst, (float(np.abs(blk - ser[j]).max() / np.abs(ser[j]).max()), i))
            states = max(states, float(np.abs(endb - end[j]).max() / np.abs(end[j]).max()))
    return worst, states


def test_blocked_scan_stays_inside_the_committed_constant(api):
    """E = 8 x the worst max|blocked - serial| / max|serial| of the numpy emulation over the GPU test's own grid and inputs at
    the three rates; this recomputes that worst figure and fails above E / 8."""
    jobs, what = [], []
    for sr in VP.RATES:
        cases = VP.grid_cases(sr)
        assert len(cases) == 81
        specs = [VP.spec(api, sr, c) for c in cases]
        for car, key in VP.PAIRS:
            x, k = oracle_input(car, sr), oracle_input(key, sr)
            assert len(x) == len(k) and len(x) > 5 * NV.TILE and min(np.abs(x).max(), np.abs(k).max()) > 0.05
            jobs.append((x, k, specs))
            what.append((cases, sr, car, key))
    with multiprocessing.Pool(max(1, min(len(jobs), os.cpu_count() or 1))) as pool:
        results = pool.map(_emulate, jobs)
    worst, states, n = (0.0, None), 0.0, 0
    for (w, st), (cases, sr, car, key) in zip(results, what):
        if w[0] > worst[0]:
            worst = (w[0], (cases[w[1]], sr, car, key))
        states, n = max(states, st), n + len(cases)
    print("blocked scan: %d cases, worst max|blocked - serial| / max|serial| %.3g at %s (E_EMULATED %.3g, E %.3g = 2^%.1f); end states "
          "within %.3g of their largest word" % (n, worst[0], worst[1], VP.E_EMULATED, VP.E, math.log2(VP.E), states))
    assert n == 3 * 3 * 81
    assert 0.0 < worst[0] <= VP.E_EMULATED and VP.E == 8 * VP.E_EMULATED and VP.E <= 2 ** -28


def test_blocked_scan_continues_from_a_carried_state(api):
    x, k = oracle_input("noise", SR)[:9000], oracle_input("drums", SR)[:9000]
    sp = _spec(api, bands=16, lo_hz=40.0, hi_hz=0.45 * SR, q=20.0, response_ms=1000.0)
    v, end = NV.serial(x, k, sp)
    for cut in (1, 777, 2048, 4999):
        a, st = NV.blocked(x[:cut], k[:cut], sp)
        b, st = NV.blocked(x[cut:], k[cut:], sp, state=st)
        assert np.abs(np.concatenate([a, b]) - v).max() <= VP.E_EMULATED * np.abs(v).max()
        assert np.abs(st - end).max() <= 2.0 ** -28 * np.abs(end).max()   # (the states are conditioned worse than p: see _emulate)


# ---- the host engine under sanitizers ----
@pytest.fixture(scope="module")
def asan_exe(tmp_path_factory):
    return fx_rig.asan_exe(tmp_path_factory, "asan_vocoder", ["mock_guard.cpp", "mock_vocoder.cpp", "asan_fx.cpp"])


VOC_LAUNCHES = ("k_voc_local", "k_voc_carry_z", "k_voc_env", "k_voc_carry_env", "k_voc_apply")


def test_random_vocoder_projects_hold_one_to_three_vocoders_and_keys():
    keyed = 0
    for seed in range(16):
        p = VP.random_vocoder_project(seed)
        assert 1 <= len(p.calls["add_vocoder"]) <= 3
        keyed += len(p.calls["connect_key"])
    assert keyed >= 8


def test_vocoder_projects_under_sanitizers(asan_exe, tmp_path):
    n = int(os.environ.get("TD_ASAN_VOCODER_SEEDS", "32"))
    workers = max(1, min(8, os.cpu_count() or 1))
    seeds = list(range(n))
    base = str(tmp_path / "p")
    with multiprocessing.Pool(workers) as pool:
        lists = pool.map(VP.write_projects, [(base, seeds[i::workers]) for i in range(workers) if seeds[i::workers]])
    procs = [subprocess.Popen([asan_exe] + lst, env=dict(os.environ, **ENV), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for lst in lists]
    tot = dict(apply=0, vertices=0, single=0, fresh=0, carried=0, local=0, rejected=0, restarts=0, short=0, keyed=0, keyed_single=0)
    for p in procs:
        out, err = p.communicate(timeout=1800)
        assert p.returncode == 0, (out[-800:], err[-4000:])
        tail = out.split("asan_vocoder done:")[1]
        tot["apply"] += int(tail.split("k_voc_apply descriptors ")[1].split()[0])
        tot["vertices"] += int(tail.split("(")[1].split()[0])
        tot["single"] += int(tail.split(" one-launch")[0].split()[-1])
        tot["fresh"] += int(tail.split(" entered fresh")[0].split()[-1])
        tot["carried"] += int(tail.split(" entered with the line")[0].split()[-1])
        tot["local"] += int(tail.split(" k_voc_local descriptors")[0].split()[-1])
        tot["restarts"] += int(tail.split(" restarts checked")[0].split()[-1])
        tot["short"] += int(tail.split(" short chunks")[0].split()[-1])
        tot["rejected"] += int(tail.split(" rejected refreshes")[0].split()[-1])
        kd = out.split("mock_vocoder: ")[1]
        tot["keyed"] += int(kd.split()[0])
        tot["keyed_single"] += int(kd.split("descriptors, ")[1].split()[0])
    # whole renders and 4 096-frame chunks take five launches, block pulls one; chunks and pulls enter with the line; keyed
    # vertices occur in both forms (the mock aborts where one goes through an entry point of the other kind)
    assert tot["rejected"] == 0 and tot["apply"] >= n // 2 and tot["vertices"] == tot["apply"], tot
    assert tot["fresh"] > 0 and tot["carried"] > 0 and tot["single"] > 0 and 0 < tot["local"] < tot["apply"], tot
    assert tot["restarts"] > 0 and tot["short"] > 0 and tot["keyed"] > tot["keyed_single"] > 0, tot
    print("asan_vocoder: %d projects clean: %s" % (n, tot))


VOC = (8, 200.0, 4000.0, 4.0, 10.0, 12.0)


def _guard_project(shape, seconds=0.5):
    """The guard's shapes: `b` / `y` is what the guard would speed up (a band-pass under band_mode 2, a synth under sine_mode 2)."""
    p = W.ProjectScript(SR, 1024)
    p.set_length(seconds)
    p.assets["a"] = W.Asset(W.noise_int16(7, 9000))
    p.assets["a2"] = W.Asset(W.noise_int16(8, 9001))
    p.load_sample("a", "a", "")
    p.load_sample("a2", "a2", "")
    p.event_files["f"] = np.array([(0.01, 60.0, 0.8), (0.2, 60.0, 0.0), (0.25, 62.0, 0.6)], np.float32)
    p.load_midi_floww("f", "f")
    wet = 0.0 if shape.endswith("_dry") else 1.0
    if shape in ("in_up", "in_dry", "in_plain"):      # loop -> band-pass -> vocoder | dry vocoder | Sum; a second loop as key
        p.add_sampleloop("s", 1.0, 0.0, "a")
        p.add_sampleloop("k", 1.0, 0.0, "a2")
        p.add_bandpass("b", 1.0, 0.0, 1.0, 300.0, 5000.0, True)
        if shape == "in_plain":
            p.add_sum("c", 1.0, 0.0)
        else:
            p.add_vocoder("c", 1.0, 0.0, wet, *VOC)
        p.connect("s", "b"); p.connect("b", "c")
        if shape != "in_plain":
            p.connect_key("k", "c")
        p.set_output("c")
    elif shape in ("key_up", "key_dry", "key_plain"):   # loop -> vocoder, keyed by loop -> band-pass (dry: the key is ignored, but rendered)
        p.add_sampleloop("s", 1.0, 0.0, "a")
        p.add_sampleloop("k", 1.0, 0.0, "a2")
        p.add_bandpass("b", 1.0, 0.0, 1.0, 300.0, 5000.0, True)
        p.add_vocoder("c", 1.0, 0.0, wet, *VOC)
        p.add_sum("m", 1.0, 0.0)
        p.connect("k", "b"); p.connect("s", "c")
        if shape != "key_plain":
            p.connect_key("b", "c")
        p.connect("c", "m"); p.connect("b", "m")
        p.set_output("m")
    elif shape == "down":                            # loop -> vocoder -> band-pass
        p.add_sampleloop("s", 1.0, 0.0, "a")
        p.add_vocoder("c", 1.0, 0.0, 1.0, *VOC)
        p.add_bandpass("b", 1.0, 0.0, 1.0, 300.0, 5000.0, True)
        p.connect("s", "c"); p.connect("c", "b"); p.set_output("b")
    elif shape in ("sine_up", "one_tile", "mixed"):  # synth -> vocoder (one_tile: a render of 2 048 frames)
        p.add_synth("y", 1.0, 0.0, "f", 0.4, 0.3, W.HIT_ADSR, 1.0, 0.8, W.NOTE_ADSR, 0.5, W.STD_ADSR)
        p.add_sampleloop("k", 1.0, 0.0, "a2")
        p.add_vocoder("c", 1.0, 0.0, 1.0, *VOC)
        p.connect("y", "c")
        if shape == "mixed":     # ... and three more in the same level: another band count, and two keyed ones of the two counts
            p.add_vocoder("c16", 1.0, 0.0, 1.0, 16, 200.0, 4000.0, 4.0, 10.0, 12.0)
            p.add_vocoder("k8", 1.0, 0.0, 1.0, *VOC)
            p.add_vocoder("k16", 1.0, 0.0, 1.0, 16, 100.0, 8000.0, 2.0, 1.0, 0.0)
            p.add_sum("m", 1.0, 0.0)
            for v in ("c16", "k8", "k16"):
                p.connect("y", v)
            p.connect_key("k", "k8"); p.connect_key("k", "k16")
            for v in ("c", "c16", "k8", "k16"):
                p.connect(v, "m")
        elif shape == "one_tile":
            p.connect_key("k", "c")
        p.set_output("m" if shape == "mixed" else "c")
    else:                        # synth -> sum: the control
        p.add_synth("y", 1.0, 0.0, "f", 0.4, 0.3, W.HIT_ADSR, 1.0, 0.8, W.NOTE_ADSR, 0.5, W.STD_ADSR)
        p.add_sum("c", 1.0, 0.0)
        p.connect("y", "c"); p.set_output("c")
    return p


def test_guard_modes_keep_the_exact_forms_upstream_of_a_vocoder(asan_exe, tmp_path):
    """band_mode 2 / sine_mode 2 (the driver's profiled render): the launch families each shape went through."""
    shapes = ("in_up", "in_dry", "in_plain", "key_up", "key_dry", "key_plain", "down", "sine_up", "sine_free", "mixed")
    projects = {s: _guard_project(s) for s in shapes}
    projects["one_tile"] = _guard_project("one_tile", seconds=0.04)
    assert projects["one_tile"].cs * 1024 == NV.TILE
    fams = _families(asan_exe, tmp_path, projects)
    exact = ("k_band_pass", "k_band_spec")
    # upstream of the input and upstream of the key of a vocoder that is not dry: the exact forms
    for name in ("in_up", "key_up"):
        f = fams[name]
        assert "k_band_scan" not in f and any(k in f for k in exact), (name, f)
        assert [(k, v) for k, v in f.items() if k.startswith("k_voc")] == [(k, 1) for k in VOC_LAUNCHES], (name, f)   # (and in this order)
    # downstream of it the guard is free
    down = fams["down"]
    assert "k_band_scan" in down and not any(k in down for k in exact), down
    # wet < 0.0001 compiles to k_sum and changes nothing upstream: the launch list of the project with a Sum in the vocoder's
    # place, or without the key edge
    for dry, plain in (("in_dry", "in_plain"), ("key_dry", "key_plain")):
        assert not any(k.startswith("k_voc") for k in fams[dry]) and "k_band_scan" in fams[dry], fams[dry]
        if dry == "in_dry":
            assert {k: v for k, v in fams[dry].items() if k != "k_sample_loop"} == {k: v for k, v in fams[plain].items() if k != "k_sample_loop"}, (fams[dry], fams[plain])
    assert "k_band_scan" in fams["key_plain"], fams["key_plain"]
    sup, sfree = fams["sine_up"], fams["sine_free"]
    assert "k_sine_probe" not in sup and "k_synth" in sup, sup
    assert "k_sine_probe" in sfree and not any(k.startswith("k_voc") for k in sfree), sfree
    # a chunk of one tile is k_voc_apply alone; a level with two band counts, keyed and not, takes each step once per group
    assert [(k, v) for k, v in fams["one_tile"].items() if k.startswith("k_voc")] == [("k_voc_apply", 1)], fams["one_tile"]
    assert [(k, v) for k, v in fams["mixed"].items() if k.startswith("k_voc")] == [(k, 4) for k in VOC_LAUNCHES], fams["mixed"]


def test_projects_without_a_vocoder_keep_their_launch_list(asan_exe, tmp_path):
    projects = {"drums": W.drum_project(seconds=0.5), "config2": W.config2(seconds=0.5, n_src=8), "config4": W.config4(seconds=0.5, depth=6)}
    fams = _families(asan_exe, tmp_path, projects)
    for name in projects:
        got = " ".join("%s=%d" % kv for kv in fams[name].items())
        assert not any(k.startswith("k_voc") for k in fams[name]) and got == PARENT_LAUNCHES[name], (name, got)
