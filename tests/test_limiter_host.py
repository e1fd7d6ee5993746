"""The limiter vertex without a GPU (td_graph_add_limiter): the ranges through the C ABI and Lua, the canonical
dump line, td_limiter_params against numpy, the facts of the float64 twin (tests/np_limiter.py) that the definition promises,
the derivation of the GPU test's error constant from the numpy emulation of the kernels' order, the host engine under ASan / UBSan
-- a stand-alone program: tests/asan_fx.cpp with tests/mock_hip.cpp, tests/mock_guard.cpp and tests/mock_limiter.cpp, whose
launches check every descriptor -- and the guard rule and the launch lists, read from the launch families that build reports."""
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
import limiter_projects as LP  # noqa: E402
import np_limiter as NL  # noqa: E402
from fx_rig import ENV, PARENT_LAUNCHES, _families  # noqa: E402

GOOD = dict(ceiling_db=-1.0, lookahead_ms=5.0, release_ms=80.0, drive_db=6.0)
RANGES = dict(ceiling_db=(-24.0, 0.0), lookahead_ms=(0.0, 50.0), release_ms=(1.0, 10000.0), drive_db=(-24.0, 24.0))
ORDER = ["ceiling_db", "lookahead_ms", "release_ms", "drive_db"]
BAD = [(k, v) for k, (lo, hi) in RANGES.items() for v in (np.nextafter(np.float32(lo), np.float32(-1e9)), np.nextafter(np.float32(hi), np.float32(1e9)),
                                                           float("nan"), float("inf"), float("-inf"))]
SR_ENDS = 40000   # (the range ends are taken at a rate where 50 ms is no more than 2 048 frames)


def _args(**kw):
    return fx_rig._args(GOOD, ORDER, as_float=True, **kw)


# ---- ranges, the Lua line, the project script ----
@pytest.mark.parametrize("name,value", BAD)
def test_out_of_range_parameters_are_rejected_by_name(api, name, value):
    fx_rig.out_of_range_is_rejected_by_name(api, SR_ENDS, lambda g, *a: g.add_limiter("m", 1.0, 0.0, 1.0, *a), api.limiter_params, _args(**{name: value}), name)


def test_range_ends_are_accepted(api):
    fx_rig.range_ends_are_accepted(api, SR_ENDS, lambda g, *a: g.add_limiter(*a), "m", RANGES, ORDER, _args())
    assert api.limiter_params(SR_ENDS, *[RANGES[k][1] for k in ORDER])[2] == 2000


@pytest.mark.parametrize("sr", LP.RATES)
def test_a_window_of_2048_frames_is_accepted_and_2049_rejected(api, sr):
    ok, over = LP.lookahead_ms(sr, 2048), LP.lookahead_ms(sr, 2049)
    assert over <= 50.0
    c = api.limiter_params(sr, -1.0, ok, 80.0, 6.0)
    assert c[2] == 2048 and c[4] == 2047
    g = api.Graph(64, sr)
    g.add_limiter("m", 1.0, 0.0, 1.0, -1.0, ok, 80.0, 6.0)
    for call in (lambda: api.limiter_params(sr, -1.0, over, 80.0, 6.0), lambda: g.add_limiter("n", 1.0, 0.0, 1.0, -1.0, over, 80.0, 6.0)):
        with pytest.raises(api.TermdawError, match="lookahead_ms"):
            call()
    s = api.State("", sr, 64)
    assert not s.refresh(_lua('add_limiter("g", 1.0, 0.0, 1.0, -1.0, %r, 80.0, 6.0);' % over))
    assert "lookahead_ms" in api.last_error() and "2048" in api.last_error(), api.last_error()
    assert s.refresh(_lua('add_limiter("g", 1.0, 0.0, 1.0, -1.0, %r, 80.0, 6.0);' % ok)), api.last_error()


def _lua(line):
    return fx_rig._lua(line, "g")


@pytest.mark.parametrize("name,value", [(k, v) for k, v in BAD if math.isfinite(v)])
def test_lua_rejects_the_same_ranges(api, name, value):
    fx_rig.lua_rejects_the_same_ranges(api, SR_ENDS, "add_limiter", _args(**{name: value}), name)


def test_lua_accepts_and_dumps_the_canonical_line(api):
    s = api.State("", 48000, 64)
    assert s.refresh(_lua('add_limiter("g", 0.5, -30, 1, -3, 4, 100.5, 6.5);')), api.last_error()
    dump = s.dump_calls()
    band = api.State("", 48000, 64)
    assert band.refresh('add_sum("in", 1.0, 0.0);\nadd_bandpass("b", 0.5, -30, 1, 100.5, 4, true);\nconnect("in", "b");\nset_output("b");\n'), api.last_error()
    # the numbers print as add_bandpass prints the same values
    half, m30, one, x1005, four = band.dump_calls().split('add_bandpass("b",')[1].split(")")[0].split(",")[:5]
    line = [ln for ln in dump.splitlines() if ln.startswith("add_limiter(")]
    assert len(line) == 1
    args = line[0][len("add_limiter("):-1].split(",")
    assert args[0] == '"g"' and args[1] == half and args[2] == m30 and args[3] == one and args[5] == four and args[6] == x1005, line
    assert len(args) == 8 and " " not in line[0]


def test_connect_key_into_a_limiter_is_refused(api):
    g = api.Graph(64, 48000)
    g.add_sum("in", 1.0, 0.0)
    g.add_sum("key", 1.0, 0.0)
    g.add_limiter("m", 1.0, 0.0, 1.0, *_args())
    assert g.connect("in", "m")
    assert not g.connect_key("key", "m")
    assert "takes no key input" in api.last_error(), api.last_error()


def test_project_script_records_and_writes_the_call(tmp_path):
    p = W.ProjectScript(48000, 64)
    p.add_sum("in", 1.0, 0.0)
    p.add_limiter("m", 1.0, 0.0, 1.0, -1.0, 5.0, 80.0, 6.0)
    p.connect("in", "m")
    p.set_output("m")
    assert p.calls["add_limiter"] == [("m", 1.0, 0.0, 1.0, -1.0, 5.0, 80.0, 6.0)]
    assert 'add_limiter("m", 1.0, 0.0, 1.0, -1.0, 5.0, 80.0, 6.0);' in p.to_lua(str(tmp_path))
    q = W.limiter_project(seconds=0.5)
    assert q.output_vertex == "lim" and ("band", "lim") in q.calls["connect"] and len(q.calls["add_limiter"]) == 1


# ---- td_limiter_params ----
def test_limiter_params_match_the_formulas(api):
    """c, gin against numpy's float64 power, a against numpy's exp, L against round-half-away.  pow and exp come from the same libm
    on both sides here, but only correct rounding would make that a promise: the assertion is a few ulp; the agreement found on
    this grid is printed."""
    worst = 0
    for sr in LP.RATES + (8000, 192000):
        cases = [c for c, _ in LP.grid_cases(48000)] + [(-17.3, 3.3, 77.7, 11.9), (-24.0, 0.0, 1.0, -24.0), (0.0, 10.0, 10000.0, 24.0)]
        for case in cases:
            ce, la, re, dr = (float(np.float32(v)) for v in case)
            if math.floor(la * sr / 1000.0 + 0.5) > 2048:
                continue
            c, gin, Lw, a, lat = api.limiter_params(sr, *case)
            want = (np.power(10.0, ce / 20.0), np.power(10.0, dr / 20.0), np.exp(-1.0 / (re * sr / 1000.0)))
            for got, w in zip((c, gin, a), want):
                ulps = abs(got - float(w)) / np.spacing(float(w))
                worst = max(worst, ulps)
                assert ulps <= 2.0, (sr, case, got, w)
            assert Lw == max(1, int(math.floor(la * sr / 1000.0 + 0.5))) and lat == Lw - 1 and isinstance(Lw, int), (sr, case, Lw)
            assert 0.0 < c <= 1.0 and 0.0 < a < 1.0
    print("limiter_params: worst disagreement with numpy %.3g ulp" % worst)
    instant = api.limiter_params(48000, -6.0, 0.0, 50.0, 0.0)
    assert instant[2] == 1 and instant[4] == 0   # (lookahead_ms 0: one frame, no latency)


# ---- facts of the twin ----
def _consts(api, sr, case):
    return api.limiter_params(sr, *case)


def _bursts(n, seed=3, peak=0.9):
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    env = 0.02 + peak * np.exp(-(t % 3000) / 400.0)
    l = env * rng.uniform(-1.0, 1.0, n)
    return np.stack([l, 0.7 * l[::-1]], axis=1).astype(np.float32)


def test_twin_wet_path_never_exceeds_the_ceiling(api):
    """|p| <= c (1 + 2^-23) on every grid case: gin |xd| G <= c before p's one f32 rounding."""
    x = _bursts(12000)
    worst = 0.0
    for sr in LP.RATES:
        for case, Lw in LP.grid_cases(sr):
            k = _consts(api, sr, case)
            p, xd, G, _, p64 = NL.serial(x, k)
            worst = max(worst, float(np.abs(p).max() / k[0] - 1.0))
            assert np.abs(p).max() <= k[0] * (1.0 + 2.0 ** -23), (sr, case, float(np.abs(p).max()), k[0])
            assert (G <= 1.0).all() and (G >= 0.0).all()
    print("twin: worst overshoot over the ceiling %.3g (2^-23 = %.3g)" % (worst, 2.0 ** -23))


def test_twin_hands_an_idle_input_on_driven_and_delayed_bit_for_bit(api):
    x = _bursts(9000, peak=0.3)
    for Lw in (1, 2, 48, 480, 2048):
        k = _consts(api, 48000, (-0.1, LP.lookahead_ms(48000, Lw), 50.0, 6.0))
        assert k[2] == Lw and np.abs(x).max() * k[1] < k[0]
        p, xd, G, end, _ = NL.serial(x, k)
        assert (G == 1.0).all() and end[0] == 0.0 and (end[2] == 1.0).all()
        want = np.concatenate([np.zeros((Lw - 1, 2), np.float32), x])[:len(x)]
        assert np.array_equal(xd, want)
        assert np.array_equal(p.view(np.uint32), (want.astype(np.float64) * k[1]).astype(np.float32).view(np.uint32))
        pb, _, Gb, _, _ = NL.blocked(x, k)
        assert (Gb == 1.0).all() and np.array_equal(pb.view(np.uint32), p.view(np.uint32))   # (also in the tiled prefix-sum form)


def test_twin_splits_give_the_one_piece_result_bitwise(api):
    x = _bursts(7000)
    cuts = [0, 1, 63, 777, 2048, 4999, len(x)]
    for Lw in (1, 2, 48, 480, 2048):   # (at 480 and 2 048 the first three pieces are shorter than L - 1)
        k = _consts(api, 48000, (-6.0, LP.lookahead_ms(48000, Lw), 50.0, 12.0))
        p, _, G, end, _ = NL.serial(x, k)
        assert G.min() < 0.5
        st, parts = None, []
        for a, b in zip(cuts[:-1], cuts[1:]):
            q, _, _, st, _ = NL.serial(x[a:b], k, st)
            parts.append(q)
        assert np.array_equal(np.concatenate(parts).view(np.uint32), p.view(np.uint32)), Lw
        assert st[0] == end[0] and np.array_equal(st[1], end[1]) and np.array_equal(st[2], end[2])


def test_twin_keeps_a_nan_frame_out_of_the_state(api):
    for bad in (float("nan"), float("inf"), float("-inf")):
        for Lw in (1, 48):
            k = _consts(api, 48000, (-6.0, LP.lookahead_ms(48000, Lw), 50.0, 12.0))
            x = _bursts(4000)
            y = x.copy()
            y[1000, 0] = bad
            y[1000, 1] = np.float32(0.0)
            x[1000] = 0.0   # (the same frame, silent: what the state sees of the bad one)
            p, _, G, end, _ = NL.serial(x, k)
            q, _, Gq, endq, _ = NL.serial(y, k)
            assert np.array_equal(G, Gq) and endq[0] == end[0] and np.array_equal(endq[2], end[2])
            at = 1000 + Lw - 1
            fin = np.isfinite(q)
            assert not fin[at, 0] and fin.sum() == q.size - 1   # it surfaces at frame n + L - 1, on its channel, and nowhere else
            keep = np.ones(len(x), bool)
            keep[at] = False
            assert np.array_equal(q[keep].view(np.uint32), p[keep].view(np.uint32))


# ---- the bound of tests/test_gpu_limiter.py ----
def _emulate(job):
    sr, kind, consts = job
    x = LP.oracle_input(kind, sr)
    assert len(x) > 5 * NL.TILE and np.abs(x).max() > 0.05
    worst, deep = (0.0, -1), 0
    for i, k in enumerate(consts):
        p, _, G, end, p64 = NL.serial(x, k)
        pb, _, _, endb, pb64 = NL.blocked(x, k)
        worst = max(worst, (float(np.abs(pb64 - p64).max() / np.abs(p64).max()), i))
        deep += int(G.min() < 0.5)
        assert np.array_equal(endb[1], end[1]) and np.abs(endb[2] - end[2]).max(initial=0.0) <= 2.0 ** -28 and abs(endb[0] - end[0]) <= 2.0 ** -28
    return worst, deep


def test_blocked_order_stays_inside_the_committed_constant(api):
    """E = 8 x the worst max|blocked - serial| / max|serial| of the numpy emulation over the GPU test's own grid and inputs at the
    three rates; this recomputes that worst figure and fails above E / 8."""
    jobs, what = [], []
    for sr in LP.RATES:
        cases = LP.grid_cases(sr)
        assert len(cases) == 45
        consts = [api.limiter_params(sr, *c) for c, _ in cases]
        assert [k[2] for k in consts] == [Lw for _, Lw in cases]
        for kind in LP.INPUTS:
            jobs.append((sr, kind, consts))
            what.append((cases, sr, kind))
    with multiprocessing.Pool(max(1, min(len(jobs), os.cpu_count() or 1))) as pool:
        results = pool.map(_emulate, jobs)
    worst, n = (0.0, None), 0
    for (w, deep), (cases, sr, kind) in zip(results, what):
        if w[0] > worst[0]:
            worst = (w[0], (cases[w[1]], sr, kind))
        n += len(cases)
        assert 3 * deep >= len(cases), (sr, kind, deep)   # (the grid works: G under 0.5 in at least a third of the cases)
    print("blocked order: %d cases, worst max|blocked - serial| / max|serial| %.3g at %s (E_EMULATED %.3g, E %.3g = 2^%.1f)" %
          (n, worst[0], worst[1], LP.E_EMULATED, LP.E, math.log2(LP.E)))
    assert n == 3 * 3 * 45
    assert 0.0 < worst[0] <= LP.E_EMULATED and LP.E == 8 * LP.E_EMULATED and LP.E <= 2 ** -28


def test_blocked_order_continues_from_a_carried_state(api):
    x = _bursts(9000)
    for Lw in (1, 48, 2048):
        k = _consts(api, 48000, (-6.0, LP.lookahead_ms(48000, Lw), 50.0, 12.0))
        _, _, _, end, p64 = NL.serial(x, k)
        for cut in (1, 777, 2048, 4999):
            _, _, _, st, a = NL.blocked(x[:cut], k)
            _, _, _, st, b = NL.blocked(x[cut:], k, st)
            assert np.abs(np.concatenate([a, b]) - p64).max() <= LP.E_EMULATED * np.abs(p64).max(), (Lw, cut)
            assert np.array_equal(st[1], end[1]) and np.abs(st[2] - end[2]).max(initial=0.0) <= 2.0 ** -28


# ---- the host engine under sanitizers ----
@pytest.fixture(scope="module")
def asan_exe(tmp_path_factory):
    return fx_rig.asan_exe(tmp_path_factory, "asan_limiter", ["mock_guard.cpp", "mock_limiter.cpp", "asan_fx.cpp"])


LIM_LAUNCHES = ("k_lim_detect", "k_lim_carry", "k_lim_apply")


def test_random_limiter_projects_hold_one_to_four_limiters():
    long_windows = 0
    for seed in range(16):
        p = LP.random_limiter_project(seed)
        assert 1 <= len(p.calls["add_limiter"]) <= 4
        long_windows += sum(1 for c in p.calls["add_limiter"] if c[5] > 40.0)
    assert long_windows >= 2   # (windows of 2 048 frames: a 1 024-frame pull is shorter than the line)


def test_limiter_projects_under_sanitizers(asan_exe, tmp_path):
    n = int(os.environ.get("TD_ASAN_LIMITER_SEEDS", "32"))
    workers = max(1, min(8, os.cpu_count() or 1))
    seeds = list(range(n))
    base = str(tmp_path / "p")
    with multiprocessing.Pool(workers) as pool:
        lists = pool.map(LP.write_projects, [(base, seeds[i::workers]) for i in range(workers) if seeds[i::workers]])
    procs = [subprocess.Popen([asan_exe] + lst, env=dict(os.environ, **ENV), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for lst in lists]
    tot = dict(apply=0, vertices=0, single=0, fresh=0, carried=0, detect=0, rejected=0, restarts=0, short=0)
    for p in procs:
        out, err = p.communicate(timeout=1800)
        assert p.returncode == 0, (out[-800:], err[-4000:])
        tail = out.split("asan_limiter done:")[1]
        tot["apply"] += int(tail.split("k_lim_apply descriptors ")[1].split()[0])
        tot["vertices"] += int(tail.split("(")[1].split()[0])
        tot["single"] += int(tail.split(" one-launch")[0].split()[-1])
        tot["fresh"] += int(tail.split(" entered fresh")[0].split()[-1])
        tot["carried"] += int(tail.split(" entered with the line")[0].split()[-1])
        tot["detect"] += int(tail.split(" k_lim_detect descriptors")[0].split()[-1])
        tot["restarts"] += int(tail.split(" restarts checked")[0].split()[-1])
        tot["short"] += int(tail.split(" short chunks")[0].split()[-1])
        tot["rejected"] += int(tail.split(" rejected refreshes")[0].split()[-1])
    # whole renders and 4 096-frame chunks take three launches, block pulls one; chunks and pulls enter with the line; pulls
    # shorter than the line occur; the pull behind a set_time enters fresh (the mock aborts where it does not)
    assert tot["rejected"] == 0 and tot["apply"] >= n // 2 and tot["vertices"] == tot["apply"], tot
    assert tot["fresh"] > 0 and tot["carried"] > 0 and tot["single"] > 0 and 0 < tot["detect"] < tot["apply"], tot
    assert tot["restarts"] > 0 and tot["short"] > 0, tot
    print("asan_limiter: %d projects clean: %s" % (n, tot))


LIM = (-6.0, 5.0, 80.0, 12.0)


def _guard_project(shape, seconds=0.5):
    return fx_rig.guard_project(shape, lambda p, name, dry: p.add_limiter(name, 1.0, 0.0, 0.0 if dry else 1.0, *LIM), seconds=seconds)


def test_launch_families_and_the_guard_rule(asan_exe, tmp_path):
    """band_mode 2 / sine_mode 2 (the driver's profiled render): the launch families each shape went through."""
    shapes = ("band_up", "band_down", "band_dry", "band_plain", "sine_up", "sine_free")
    projects = {s: _guard_project(s) for s in shapes}
    projects["one_tile"] = _guard_project("one_tile", seconds=0.04)
    assert projects["one_tile"].cs * 1024 == NL.TILE
    fams = _families(asan_exe, tmp_path, projects)
    exact = ("k_band_pass", "k_band_spec")
    up, down = fams["band_up"], fams["band_down"]
    # upstream of a limiter that is not dry: the exact forms; downstream the guard is free
    assert "k_band_scan" not in up and any(k in up for k in exact), up
    assert "k_band_scan" in down and not any(k in down for k in exact), down
    for f in (up, down):
        assert [(k, v) for k, v in f.items() if k.startswith("k_lim")] == [(k, 1) for k in LIM_LAUNCHES], f   # (the three, in this order)
    # wet < 0.0001 compiles to k_sum: the launch list of the project with a Sum in the limiter's place
    dry, plain = fams["band_dry"], fams["band_plain"]
    assert not any(k.startswith("k_lim") for k in dry) and list(dry.items()) == list(plain.items()), (dry, plain)
    sup, sfree = fams["sine_up"], fams["sine_free"]
    assert "k_sine_probe" not in sup and "k_synth" in sup, sup
    assert "k_sine_probe" in sfree and not any(k.startswith("k_lim") for k in sfree), sfree
    # a chunk of one tile is k_lim_apply alone
    assert [(k, v) for k, v in fams["one_tile"].items() if k.startswith("k_lim")] == [("k_lim_apply", 1)], fams["one_tile"]


def test_projects_without_a_limiter_keep_their_launch_list(asan_exe, tmp_path):
    projects = {"drums": W.drum_project(seconds=0.5), "config2": W.config2(seconds=0.5, n_src=8), "config4": W.config4(seconds=0.5, depth=6)}
    fams = _families(asan_exe, tmp_path, projects)
    for name in projects:
        got = " ".join("%s=%d" % kv for kv in fams[name].items())
        assert not any(k.startswith("k_lim") for k in fams[name]) and got == PARENT_LAUNCHES[name], (name, got)
