"""The gate vertex on the host, no GPU (include/termdaw_amd.h td_graph_add_gate): parameter ranges rejected with
messages that name the parameter, through the C ABI and through the Lua front-end; the canonical dump line; td_gate_params against
numpy's evaluation of the formulas; facts of the float64 twin (tests/np_gate.py) that can be derived by hand; the tiled scan
restated in numpy (np_gate.blocked) against the serial loop -- t[n] exactly, env within the bound's constant, which this file
derives; the host engine on random projects with gate vertices under AddressSanitizer / UBSan (tests/asan_comp.cpp as it is,
against tests/mock_hip.cpp + tests/mock_gate.cpp, whose mock launches check every descriptor's bounds, tiling, carry words and
launch order); and the guard rule and the launch lists, read from the launch families the mock build reports.

The inputs of the scan tests are made here without a device: the `gated` asset at the levels its loop plays it at
(gate_projects.gated_frames), and noise and drum-like bursts of the levels the GPU test's buses have."""
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
import gate_projects as GP  # noqa: E402
import np_gate as NG  # noqa: E402
from fx_rig import ENV, PARENT_LAUNCHES, _families  # noqa: E402

GOOD = dict(threshold_db=-30.0, hysteresis_db=6.0, hold_ms=10.0, attack_ms=1.0, release_ms=100.0, range_db=-60.0)
RANGES = dict(threshold_db=(-80.0, 0.0), hysteresis_db=(0.0, 24.0), hold_ms=(0.0, 2000.0), attack_ms=(0.0, 1000.0), release_ms=(1.0, 10000.0),
              range_db=(-120.0, 0.0))
ORDER = ["threshold_db", "hysteresis_db", "hold_ms", "attack_ms", "release_ms", "range_db"]
BAD = [(k, v) for k, (lo, hi) in RANGES.items() for v in (np.nextafter(np.float32(lo), np.float32(-1e9)), np.nextafter(np.float32(hi), np.float32(1e9)),
                                                           float("nan"), float("inf"), float("-inf"))]


def _args(**kw):
    return fx_rig._args(GOOD, ORDER, as_float=True, **kw)


# ---- ranges, the Lua line, the project script ----
@pytest.mark.parametrize("name,value", BAD)
def test_out_of_range_parameters_are_rejected_by_name(api, name, value):
    fx_rig.out_of_range_is_rejected_by_name(api, 48000, lambda g, *a: g.add_gate("g", 1.0, 0.0, 1.0, *a), api.gate_params, _args(**{name: value}), name)


def test_range_ends_are_accepted(api):
    fx_rig.range_ends_are_accepted(api, 48000, lambda g, *a: g.add_gate(*a), "g", RANGES, ORDER, _args())


def _lua(line):
    return fx_rig._lua(line, "g")


@pytest.mark.parametrize("name,value", [(k, v) for k, v in BAD if math.isfinite(v)])
def test_lua_rejects_the_same_ranges(api, name, value):
    fx_rig.lua_rejects_the_same_ranges(api, 48000, "add_gate", _args(**{name: value}), name)


def test_lua_accepts_and_dumps_the_canonical_line(api):
    s = api.State("", 48000, 64)
    assert s.refresh(_lua('add_gate("g", 0.5, -30, 1, -30, 4, 0, 100.5, 6.5, -60);')), api.last_error()
    dump = s.dump_calls()
    band = api.State("", 48000, 64)
    assert band.refresh('add_sum("in", 1.0, 0.0);\nadd_bandpass("b", 0.5, -30, 1, 100.5, 4, true);\nconnect("in", "b");\nset_output("b");\n'), api.last_error()
    # the numbers print as add_bandpass prints the same values
    half, m30, one, x1005, four = band.dump_calls().split('add_bandpass("b",')[1].split(")")[0].split(",")[:5]
    line = [ln for ln in dump.splitlines() if ln.startswith("add_gate(")]
    assert len(line) == 1
    args = line[0][len("add_gate("):-1].split(",")
    assert args[0] == '"g"' and args[1] == half and args[2] == m30 and args[3] == one and args[4] == m30 and args[5] == four and args[7] == x1005, line
    assert len(args) == 10 and " " not in line[0]


def test_project_script_records_and_writes_the_call(tmp_path):
    p = W.ProjectScript(48000, 64)
    p.add_sum("in", 1.0, 0.0)
    p.add_gate("g", 1.0, 0.0, 1.0, -30.0, 6.0, 10.0, 1.0, 100.0, -60.0)
    p.connect("in", "g")
    p.set_output("g")
    assert p.calls["add_gate"] == [("g", 1.0, 0.0, 1.0, -30.0, 6.0, 10.0, 1.0, 100.0, -60.0)]
    assert 'add_gate("g", 1.0, 0.0, 1.0, -30.0, 6.0, 10.0, 1.0, 100.0, -60.0);' in p.to_lua(str(tmp_path))


# ---- td_gate_params ----
def test_gate_params_match_the_formulas(api):
    """To, Tc, F against numpy's float64 power, aA, aR against numpy's exp, H against Python's round-half-away.  pow and exp come
    from the same libm on both sides here, but only correct rounding would make that a promise: the assertion is one ulp; the
    agreement found on this grid is printed (equal on every value when this test was written)."""
    worst = 0
    for sr in GP.RATES + (8000, 192000):
        for c in GP.grid_cases() + [tuple(RANGES[k][0] for k in ORDER), tuple(RANGES[k][1] for k in ORDER), (-17.3, 2.7, 33.3, 0.7, 77.7, -41.9)]:
            thr, hy, ho, at, re, ra = (float(np.float32(v)) for v in c)
            To, Tc, H, aA, aR, F = api.gate_params(sr, *c)
            want = (np.power(10.0, thr / 20.0), np.power(10.0, (thr - hy) / 20.0),
                    np.exp(-1.0 / (at * sr / 1000.0)) if at > 0.0 else 0.0, np.exp(-1.0 / (re * sr / 1000.0)), np.power(10.0, ra / 20.0))
            for got, w in zip((To, Tc, aA, aR, F), want):
                ulps = abs(got - float(w)) / np.spacing(float(w)) if w else abs(got)
                worst = max(worst, ulps)
                assert ulps <= 1.0, (sr, c, got, w)
            assert H == int(math.floor(ho * sr / 1000.0 + 0.5)) and isinstance(H, int), (sr, c, H)
            assert Tc <= To <= 1.0 and 0.0 < F <= 1.0 and 0.0 <= aA < 1.0 and 0.0 < aR < 1.0
    print("gate_params: worst disagreement with numpy %.3g ulp" % worst)
    assert api.gate_params(48000, -30.0, 6.0, 10.0, 0.0, 100.0, -20.0)[2:4] == (480, 0.0)


# ---- facts of the twin ----
def _const(level_db, n, sign=1.0):
    a = np.float32(10.0 ** (level_db / 20.0))
    return np.stack([np.full(n, sign * a, np.float32), np.full(n, np.float32(0.25) * a, np.float32)], axis=1)


def _consts(api, sr=48000, **kw):
    return api.gate_params(sr, *_args(**kw))


def test_twin_settles_open_above_the_threshold_and_stays_shut_below(api):
    c = _consts(api)
    x = _const(-12.0, 48000, -1.0)
    p, end = NG.process(x, c, processed=True)
    assert end[1] == 1 and end[2] == 0 and abs(end[0] - 1.0) < 1e-12
    assert np.array_equal(p[-1000:], x[-1000:])   # G = 1 to the last bit of f32
    q = _const(-40.0, 5000)
    p, end = NG.process(q, c, processed=True)
    F = c[5]
    assert end == (0.0, 0, c[2] + 1)
    assert np.array_equal(p, (q.astype(np.float64) * F).astype(np.float32))   # F exactly: env never leaves 0


def test_twin_keeps_the_entering_state_inside_the_band(api):
    c = _consts(api)
    band = _const(-33.0, 4000)
    t, env, end = NG.serial(NG.classes(band, c[0], c[1]), c, NG.closed(c[2]))
    assert not t.any() and end[1] == 0
    t, env, end = NG.serial(NG.classes(band, c[0], c[1]), c, (1.0, 1, 0))
    assert t.all() and end[1:] == (1, 0)
    # with no hysteresis there is no band: -33 dB closes
    c0 = _consts(api, hysteresis_db=0.0)
    t, _, end = NG.serial(NG.classes(band, c0[0], c0[1]), c0, (1.0, 1, 0))
    assert end[1] == 0 and t[:c0[2]].all() and not t[c0[2]:].any()


def test_twin_holds_a_gap_of_h_frames_and_closes_at_h_plus_one(api):
    c = _consts(api)
    H = c[2]
    assert H == 480
    for gap, closes in ((H, False), (H + 1, True)):
        x = np.concatenate([_const(-12.0, 100), _const(-60.0, gap), _const(-12.0, 50)])
        t, _, _ = NG.serial(NG.classes(x, c[0], c[1]), c, NG.closed(H))
        assert t[:100].all() and t[100 + gap:].all()
        assert (not t[100:100 + gap].all()) == closes and int((t[100:100 + gap] == 0).sum()) == (1 if closes else 0)


def test_twin_opens_in_one_frame_at_attack_zero(api):
    c = _consts(api, attack_ms=0.0)
    assert c[3] == 0.0
    x = np.concatenate([_const(-60.0, 10), _const(-6.0, 10)])
    _, env, _ = NG.serial(NG.classes(x, c[0], c[1]), c, NG.closed(c[2]))
    assert not env[:10].any() and (env[10:] == 1.0).all()


def test_twin_nan_and_infinite_frames_force_nothing(api):
    """Step 1: such a frame forces nothing in step 2 -- h stays what it was (an infinite sample does not open, a NaN does not
    close), and c goes on by step 3 as on any frame that keeps h: it stays 0 while open and H + 1 once shut.  The frame itself
    comes out as what IEEE makes of it, and only that frame."""
    c = _consts(api)
    H = c[2]
    for bad in (float("nan"), float("inf"), float("-inf")):
        x = _const(-12.0, 64)
        x[20, 0] = bad
        x[41, 1] = bad
        cl = NG.classes(x, c[0], c[1])
        assert cl[20] == 0 and cl[41] == 0
        _, _, end = NG.serial(cl, c, (1.0, 1, 0))
        assert end[1:] == (1, 0)
        p, _ = NG.process(x, c, processed=True, state=(1.0, 1, 0))
        fin = np.isfinite(p)
        assert not fin[20, 0] and not fin[41, 1] and fin.sum() == p.size - 2
        q = _const(-60.0, 64)
        q[20, 0] = bad
        _, env, end = NG.serial(NG.classes(q, c[0], c[1]), c, NG.closed(H))
        assert end == (0.0, 0, H + 1) and not env.any()   # (an infinite sample did not open it)


def _inputs(sr):
    """The three inputs at rate sr without a device, 0.5 s: `gated` as decoded (looped), noise of the GPU test's level, and drum-like
    decaying bursts."""
    n = int(math.ceil(0.5 * sr / 1024.0)) * 1024
    g = GP.gated_frames()
    gated = np.tile(g, (n // len(g) + 1, 1))[:n]
    rng = np.random.default_rng(sr)
    noise = (0.5 * rng.uniform(-1.0, 1.0, (n, 2))).astype(np.float32)
    tt = np.arange(n) % (sr // 8)
    drums = (0.9 * np.exp(-tt / (0.02 * sr))[:, None] * rng.uniform(-1.0, 1.0, (n, 2))).astype(np.float32)
    return {"drums": drums, "noise": noise, "gated": gated}


def test_twin_splits_give_the_one_piece_result_bitwise(api):
    x = _inputs(48000)["gated"][:6000]
    for case in GP.grid_cases()[::7]:
        c = api.gate_params(48000, *case)
        whole, end = NG.process(x, c, wet=0.7, gain=1.7, angle=30.0)
        for cut in (1, 777, 2048, 4999):
            a, st = NG.process(x[:cut], c, wet=0.7, gain=1.7, angle=30.0)
            b, st = NG.process(x[cut:], c, wet=0.7, gain=1.7, angle=30.0, state=st)
            assert np.array_equal(np.concatenate([a, b]).view(np.uint32), whole.view(np.uint32)) and st == end, (case, cut)


def test_array_forms_are_the_serial_loop(api):
    """target() and fade(), which the GPU test runs the grid through, against the plain loops -- bit for bit."""
    x = _inputs(44100)["gated"]
    for case in GP.grid_cases()[::11]:
        c = api.gate_params(44100, *case)
        cl = NG.classes(x, c[0], c[1])
        for st in (NG.closed(c[2]), (0.3, 1, 0), (0.9, 0, 3))[:2 + (case[2] > 0.0)]:
            t, env, end = NG.serial(cl, c, st)
            h2, c2, t2, e2 = NG.target(cl, c[2], st)
            assert np.array_equal(t, t2) and e2 == end[1:], case
            assert np.array_equal(NG.fade(t2[None], c[3], c[4], st[0])[0], env), case


# ---- the tiled scan restated ----
def _scan_grid(api):
    """Per rate and input: the grid's cases that differ in t or env (range_db enters neither), their constants and classes."""
    for sr in GP.RATES:
        ins = _inputs(sr)
        for kind in GP.INPUTS:
            seen = {}
            for case in GP.grid_cases():
                c = api.gate_params(sr, *case)
                seen.setdefault(c[:5], (case, c, NG.classes(ins[kind], c[0], c[1])))
            yield sr, kind, list(seen.values())


def test_blocked_scan_gives_the_serial_target_exactly_and_env_within_the_constant(api):
    """Over the whole grid, the three inputs, the three rates and every tiling of gate_projects.TILINGS: t[n] and the end (h, c)
    of np_gate.blocked() are the serial loop's, and the worst |env_blocked - env_serial| (full scale 1) stays at or under
    gate_projects.E_EMULATED, the figure the GPU test's bound is 8 x of."""
    worst, n = 0.0, 0
    for sr, kind, cases in _scan_grid(api):
        ts = [NG.target(cl, c[2], NG.closed(c[2])) for _, c, cl in cases]
        envs = NG.fade(np.stack([t[2] for t in ts]), np.array([c[3] for _, c, _ in cases]), np.array([c[4] for _, c, _ in cases]), 0.0)
        for (case, c, cl), (_, _, t, hc), env in zip(cases, ts, envs):
            for tile, run, lanes in GP.TILINGS:
                tb, eb, end = NG.blocked(cl, c, None, tile, run, lanes)
                assert np.array_equal(tb, t) and end[1:] == hc, (sr, kind, case, tile, run, lanes)
                worst = max(worst, float(np.abs(eb - env).max()))
            n += 1
    print("blocked scan: %d cases x %d tilings, worst |env - serial| %.3g (E_EMULATED %.3g, E %.3g = 2^%.1f)" %
          (n, len(GP.TILINGS), worst, GP.E_EMULATED, GP.E, math.log2(GP.E)))
    assert n == 3 * 3 * 54
    assert 0.0 < worst <= GP.E_EMULATED and GP.E == 8.0 * GP.E_EMULATED and GP.E <= 2.0 ** -28


def test_blocked_scan_continues_from_a_carried_state(api):
    x = _inputs(48000)["gated"]
    c = api.gate_params(48000, -30.0, 6.0, 10.0, 1.0, 100.0, -20.0)
    cl = NG.classes(x, c[0], c[1])
    t, env, end = NG.serial(cl, c, NG.closed(c[2]))
    for cut in (1, 777, 2048, 4999):
        ta, ea, st = NG.blocked(cl[:cut], c, None)
        tb, eb, st = NG.blocked(cl[cut:], c, st)
        assert np.array_equal(np.concatenate([ta, tb]), t) and st[1:] == end[1:]
        assert np.abs(np.concatenate([ea, eb]) - env).max() <= GP.E_EMULATED


# ---- the host engine under sanitizers ----
@pytest.fixture(scope="module")
def asan_exe(tmp_path_factory):
    return fx_rig.asan_exe(tmp_path_factory, "asan_gate", ["mock_gate.cpp", "asan_comp.cpp"])


GATE_LAUNCHES = ("k_gate_detect", "k_gate_carry_hc", "k_gate_env", "k_gate_carry_env", "k_gate_apply")


def test_gate_projects_under_sanitizers(asan_exe, tmp_path):
    n = int(os.environ.get("TD_ASAN_GATE_SEEDS", "32"))
    workers = max(1, min(8, os.cpu_count() or 1))
    seeds = list(range(n))
    base = str(tmp_path / "p")
    with multiprocessing.Pool(workers) as pool:
        lists = pool.map(GP.write_projects, [(base, seeds[i::workers]) for i in range(workers) if seeds[i::workers]])
    procs = [subprocess.Popen([asan_exe] + lst, env=dict(os.environ, **ENV), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for lst in lists]
    launches = vertices = carried = fresh = 0
    for p in procs:
        out, err = p.communicate(timeout=1800)
        assert p.returncode == 0, (out[-800:], err[-4000:])
        # (the driver is the compressor's, as it is: its summary calls the effect launches it counted "k_comp")
        tail = out.split("asan_comp done:")[1]
        launches += int(tail.split("k_comp launches ")[1].split()[0])
        vertices += int(tail.split("(")[1].split()[0])
        fresh += int(tail.split(" entered fresh")[0].split()[-1])
        carried += int(tail.split(" entered with carried state")[0].split()[-1])
    # every project holds a gate vertex; multi-chunk renders and block pulls enter with carried state
    assert launches >= n and vertices >= launches and fresh > 0 and carried > 0, (launches, vertices, fresh, carried)
    print("asan_gate: %d projects, %d launches, %d vertices (%d fresh, %d carried) clean" % (n, launches, vertices, fresh, carried))


def _guard_project(shape):
    return fx_rig.guard_project(shape, lambda p, name, dry: p.add_gate(name, 1.0, 0.0, 0.0 if dry else 1.0, -30.0, 6.0, 10.0, 1.0, 100.0, -40.0))


def test_guard_modes_keep_the_exact_forms_upstream_of_a_gate(asan_exe, tmp_path):
    """band_mode 2 / sine_mode 2 (the driver's profiled render): the launch families each shape went through."""
    shapes = ("band_up", "band_down", "band_both", "band_dry", "band_plain", "sine_up", "sine_free")
    fams = _families(asan_exe, tmp_path, {s: _guard_project(s) for s in shapes})
    exact = ("k_band_pass", "k_band_spec")
    up, down, both = fams["band_up"], fams["band_down"], fams["band_both"]
    assert "k_band_scan" not in up and any(k in up for k in exact), up
    assert "k_band_scan" in down and not any(k in down for k in exact), down
    assert "k_band_scan" in both and any(k in both for k in exact), both
    for f in (up, down, both):
        assert all(f.get(k) == 1 for k in GATE_LAUNCHES), f
        assert [k for k in f if k.startswith("k_gate")] == list(GATE_LAUNCHES), f   # (and in this order)
    # wet < 0.0001 compiles to k_sum: the launch list of the project with a Sum in the gate's place
    dry, plain = fams["band_dry"], fams["band_plain"]
    assert not any(k.startswith("k_gate") for k in dry) and list(dry.items()) == list(plain.items()), (dry, plain)
    sup, sfree = fams["sine_up"], fams["sine_free"]
    assert "k_sine_probe" not in sup and "k_synth" in sup, sup
    assert "k_sine_probe" in sfree, sfree
    assert not any(k.startswith("k_gate") for k in sfree), sfree


def test_projects_without_a_gate_keep_their_launch_list(asan_exe, tmp_path):
    projects = {"drums": W.drum_project(seconds=0.5), "config2": W.config2(seconds=0.5, n_src=8), "config4": W.config4(seconds=0.5, depth=6)}
    fams = _families(asan_exe, tmp_path, projects)
    for name in projects:
        got = " ".join("%s=%d" % kv for kv in fams[name].items())
        assert not any(k.startswith("k_gate") for k in fams[name]) and got == PARENT_LAUNCHES[name], (name, got)
