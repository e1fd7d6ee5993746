"""The phaser vertex on the host, no GPU (include/termdaw_amd.h td_graph_add_phaser): parameter ranges rejected
with messages that name the parameter, through the C ABI and through the Lua front-end (NaN and the infinities included); the
canonical dump line; td_phaser_params against numpy's evaluation of the formulas; facts of the float64 twin (tests/np_phaser.py)
that can be derived by hand; the tiled scan restated in numpy (np_phaser.blocked, the kernels' tile geometry and join order)
against the serial loop, within the bound's constant, which this file derives; the host engine on random projects with phaser
vertices under AddressSanitizer / UBSan (a stand-alone program: tests/asan_comp.cpp as it is, against tests/mock_hip.cpp +
tests/mock_phaser.cpp, whose mock launches check every descriptor's bounds, tile counts, scratch sizes and launch order); and the
guard rule and the launch lists, read from the launch families the mock build reports."""
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
import np_phaser as NP  # noqa: E402
import phaser_projects as PP  # noqa: E402
from fx_rig import ENV, PARENT_LAUNCHES, _families, oracle_input  # noqa: E402
SR = 48000

GOOD = dict(stages=4, lo_hz=200.0, hi_hz=2000.0, rate_hz=1.0, feedback=0.5, stereo=0.25, shape=0)
ORDER = ["stages", "lo_hz", "hi_hz", "rate_hz", "feedback", "stereo", "shape"]
RANGES = dict(lo_hz=(20.0, None), hi_hz=(None, 0.45 * SR), rate_hz=(0.01, 20.0), feedback=(-0.95, 0.95), stereo=(0.0, 0.5))
NON_FINITE = (float("nan"), float("inf"), float("-inf"))


def _below(v):
    return float(np.nextafter(np.float32(v), np.float32(-1e9)))


def _above(v):
    return float(np.nextafter(np.float32(v), np.float32(1e9)))


BAD = [(k, _below(lo)) for k, (lo, hi) in RANGES.items() if lo is not None] + [(k, _above(hi)) for k, (lo, hi) in RANGES.items() if hi is not None]
BAD += [(k, v) for k in RANGES for v in NON_FINITE]
BAD += [("stages", v) for v in (0, 1, 3, 5, 7, 9, 10, -2)] + [("shape", 2), ("shape", -1)]
BAD += [("lo_hz", 2000.5), ("hi_hz", 199.5)]   # lo_hz <= hi_hz: the message names both


def _args(**kw):
    return fx_rig._args(GOOD, ORDER, **kw)


# ---- ranges, the Lua line, the project script ----
@pytest.mark.parametrize("name,value", BAD)
def test_out_of_range_parameters_are_rejected_by_name(api, name, value):
    fx_rig.out_of_range_is_rejected_by_name(api, SR, lambda g, *a: g.add_phaser("p", 1.0, 0.0, 1.0, *a), api.phaser_params, _args(**{name: value}), name)


def test_range_ends_are_accepted_and_follow_the_rate(api):
    g = api.Graph(64, SR)
    g.add_sum("in", 1.0, 0.0)
    ends = [(2, 20.0, 0.45 * SR, 0.01, -0.95, 0.0, "sine"), (8, 20.0, 20.0, 20.0, 0.95, 0.5, "triangle"), (6, 0.45 * SR, 0.45 * SR, 1.0, 0.0, 0.25, 1)]
    for i, c in enumerate(ends):
        g.add_phaser("p%d" % i, 1.0, 0.0, 1.0, *c)
        assert g.connect("in", "p%d" % i)
    g.add_phaser("wet", 1.0, 0.0, 7.0, *_args())   # (wet is clamped, not rejected: graph.rs:256)
    g.add_phaser("dry", 1.0, 0.0, -3.0, *_args())
    assert g.set_output("p1") and g.check_graph()
    for sr in (44100, 96000):   # hi_hz's end is 0.45 of the graph's own rate
        h = api.Graph(64, sr)
        h.add_phaser("p", 1.0, 0.0, 1.0, *_args(hi_hz=0.45 * sr))
        with pytest.raises(api.TermdawError, match="hi_hz"):
            h.add_phaser("q", 1.0, 0.0, 1.0, *_args(hi_hz=_above(0.45 * sr)))


def _lua(line):
    return fx_rig._lua(line, "g")


def _lit(v):
    if isinstance(v, str):
        return '"%s"' % v
    if isinstance(v, int):
        return str(v)
    if math.isnan(v):
        return "0/0"
    if math.isinf(v):
        return "1/0" if v > 0 else "-1/0"
    return repr(float(v))


@pytest.mark.parametrize("name,value", [(k, v) for k, v in BAD if k != "shape"])
def test_lua_rejects_the_same_ranges(api, name, value):
    s = api.State("", SR, 64)
    a = _args(**{name: value})
    a[6] = "sine"
    line = 'add_phaser("g", 1.0, 0.0, 1.0, %s);' % ", ".join(_lit(v) for v in a)
    assert not s.refresh(_lua(line))
    assert name in api.last_error(), api.last_error()


def test_lua_rejects_unknown_shape_strings(api):
    s = api.State("", SR, 64)
    assert not s.refresh(_lua('add_phaser("g", 1.0, 0.0, 1.0, 4, 200.0, 2000.0, 1.0, 0.5, 0.25, "square");'))
    assert "shape" in api.last_error(), api.last_error()


def test_lua_accepts_and_dumps_the_canonical_line(api):
    s = api.State("", SR, 64)
    assert s.refresh(_lua('add_phaser("g", 0.5, -30, 1, 4, 100.5, 2000, 1, 0.5, 0.25, "triangle");')), api.last_error()
    dump = s.dump_calls()
    band = api.State("", SR, 64)
    assert band.refresh('add_sum("in", 1.0, 0.0);\nadd_bandpass("b", 0.5, -30, 1, 100.5, 4, true);\nconnect("in", "b");\nset_output("b");\n'), api.last_error()
    # the numbers print as add_bandpass prints the same values
    half, m30, one, x1005, four = band.dump_calls().split('add_bandpass("b",')[1].split(")")[0].split(",")[:5]
    line = [ln for ln in dump.splitlines() if ln.startswith("add_phaser(")]
    assert len(line) == 1
    args = line[0][len("add_phaser("):-1].split(",")
    assert args[0] == '"g"' and args[1] == half and args[2] == m30 and args[3] == one and args[4] == four and args[5] == x1005 and args[7] == one, line
    assert args[8] == half and args[10] == '"triangle"' and len(args) == 11 and " " not in line[0]


def test_project_script_records_and_writes_the_call(tmp_path):
    p = W.ProjectScript(SR, 64)
    p.add_sum("in", 1.0, 0.0)
    p.add_phaser("g", 1.0, 0.0, 1.0, 4, 200.0, 2000.0, 1.0, 0.5, 0.25, "sine")
    p.connect("in", "g")
    p.set_output("g")
    assert p.calls["add_phaser"] == [("g", 1.0, 0.0, 1.0, 4, 200.0, 2000.0, 1.0, 0.5, 0.25, "sine")]
    assert 'add_phaser("g", 1.0, 0.0, 1.0, 4, 200.0, 2000.0, 1.0, 0.5, 0.25, "sine");' in p.to_lua(str(tmp_path))


# ---- td_phaser_params ----
def test_phaser_params_match_the_formulas(api):
    """a_lo, a_hi against numpy's float64 tangent.  tan comes from the same libm on both sides here, but only correct rounding
    would make that a promise: the assertion is two ulp of the tangent carried through the quotient; am, ad, f and fb are IEEE
    operations on those and must agree to the bit."""
    worst = 0.0
    for sr in PP.RATES + (8000, 192000):
        for c in PP.grid_cases(sr) + [(6, 33.3, 0.31 * sr, 3.3, -0.31, 0.1, "sine")]:
            n, lo, hi, rate, fb = c[0], *(float(np.float32(v)) for v in c[1:5])
            N, a_lo, a_hi, am, ad, f, fbk = api.phaser_params(sr, *c)
            assert N == n and isinstance(N, int)
            for got, fc in ((a_lo, lo), (a_hi, hi)):
                t = np.tan(np.pi * fc / sr)
                want = (t - 1.0) / (t + 1.0)
                ulps = abs(got - float(want)) / np.spacing(abs(float(want)))
                worst = max(worst, ulps)
                assert ulps <= 4.0, (sr, c, got, want)
            assert am == 0.5 * (a_lo + a_hi) and ad == 0.5 * (a_hi - a_lo) and f == rate / sr and fbk == fb
            assert -1.0 < a_lo <= a_hi < 1.0 and ad >= 0.0
    print("phaser_params: worst disagreement with numpy %.3g ulp" % worst)


# ---- facts of the twin ----
def _spec(api, **kw):
    c = _args(**kw)
    return NP.spec(api.phaser_params(SR, *c), c[5], c[6])


def test_twin_static_chain_without_feedback_preserves_the_energy_of_a_burst(api):
    """lo_hz == hi_hz, feedback 0, wet 1: a chain of all-pass sections -- |H| = 1 at every frequency, so once the burst has rung
    out the output's energy is the input's."""
    rng = np.random.default_rng(5)
    x = np.zeros((6000, 2), np.float32)
    x[100:1100] = rng.uniform(-0.5, 0.5, (1000, 2)).astype(np.float32)
    for stages in (2, 4, 6, 8):
        v, end = NP.serial(x, _spec(api, stages=stages, lo_hz=1000.0, hi_hz=1000.0, feedback=0.0))
        ein, eout = (x.astype(np.float64) ** 2).sum(axis=0), (v ** 2).sum(axis=0)
        assert np.abs(end).max() < 1e-12   # (rung out)
        assert (np.abs(eout / ein - 1.0) <= 1e-9).all(), (stages, eout / ein)


def test_twin_two_stages_at_half_wet_cancel_a_steady_tone_at_the_centre(api):
    """Each section turns the phase by 90 degrees at fc = lo_hz = hi_hz: two of them by 180, p = -x, and the half-wet mix is 0."""
    fc = 1000.0
    n = np.arange(9600)
    tone = (0.5 * np.sin(2.0 * np.pi * fc * n / SR)).astype(np.float32)
    x = np.stack([tone, tone], axis=1)
    out, _ = NP.process(x, _spec(api, stages=2, lo_hz=fc, hi_hz=fc, feedback=0.0), wet=0.5)
    assert np.abs(out[4800:]).max() <= 1e-6 * 0.5 and np.abs(out[:50]).max() > 0.01   # (the transient has died by then)


def test_twin_stereo_zero_gives_equal_channels_for_equal_input(api):
    rng = np.random.default_rng(6)
    m = rng.uniform(-0.5, 0.5, 5000).astype(np.float32)
    x = np.stack([m, m], axis=1)
    v, end = NP.serial(x, _spec(api, stereo=0.0, feedback=0.9, rate_hz=20.0))
    assert np.array_equal(v[:, 0], v[:, 1]) and np.array_equal(end[:, 0], end[:, 1])
    w, _ = NP.serial(x, _spec(api, stereo=0.25, feedback=0.9, rate_hz=20.0))
    assert np.array_equal(w[:, 0], v[:, 0]) and np.abs(w[:, 1] - v[:, 1]).max() > 1e-3


def test_twin_without_feedback_n_stages_are_n_half_two_stage_vertices_in_series(api):
    """feedback 0: the chain is its sections in series, every one with the same a[n] -- to the f32 rounding between vertices."""
    rng = np.random.default_rng(7)
    x = rng.uniform(-0.5, 0.5, (6000, 2)).astype(np.float32)
    for stages in (4, 6, 8):
        p, _ = NP.process(x, _spec(api, stages=stages, feedback=0.0, rate_hz=5.0), processed=True)
        y = x
        for _ in range(stages // 2):
            y, _ = NP.process(y, _spec(api, stages=2, feedback=0.0, rate_hz=5.0), processed=True)
        assert np.abs(p.astype(np.float64) - y).max() <= stages * 2.0 ** -24 * np.abs(p).max(), stages


def test_twin_splits_give_the_one_piece_result_bitwise(api):
    rng = np.random.default_rng(8)
    x = rng.uniform(-0.5, 0.5, (6000, 2)).astype(np.float32)
    sp = _spec(api, stages=6, feedback=-0.8, rate_hz=7.0)
    whole, end = NP.process(x, sp, wet=0.7, gain=1.7, angle=30.0)
    for cut in (1, 777, 2048, 4999):
        a, st = NP.process(x[:cut], sp, wet=0.7, gain=1.7, angle=30.0)
        b, st = NP.process(x[cut:], sp, wet=0.7, gain=1.7, angle=30.0, state=st, t0=cut)
        assert np.array_equal(np.concatenate([a, b]).view(np.uint32), whole.view(np.uint32)) and np.array_equal(st, end), cut


# ---- the tiled scan restated ----
def _emulate(args):
    """One rate and input (a worker of its own: numpy only): the worst max|blocked - serial| / max|serial| (the end states
    included) and its case's index, the largest word of a prefix map, the largest output peak over the input's."""
    x, specs = args
    worst, maps, gain = (0.0, -1), {}, 0.0
    for N in (2, 4, 6, 8):
        idx = [i for i, s in enumerate(specs) if s[0][0] == N]
        sub = [specs[i] for i in idx]
        ser, end = NP.serial(x, sub)
        blk, endb = NP.blocked(x, sub, maps=maps)
        peak = np.abs(ser).max(axis=(1, 2))
        r = np.maximum(np.abs(blk - ser).max(axis=(1, 2)), np.abs(endb - end).max(axis=(1, 2))) / peak
        i = int(r.argmax())
        worst = max(worst, (float(r[i]), idx[i]))
        gain = max(gain, float((peak / np.abs(x).max()).max()))
    return worst, maps["peak"], gain


def test_blocked_scan_stays_inside_the_committed_constant(api):
    """E = 8 x the worst max|blocked - serial| / max|serial| of the numpy emulation over the GPU test's own grid and inputs at
    the three rates; this recomputes that worst figure and fails above E / 8.  Also printed: the largest word of a prefix map and
    the largest output peak over the input's (the scan is well conditioned: nothing grows)."""
    jobs, what = [], []
    for sr in PP.RATES:
        cases = PP.grid_cases(sr)
        assert len(cases) == 108
        specs = [PP.spec(api, sr, c) for c in cases]
        for kind in PP.INPUTS:
            x = oracle_input(kind, sr)
            assert len(x) > 5 * NP.TILE and np.abs(x).max() > 0.05
            jobs.append((x, specs))
            what.append((cases, sr, kind))
    with multiprocessing.Pool(max(1, min(len(jobs), os.cpu_count() or 1))) as pool:
        results = pool.map(_emulate, jobs)
    worst, maps, gain, n = (0.0, None), {"peak": 0.0}, 0.0, 0
    for (w, peak, g), (cases, sr, kind) in zip(results, what):
        if w[0] > worst[0]:
            worst = (w[0], (cases[w[1]], sr, kind))
        maps["peak"], gain, n = max(maps["peak"], peak), max(gain, g), n + len(cases)
    print("blocked scan: %d cases, worst max|blocked - serial| / max|serial| %.3g at %s (E_EMULATED %.3g, E %.3g = 2^%.1f); prefix "
          "maps up to %.3g, output peaks up to %.3g x the input's" % (n, worst[0], worst[1], PP.E_EMULATED, PP.E, math.log2(PP.E), maps["peak"], gain))
    assert n == 3 * 3 * 108
    assert 0.0 < worst[0] <= PP.E_EMULATED and PP.E == 8 * PP.E_EMULATED and PP.E <= 2 ** -28


def test_blocked_scan_continues_from_a_carried_state(api):
    x = oracle_input("noise", SR)[:9000]
    sp = _spec(api, stages=8, feedback=0.9, rate_hz=3.0)
    v, end = NP.serial(x, sp)
    for cut in (1, 777, 2048, 4999):
        a, st = NP.blocked(x[:cut], sp)
        b, st = NP.blocked(x[cut:], sp, state=st, t0=cut)
        assert np.abs(np.concatenate([a, b]) - v).max() <= PP.E_EMULATED * np.abs(v).max()
        assert np.abs(st - end).max() <= PP.E_EMULATED * np.abs(v).max()


# ---- the host engine under sanitizers ----
@pytest.fixture(scope="module")
def asan_exe(tmp_path_factory):
    return fx_rig.asan_exe(tmp_path_factory, "asan_phaser", ["mock_phaser.cpp", "asan_comp.cpp"])


PHASER_LAUNCHES = ("k_phaser_local", "k_phaser_carry", "k_phaser_apply")


def test_phaser_projects_under_sanitizers(asan_exe, tmp_path):
    n = int(os.environ.get("TD_ASAN_PHASER_SEEDS", "32"))
    workers = max(1, min(8, os.cpu_count() or 1))
    seeds = list(range(n))
    base = str(tmp_path / "p")
    with multiprocessing.Pool(workers) as pool:
        lists = pool.map(PP.write_projects, [(base, seeds[i::workers]) for i in range(workers) if seeds[i::workers]])
    procs = [subprocess.Popen([asan_exe] + lst, env=dict(os.environ, **ENV), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for lst in lists]
    launches = vertices = carried = fresh = rejected = 0
    for p in procs:
        out, err = p.communicate(timeout=1800)
        assert p.returncode == 0, (out[-800:], err[-4000:])
        # (the driver is the compressor's, as it is: its summary calls the effect launches it counted "k_comp")
        tail = out.split("asan_comp done:")[1]
        launches += int(tail.split("k_comp launches ")[1].split()[0])
        vertices += int(tail.split("(")[1].split()[0])
        fresh += int(tail.split(" entered fresh")[0].split()[-1])
        carried += int(tail.split(" entered with carried state")[0].split()[-1])
        rejected += int(tail.split(" rejected refreshes")[0].split()[-1])
    # multi-chunk renders and block pulls enter with carried state; every project is within the ranges
    assert rejected == 0 and launches >= n // 2 and vertices >= launches and fresh > 0 and carried > 0, (rejected, launches, vertices, fresh, carried)
    print("asan_phaser: %d projects, %d launches, %d vertices (%d fresh, %d carried) clean" % (n, launches, vertices, fresh, carried))


def _guard_project(shape, seconds=0.5):
    p = W.ProjectScript(SR, 1024)
    p.set_length(seconds)
    p.assets["a"] = W.Asset(W.noise_int16(7, 9000))
    p.load_sample("a", "a", "")
    p.event_files["f"] = np.array([(0.01, 60.0, 0.8), (0.2, 60.0, 0.0), (0.25, 62.0, 0.6)], np.float32)
    p.load_midi_floww("f", "f")
    ph = ("c", 1.0, 0.0, 0.0 if shape == "band_dry" else 1.0, 4, 200.0, 2000.0, 1.0, 0.7, 0.25, "sine")
    if shape == "band_up":       # loop -> band-pass -> phaser
        p.add_sampleloop("s", 1.0, 0.0, "a")
        p.add_bandpass("b", 1.0, 0.0, 1.0, 300.0, 5000.0, True)
        p.add_phaser(*ph)
        p.connect("s", "b"); p.connect("b", "c"); p.set_output("c")
    elif shape == "band_down":   # loop -> phaser -> band-pass
        p.add_sampleloop("s", 1.0, 0.0, "a")
        p.add_phaser(*ph)
        p.add_bandpass("b", 1.0, 0.0, 1.0, 300.0, 5000.0, True)
        p.connect("s", "c"); p.connect("c", "b"); p.set_output("b")
    elif shape == "band_both":   # loop -> band-pass -> phaser -> band-pass
        p.add_sampleloop("s", 1.0, 0.0, "a")
        p.add_bandpass("b", 1.0, 0.0, 1.0, 300.0, 5000.0, True)
        p.add_phaser(*ph)
        p.add_bandpass("b2", 1.0, 0.0, 1.0, 300.0, 5000.0, True)
        p.connect("s", "b"); p.connect("b", "c"); p.connect("c", "b2"); p.set_output("b2")
    elif shape in ("band_dry", "band_plain"):   # loop -> band-pass -> a dry phaser / a Sum in its place
        p.add_sampleloop("s", 1.0, 0.0, "a")
        p.add_bandpass("b", 1.0, 0.0, 1.0, 300.0, 5000.0, True)
        if shape == "band_dry":
            p.add_phaser(*ph)
        else:
            p.add_sum("c", 1.0, 0.0)
        p.connect("s", "b"); p.connect("b", "c"); p.set_output("c")
    elif shape in ("sine_up", "one_tile", "mixed"):     # synth -> phaser (one_tile: a render of 2 048 frames)
        p.add_synth("y", 1.0, 0.0, "f", 0.4, 0.3, W.HIT_ADSR, 1.0, 0.8, W.NOTE_ADSR, 0.5, W.STD_ADSR)
        p.add_phaser(*ph)
        p.connect("y", "c")
        if shape == "mixed":     # ... and two more in the same level, one of another stage count
            p.add_phaser("c8", 1.0, 0.0, 1.0, 8, 200.0, 2000.0, 1.0, 0.7, 0.25, "sine")
            p.add_phaser("c4", 1.0, 0.0, 1.0, 4, 20.0, 2000.0, 2.0, -0.7, 0.0, "triangle")
            p.add_sum("m", 1.0, 0.0)
            p.connect("y", "c8"); p.connect("y", "c4")
            for v in ("c", "c8", "c4"):
                p.connect(v, "m")
        p.set_output("m" if shape == "mixed" else "c")
    else:                        # synth -> sum: the control
        p.add_synth("y", 1.0, 0.0, "f", 0.4, 0.3, W.HIT_ADSR, 1.0, 0.8, W.NOTE_ADSR, 0.5, W.STD_ADSR)
        p.add_sum("c", 1.0, 0.0)
        p.connect("y", "c"); p.set_output("c")
    return p


def test_guard_modes_keep_the_exact_forms_upstream_of_a_phaser(asan_exe, tmp_path):
    """band_mode 2 / sine_mode 2 (the driver's profiled render): the launch families each shape went through."""
    shapes = ("band_up", "band_down", "band_both", "band_dry", "band_plain", "sine_up", "sine_free", "mixed")
    projects = {s: _guard_project(s) for s in shapes}
    projects["one_tile"] = _guard_project("one_tile", seconds=0.04)
    assert projects["one_tile"].cs * 1024 == NP.TILE
    fams = _families(asan_exe, tmp_path, projects)
    exact = ("k_band_pass", "k_band_spec")
    up, down, both = fams["band_up"], fams["band_down"], fams["band_both"]
    assert "k_band_scan" not in up and any(k in up for k in exact), up
    assert "k_band_scan" in down and not any(k in down for k in exact), down
    assert "k_band_scan" in both and any(k in both for k in exact), both
    for f in (up, down, both):
        assert all(f.get(k) == 1 for k in PHASER_LAUNCHES), f
        assert [k for k in f if k.startswith("k_phaser")] == list(PHASER_LAUNCHES), f   # (and in this order)
    # wet < 0.0001 compiles to k_sum: the launch list of the project with a Sum in the phaser's place
    dry, plain = fams["band_dry"], fams["band_plain"]
    assert not any(k.startswith("k_phaser") for k in dry) and list(dry.items()) == list(plain.items()), (dry, plain)
    sup, sfree = fams["sine_up"], fams["sine_free"]
    assert "k_sine_probe" not in sup and "k_synth" in sup, sup
    assert "k_sine_probe" in sfree, sfree
    assert not any(k.startswith("k_phaser") for k in sfree), sfree
    # a chunk of one tile is k_phaser_apply alone; a level with two stage counts takes each step once per count
    assert [(k, v) for k, v in fams["one_tile"].items() if k.startswith("k_phaser")] == [("k_phaser_apply", 1)], fams["one_tile"]
    assert [(k, v) for k, v in fams["mixed"].items() if k.startswith("k_phaser")] == [(k, 2) for k in PHASER_LAUNCHES], fams["mixed"]


def test_projects_without_a_phaser_keep_their_launch_list(asan_exe, tmp_path):
    projects = {"drums": W.drum_project(seconds=0.5), "config2": W.config2(seconds=0.5, n_src=8), "config4": W.config4(seconds=0.5, depth=6)}
    fams = _families(asan_exe, tmp_path, projects)
    for name in projects:
        got = " ".join("%s=%d" % kv for kv in fams[name].items())
        assert not any(k.startswith("k_phaser") for k in fams[name]) and got == PARENT_LAUNCHES[name], (name, got)
