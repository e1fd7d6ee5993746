"""The feedback delay vertex without a GPU (td_graph_add_delay): td_delay_params against the formulas; the float64
twin (tests/np_delay.py) on an impulse against the closed form; ranges, the Lua line and its dump; the constant of the GPU test's
bound from the numpy emulation of the tiled scan; the host engine on random projects with delay vertices under AddressSanitizer /
UBSan against launches that check every descriptor (tests/mock_delay.cpp, tests/asan_fx.cpp); the guard's path gain and its
backup of the line; and the launch lists of projects without the vertex."""
import math
import multiprocessing
import os
import subprocess
import sys

import numpy as np
import pytest

from termdaw_amd import workloads as W

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import delay_projects as DP  # noqa: E402
import fx_rig  # noqa: E402
import np_delay as ND  # noqa: E402
from fx_rig import ENV, driver_report, PARENT_LAUNCHES, oracle_input  # noqa: E402


# ---- td_delay_params ----
D_WANT = {   # llround(time_ms sr / 1000) by hand: 7.3 ms is 321.93 / 350.4 / 700.8 frames, 375 ms at 44.1 kHz 16 537.5 (away from zero)
    44100: {1.0: 44, 7.3: 322, 30.0: 1323, 250.0: 11025, 375.0: 16538, 2000.0: 88200},
    48000: {1.0: 48, 7.3: 350, 30.0: 1440, 250.0: 12000, 375.0: 18000, 2000.0: 96000},
    96000: {1.0: 96, 7.3: 701, 30.0: 2880, 250.0: 24000, 375.0: 36000, 2000.0: 192000},
}


@pytest.mark.parametrize("sr", [44100, 48000, 96000])
def test_params_are_the_formulas(api, sr):
    for t, want in D_WANT[sr].items():
        for f, c in ((0.0, 0.0), (0.5, 0.35), (0.98, 1.0), (0.7, 0.5)):
            D, gs, gc, h = api.delay_params(sr, t, f, c)
            f64, c64 = float(np.float32(f)), float(np.float32(c))
            assert D == want == ND.params(sr, t, f, c)[0], (sr, t, D)
            assert gs == f64 * (1.0 - c64) and gc == f64 * c64 and h == 1.0 / (1.0 - f64)
            assert (D, gs, gc, h) == ND.params(sr, t, f, c)
            # G = [[gs, gc], [gc, gs]] is symmetric with eigenvalues feedback and feedback (1 - 2 cross): its 2-norm is feedback,
            # the echo path 1 + G + G^2 + .. has the L2 gain Hecho
            ev = np.linalg.eigvalsh(np.array([[gs, gc], [gc, gs]]))
            assert np.allclose(sorted(ev), sorted([f64, f64 * (1.0 - 2.0 * c64)]), atol=1e-15)
            assert abs(1.0 / (1.0 - max(abs(ev))) - h) <= 1e-12 * h


# ---- the twin ----
@pytest.mark.parametrize("cross", [0.0, 0.35, 1.0])
def test_twin_impulse_is_the_closed_form(cross):
    """A left-channel impulse: echoes at k D with the amplitude feedback^(k-1), split over the channels as the powers of
    [[1 - c, c], [c, 1 - c]] say; at c = 1 they strictly alternate."""
    D, f = 37, 0.6
    _, gs, gc, _ = ND.params(1000, float(D), f, cross)
    x = np.zeros((10 * D + 5, 2), np.float32)
    x[3, 0] = 1.0
    p, line = ND.delay(x, D, gs, gc, processed=True)
    c64, f64 = float(np.float32(cross)), float(np.float32(f))
    want = np.zeros(x.shape)
    want[3, 0] = 1.0
    P = np.array([[1.0 - c64, c64], [c64, 1.0 - c64]])
    for k in range(1, 11):
        if 3 + k * D < len(x):
            want[3 + k * D] = f64 ** (k - 1) * np.linalg.matrix_power(P, k - 1)[:, 0]
    assert np.abs(p - want).max() <= 4e-7, np.abs(p - want).max()
    nz = np.argwhere(np.abs(p) > 1e-12)
    assert set(int(i) for i in nz[:, 0]) <= {3 + k * D for k in range(11)}
    if cross == 1.0:   # left, left (the first echo is the input itself, delayed), right, left, right ..
        for k in range(2, 10):
            on, off = ((k - 1) % 2, k % 2)
            assert p[3 + k * D, on] > 0.0 and p[3 + k * D, off] == 0.0, k
    if cross == 0.0:
        assert not p[:, 1].any()
    assert line.shape == (D, 2)


def test_twin_split_anywhere_is_the_one_piece_result():
    rng = np.random.default_rng(4)
    x = rng.standard_normal((5000, 2)).astype(np.float32)
    D, gs, gc, _ = ND.params(48000, 7.3, 0.98, 0.35)
    whole, end = ND.delay(x, D, gs, gc, wet=0.7, gain=0.8, angle=20.0)
    for cuts in ((1, 349, 350, 351, 2000), (64, 128, 4999), (3000,)):
        parts, line, a = [], None, 0
        for b in list(cuts) + [len(x)]:
            y, line = ND.delay(x[a:b], D, gs, gc, wet=0.7, gain=0.8, angle=20.0, line=line)
            parts.append(y)
            a = b
        assert np.array_equal(np.concatenate(parts).view(np.uint32), whole.view(np.uint32)) and np.array_equal(line, end)


def test_twin_keeps_non_finite_frames_out_of_the_line():
    rng = np.random.default_rng(5)
    x = rng.standard_normal((2000, 2)).astype(np.float32)
    x[100, 0], x[300, 1] = np.inf, np.nan
    D, gs, gc, _ = ND.params(48000, 1.0, 0.98, 0.35)
    p, line = ND.delay(x, D, gs, gc, processed=True)
    assert (np.isfinite(p) == np.isfinite(x)).all() and np.isfinite(line).all()
    clean = x.copy()
    clean[100, 0] = clean[300, 1] = 0.0
    q, _ = ND.delay(clean, D, gs, gc, processed=True)
    ok = np.isfinite(x)
    assert np.array_equal(p[ok], q[ok])


def test_the_emulation_is_the_serial_result_on_one_lane_set():
    """np_delay.blocked against np_delay.echo with a carried line and every tile length."""
    rng = np.random.default_rng(6)
    x = rng.standard_normal((30000, 2)).astype(np.float32)
    D, gs, gc, _ = ND.params(48000, 1.0, 0.98, 0.25)
    _, line = ND.echo(x[:777], D, gs, gc)
    ser, _ = ND.echo(x, D, gs, gc, line=line)
    for T in ND.TILES:
        b = ND.blocked(x, D, gs, gc, T, line=line)
        assert np.abs(b - ser).max() <= 1e-13 * np.abs(ser).max(), T
    assert ND.tiling(len(x), D, 8)[2] > 1 and ND.tiling(len(x), D, 64)[2] == 1   # (the carry with and without several threads per lane)


# ---- ranges ----
GOOD = dict(time_ms=250.0, feedback=0.5, cross=0.35)
BAD = [("time_ms", 0.99), ("time_ms", 2000.5), ("time_ms", -1.0), ("time_ms", float("nan")), ("time_ms", float("inf")),
       ("feedback", -0.01), ("feedback", 0.981), ("feedback", 1.0), ("feedback", float("nan")),
       ("cross", -0.01), ("cross", 1.01), ("cross", float("nan"))]


def _args(**kw):
    d = dict(GOOD, **kw)
    return d["time_ms"], d["feedback"], d["cross"]


@pytest.mark.parametrize("name,value", BAD)
def test_out_of_range_parameters_are_rejected_by_name(api, name, value):
    g = api.Graph(64, 48000)
    with pytest.raises(api.TermdawError, match=name):
        g.add_delay("d", 1.0, 0.0, 1.0, *_args(**{name: value}))
    with pytest.raises(api.TermdawError, match=name):
        api.delay_params(48000, *_args(**{name: value}))
    g.add_sum("in", 1.0, 0.0)
    assert not g.set_output("d")   # (nothing was added)


def test_range_ends_are_accepted_and_wet_is_clamped(api):
    g = api.Graph(64, 48000)
    g.add_sum("in", 1.0, 0.0)
    for i, (t, f, c) in enumerate(((1.0, 0.0, 0.0), (2000.0, 0.98, 1.0))):
        g.add_delay("d%d" % i, 1.0, 0.0, 1.0, t, f, c)
    g.add_delay("wet", 1.0, 0.0, 7.0, *_args())   # (wet is clamped, not rejected: graph.rs:256)
    g.add_delay("dry", 1.0, 0.0, -3.0, *_args())
    assert g.connect("in", "d1") and g.set_output("d1") and g.check_graph()
    assert g.device_bytes() == 0   # (the line is allocated when the vertex is first rendered)


def _lua(line):
    return fx_rig._lua(line, "d")


@pytest.mark.parametrize("name,value", [(k, v) for k, v in BAD if math.isfinite(v)])
def test_lua_rejects_the_same_ranges(api, name, value):
    s = api.State("", 48000, 64)
    t, f, c = _args(**{name: value})
    assert not s.refresh(_lua('add_delay("d", 1.0, 0.0, 1.0, %r, %r, %r);' % (t, f, c)))
    assert name in api.last_error() and "line 2" in api.last_error(), api.last_error()


def test_lua_accepts_and_dumps_the_canonical_line(api):
    s = api.State("", 48000, 64)
    assert s.refresh(_lua('add_delay("d", 0.5, -30, 1, 100.5, 0.5, 1);')), api.last_error()
    dump = s.dump_calls()
    band = api.State("", 48000, 64)
    assert band.refresh('add_sum("in", 1.0, 0.0);\nadd_bandpass("b", 0.5, -30, 1, 100.5, 4, true);\nconnect("in", "b");\nset_output("b");\n'), api.last_error()
    # the numbers print as add_bandpass prints the same values
    half, m30, one, x1005 = band.dump_calls().split('add_bandpass("b",')[1].split(")")[0].split(",")[:4]
    line = [ln for ln in dump.splitlines() if ln.startswith("add_delay(")]
    assert len(line) == 1
    args = line[0][len("add_delay("):-1].split(",")
    assert args == ['"d"', half, m30, one, x1005, half, one] and " " not in line[0], line
    # ... and the dumped line is a project line again: it round-trips
    again = api.State("", 48000, 64)
    assert again.refresh(_lua(line[0] + ";")), api.last_error()
    assert [ln for ln in again.dump_calls().splitlines() if ln.startswith("add_delay(")] == line


def test_project_script_records_and_writes_the_call(tmp_path):
    p = W.ProjectScript(48000, 64)
    p.add_sum("in", 1.0, 0.0)
    p.add_delay("d", 1.0, 0.0, 1.0, 375.0, 0.5, 1.0)
    p.connect("in", "d")
    p.set_output("d")
    assert p.calls["add_delay"] == [("d", 1.0, 0.0, 1.0, 375.0, 0.5, 1.0)]
    assert 'add_delay("d", 1.0, 0.0, 1.0, 375.0, 0.5, 1.0);' in p.to_lua(str(tmp_path))


# ---- the bound of tests/test_gpu_delay.py ----
def test_the_emulated_scan_stays_inside_the_committed_constant():
    """E = 8 x the worst max|blocked - serial| / max|serial| of the numpy emulation over the GPU test's own grid and inputs, with
    every candidate tile length; this recomputes that worst figure and fails above E / 8.  Also: no float32 value of the grid
    changes, and every grid case moves its input by far more than the bound (so the GPU test cannot pass on a vertex that does
    nothing)."""
    worst, weakest, changed, multi = (0.0, None), (9e9, None), 0, 0
    for sr in DP.RATES:
        for kind in DP.INPUTS:
            x = oracle_input(kind, sr)
            assert np.abs(x).max() > 0.05
            for t, f, c in DP.grid_cases(sr):
                D, gs, gc, _ = ND.params(sr, t, f, c)
                ser, _ = ND.echo(x, D, gs, gc)
                peak = np.abs(ser).max()
                for T in ND.TILES:
                    if ND.tiling(len(x), D, T)[1] == 1:
                        continue   # (one tile: the single-launch form, nothing re-associated)
                    b = ND.blocked(x, D, gs, gc, T)
                    multi += 1
                    r = float(np.abs(b - ser).max() / peak)
                    changed += int((b.astype(np.float32) != ser.astype(np.float32)).sum())
                    if r > worst[0]:
                        worst = (r, (t, f, c, sr, kind, T))
                acts = float(np.abs(ser - x.astype(np.float64)).max() / (peak * (2.0 ** -23 + DP.E)))
                if acts < weakest[0]:
                    weakest = (acts, (t, f, c, sr, kind))
    print("emulated scan, %d runs: worst %.3g = 2^%.1f of the peak at %s; %d float32 values changed; the weakest case moves its input "
          "by %.3g bounds (%s)" % (multi, worst[0], math.log2(worst[0]), worst[1], changed, weakest[0], weakest[1]))
    assert multi > 500
    assert 0.0 < worst[0] <= DP.E_EMULATED and DP.E == 8.0 * DP.E_EMULATED and DP.E <= 2.0 ** -28
    assert changed == 0
    assert weakest[0] > 64.0


# ---- the host engine under sanitizers ----


@pytest.fixture(scope="module")
def asan_exe(tmp_path_factory):
    return fx_rig.asan_exe(tmp_path_factory, "asan_delay", ["mock_guard.cpp", "mock_delay.cpp", "asan_fx.cpp"])


def test_delay_projects_under_sanitizers(asan_exe, tmp_path):
    n = int(os.environ.get("TD_ASAN_DELAY_SEEDS", "32"))
    workers = max(1, min(8, os.cpu_count() or 1))
    seeds = list(range(n))
    base = str(tmp_path / "p")
    with multiprocessing.Pool(workers) as pool:
        lists = pool.map(DP.write_projects, [(base, seeds[i::workers]) for i in range(workers) if seeds[i::workers]])
    procs = [subprocess.Popen([asan_exe] + lst, env=dict(os.environ, **ENV), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for lst in lists]
    tot = dict(apply=0, vertices=0, single=0, fresh=0, carried=0, local=0, rejected=0, restarts=0)
    for p in procs:
        out, err = p.communicate(timeout=1800)
        assert p.returncode == 0, (out[-800:], err[-4000:])
        tail = out.split("asan_delay done:")[1]
        tot["apply"] += int(tail.split("k_delay_apply launches ")[1].split()[0])
        tot["vertices"] += int(tail.split("(")[1].split()[0])
        tot["single"] += int(tail.split(" single-launch")[0].split()[-1])
        tot["fresh"] += int(tail.split(" entered fresh")[0].split()[-1])
        tot["carried"] += int(tail.split(" entered with the line")[0].split()[-1])
        tot["local"] += int(tail.split(" k_delay_local launches")[0].split()[-1])
        tot["restarts"] += int(tail.split(" restarts checked")[0].split()[-1])
        tot["rejected"] += int(tail.split(" rejected refreshes")[0].split()[-1])
    # multi-chunk renders and block pulls enter with the line; short delays take three launches, long ones and block pulls one
    assert tot["rejected"] == 0 and tot["apply"] >= n // 2 and tot["vertices"] >= tot["apply"], tot
    assert tot["fresh"] > 0 and tot["carried"] > 0 and tot["single"] > 0 and 0 < tot["local"] < tot["apply"], tot
    # the pull right behind a set_time entered with nothing of its line, for every vertex the mock saw there (it aborts otherwise)
    assert tot["restarts"] > 0, tot
    print("asan_delay: %d projects clean: %s" % (n, tot))


def _guard_project(shape, wet=0.75, feedback=0.5):
    """(10 ms are 480 frames: below the block length)"""
    return fx_rig.guard_project(shape, lambda p, name, dry: p.add_delay(name, 1.0, 0.0, 0.00009 if dry else wet, 10.0, feedback, 0.35), name="e")


DELAY_LAUNCHES = ("k_delay_local", "k_delay_carry", "k_delay_apply")


def test_guard_modes_carry_the_estimate_through_a_delay(api, asan_exe, tmp_path):
    """band_mode 2 / sine_mode 2 (the driver's profiled render): upstream of a delay the scan / fast forms stay, and the guard's
    estimate at the output is the one of the same project without the delay times 1 + wet Hecho."""
    shapes = ("band_up", "band_plain", "band_dry", "sine_up", "sine_free")
    fams, gains, _ = driver_report(asan_exe, tmp_path, {s: _guard_project(s) for s in shapes})
    exact = ("k_band_pass", "k_band_spec")
    for s in ("band_up", "band_plain", "band_dry"):
        assert "k_band_scan" in fams[s] and not any(k in fams[s] for k in exact), (s, fams[s])
    # 0.5 s at 10 ms: 50 steps, four tiles of 16 -- three launches
    assert [k for k in fams["band_up"] if k.startswith("k_delay")] == list(DELAY_LAUNCHES) and all(fams["band_up"][k] == 1 for k in DELAY_LAUNCHES), fams["band_up"]
    # wet < 0.0001 compiles to k_sum: the launch list of the project with a Sum in the delay's place
    assert not any(k.startswith("k_delay") for k in fams["band_dry"]) and list(fams["band_dry"].items()) == list(fams["band_plain"].items()), (fams["band_dry"], fams["band_plain"])
    for s in ("sine_up", "sine_free"):
        assert "k_sine_probe" in fams[s], (s, fams[s])
    assert all(fams["sine_up"].get(k) == 1 for k in DELAY_LAUNCHES) and not any(k.startswith("k_delay") for k in fams["sine_free"])
    # the path gain: the driver prints the audit's gain from the band-pass vertex to the output (AuditHead)
    hecho = api.delay_params(48000, 10.0, 0.5, 0.35)[3]
    assert hecho == 2.0
    want = 1.0 + 0.75 * hecho
    assert gains["band_plain"]["path"] > 0.0
    assert abs(gains["band_up"]["path"] / gains["band_plain"]["path"] - want) < 1e-6 * want, (gains, want)
    assert abs(gains["band_dry"]["path"] / gains["band_plain"]["path"] - 1.0) < 1e-6, gains


def test_a_guarded_pull_that_runs_again_enters_with_the_line_it_first_entered_with(asan_exe, tmp_path):
    """Three guarded block pulls, each told to run again (mock_delay.cpp): the first starts afresh both times and reads nothing of
    the line; the second and the third continue from it, so the guard copies it in front of the pull and puts it back in front
    of the second run -- both runs find the same stamp, the one the run before them left last."""
    _, _, redo = driver_report(asan_exe, tmp_path, {"band_up": _guard_project("band_up"), "band_plain": _guard_project("band_plain")})
    assert int(redo["band_up"]["redos"]) == 3 and int(redo["band_plain"]["redos"]) == 3, redo
    e = [int(v) for v in redo["band_up"]["entries"].split(",")]
    assert len(e) == 4 and e[0] == e[1] and e[2] == e[3] and e[2] == e[0] + 2, e
    assert redo["band_plain"].get("entries", "") == ""


def test_projects_without_a_delay_keep_their_launch_list(asan_exe, tmp_path):
    """The launch lists of drum_project, config 2 and config 4 (families and launch counts of one profiled render under the
    front-end's guard modes) as the parent commit compiled them."""
    projects = {"drums": W.drum_project(seconds=0.5), "config2": W.config2(seconds=0.5, n_src=8), "config4": W.config4(seconds=0.5, depth=6)}
    fams, _, _ = driver_report(asan_exe, tmp_path, projects)
    for name in projects:
        got = " ".join("%s=%d" % kv for kv in fams[name].items())
        assert not any(k.startswith("k_delay") for k in fams[name]) and got == PARENT_LAUNCHES[name], (name, got)
