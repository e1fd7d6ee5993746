"""The saturator vertex without a GPU (td_graph_add_saturator): the engine's taps against the formula, their
frequency response, td_saturator_params against the formulas; the float64 twin (tests/np_saturator.py) split anywhere, on an
impulse, and on the aliasing case the vertex exists for; ranges, the Lua line and its dump; the host engine on random projects
with saturator vertices under AddressSanitizer / UBSan against launches that check every descriptor (tests/mock_sat.cpp,
tests/asan_fx.cpp); the guard's path gain and its backup of the line; and the launch lists of projects without the vertex."""
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
import np_saturator as NS  # noqa: E402
import sat_projects as SP  # noqa: E402
from fx_rig import ENV, driver_report, PARENT_LAUNCHES  # noqa: E402
FACTORS = (1, 2, 4, 8)


# ---- the taps ----
@pytest.mark.parametrize("R", FACTORS)
def test_taps_are_the_formula_symmetric_and_sum_to_one(api, R):
    h = api.saturator_taps(R)
    assert len(h) == 2 * NS.Z * R + 1
    assert np.abs(h - NS.taps_formula(R)).max() <= 1e-15
    assert np.abs(h - h[::-1]).max() <= 1e-15
    assert abs(float(np.sum(h.astype(np.longdouble))) - 1.0) <= 1e-15


def _response_db(h, f):
    """|H| in dB at the frequencies f, in cycles per oversampled sample."""
    k = np.arange(len(h))
    H = np.exp(-2j * np.pi * np.outer(f, k)) @ h
    return 20.0 * np.log10(np.maximum(np.abs(H), 1e-300))


@pytest.mark.parametrize("R", (2, 4, 8))
def test_frequency_response(api, R):
    """In units of sr: flat within 1e-4 dB up to 0.375, -1.03 dB at 20 / 48, at most -105 dB from 0.5 up."""
    h = api.saturator_taps(R)
    band = _response_db(h, np.linspace(0.0, 0.375, 1501) / R)
    at20 = float(_response_db(h, np.array([20.0 / 48.0 / R]))[0])
    stop = _response_db(h, np.linspace(0.5 / R, 0.5, 4001))
    print("R %d: pass band %+.2e .. %+.2e dB, %.3f dB at 20 / 48 sr, stop band %.1f dB" % (R, band.min(), band.max(), at20, stop.max()))
    assert np.abs(band).max() <= 1e-4
    assert abs(at20 - (-1.03)) <= 0.01
    assert stop.max() <= -105.0


# ---- td_saturator_params ----
@pytest.mark.parametrize("R", FACTORS)
def test_params_are_the_formulas(api, R):
    h = api.saturator_taps(R)
    for kind in NS.KINDS:
        for d, b, o in ((0.0, 0.0, 0.0), (12.0, 0.2, -3.0), (36.0, -0.5, 6.0), (-24.0, 1.0, 24.0), (48.0, -1.0, -48.0)):
            got = api.saturator_params(kind, R, d, b, o)
            want = NS.params(kind, R, d, b, o, h)
            assert got[3] == want[3] == (0 if R == 1 else 64) and got[4] == want[4] == (1.5 if kind == "cubic" else 1.0)
            for a, w in zip(got[:3], want[:3]):
                assert abs(a - w) <= 4e-16 * max(abs(w), 1e-300), (kind, R, d, b, o, got, want)
            assert abs(got[5] - want[5]) <= 1e-9 * want[5], (kind, R, d, b, o, got, want)
            # Hsat = g_out Hdown Lf g_in Hup: the product of the two branch gains is essentially 1, not R
            hh = got[5] / (got[1] * got[4] * got[0])
            assert (hh == 1.0) if R == 1 else (1.0 <= hh <= 1.0001), (R, hh)
    if R > 1:
        print("R %d: Hup Hdown = %.9f" % (R, NS.branch_gain(h, R, 1.0) * NS.branch_gain(h, R, float(R))))


# ---- the twin ----
def _noise(n, seed=3, amp=0.8):
    rng = np.random.default_rng(seed)
    return (amp * (2.0 * rng.random((n, 2)) - 1.0)).astype(np.float32)


@pytest.mark.parametrize("R", (2, 4, 8))
def test_twin_split_anywhere_is_the_one_piece_result(api, R):
    h = api.saturator_taps(R)
    x = _noise(3000)
    x[100, 0] = np.inf
    x[1356, 1] = np.nan
    k = ("cubic", R, 12.0, 0.2, -3.0)
    whole, line = NS.saturator(x, *k, h=h)
    for cut in (1, 63, 64, 65, 200, 333, 1357):
        a, la = NS.saturator(x[:cut], *k, h=h)
        b, lb = NS.saturator(x[cut:], *k, h=h, line=la)
        got = np.concatenate([a, b])
        assert np.array_equal(np.isfinite(got), np.isfinite(whole)), cut
        ok = np.isfinite(whole)
        assert np.array_equal(got[ok].view(np.uint32), whole[ok].view(np.uint32)), cut
        assert np.array_equal(lb.view(np.uint32), line.view(np.uint32)), cut
    assert np.array_equal(line.view(np.uint32), x[-NS.LINE:].view(np.uint32))
    # the non-finite samples come out once, 64 frames later
    assert np.argwhere(~np.isfinite(whole)).tolist() == [[164, 0], [1420, 1]]


@pytest.mark.parametrize("R", (2, 4, 8))
def test_twin_impulse_is_the_two_filters_in_a_row(api, R):
    """A small impulse through `soft` (f(u) = u - u |u| + ..: linear to 1e-4 here) comes out as (R h) * h decimated, its peak at
    +64 frames."""
    h = api.saturator_taps(R)
    x = np.zeros((400, 2), np.float32)
    x[100, 0] = 1e-4
    g_in, g_out, fb = 1.0, 1.0, 0.0
    p, xd, _ = NS.process(x, "soft", R, g_in, 0.0, fb, g_out, h)
    hh = np.convolve(R * h, h)[::R]   # y[n] = sum_m hh[(n - 100) R - m ..]: the sample at oversampled index (n - 100) R
    want = np.zeros(400)
    want[100:100 + len(hh)] = 1e-4 * hh
    assert np.abs(p[:, 0].astype(np.float64) - want).max() <= 2e-4 * 1e-4   # (soft's curvature at 1e-4, and the f32 rounding)
    assert int(np.argmax(np.abs(p[:, 0]))) == 100 + NS.LATENCY and not p[:, 1].any()
    assert xd[100 + NS.LATENCY, 0] == np.float32(1e-4) and np.count_nonzero(xd) == 1


def _alias_db(api, R):
    """A 9 kHz sine at 48 kHz, amplitude 0.5, hard-clipped at +12 dB: the 21 kHz line (the third harmonic, folded) relative to the
    9 kHz line, from frames 2 048 .. 6 143 under a Hann window, the largest of the +-3 bins round each line."""
    t = np.arange(8192)
    s = (0.5 * np.sin(2.0 * np.pi * 9000.0 * t / 48000.0)).astype(np.float32)
    x = np.stack([s, s], axis=1)
    h = api.saturator_taps(R) if R > 1 else None
    g_in, g_out, fb = api.saturator_params("hard", R, 12.0, 0.0, 0.0)[:3]
    p, _, _ = NS.process(x, "hard", R, g_in, 0.0, fb, g_out, h)
    n = 4096
    w = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n) / n)
    sp = np.abs(np.fft.rfft(p[2048:2048 + n, 0].astype(np.float64) * w))

    def line(hz):
        b = int(round(hz * n / 48000.0))
        return sp[b - 3:b + 4].max()
    return 20.0 * math.log10(line(21000.0) / line(9000.0))


def test_oversampling_removes_the_folded_third_harmonic(api):
    db = {R: _alias_db(api, R) for R in FACTORS}
    print("21 kHz alias of a clipped 9 kHz tone, relative to the tone: " + ", ".join("R %d %.1f dB" % kv for kv in db.items()))
    assert db[1] >= -20.0
    assert db[4] <= -55.0
    assert db[8] <= -63.0
    assert db[2] < db[1] - 30.0


# ---- ranges ----
GOOD = dict(kind=1, drive_db=12.0, bias=0.2, out_db=-3.0, oversample=4)
NAN, INF = float("nan"), float("inf")
BAD = [("kind", -1), ("kind", 3), ("oversample", 0), ("oversample", 3), ("oversample", 16), ("oversample", -2),
       ("drive_db", -24.5), ("drive_db", 48.5), ("drive_db", NAN), ("drive_db", INF),
       ("bias", -1.01), ("bias", 1.01), ("bias", NAN),
       ("out_db", -48.5), ("out_db", 24.5), ("out_db", NAN), ("out_db", -INF)]


def _args(**kw):
    d = dict(GOOD, **kw)
    return d["kind"], d["drive_db"], d["bias"], d["out_db"], d["oversample"]


@pytest.mark.parametrize("name,value", BAD)
def test_out_of_range_parameters_are_rejected_by_name(api, name, value):
    g = api.Graph(64, 48000)
    with pytest.raises(api.TermdawError, match=name):
        g.add_saturator("w", 1.0, 0.0, 1.0, *_args(**{name: value}))
    k, d, b, o, R = _args(**{name: value})
    with pytest.raises(api.TermdawError, match=name):
        api.saturator_params(k, R, d, b, o)
    g.add_sum("in", 1.0, 0.0)
    assert not g.set_output("w")   # (nothing was added)


def test_taps_of_another_factor_are_rejected(api):
    assert api.lib().td_saturator_taps(3, None, 0) == 0 and "oversample" in api.last_error()


def test_range_ends_are_accepted_and_wet_is_clamped(api):
    g = api.Graph(64, 48000)
    g.add_sum("in", 1.0, 0.0)
    for i, a in enumerate(((0, -24.0, -1.0, -48.0, 1), (2, 48.0, 1.0, 24.0, 8))):
        g.add_saturator("w%d" % i, 1.0, 0.0, 1.0, *a)
    g.add_saturator("wet", 1.0, 0.0, 7.0, *_args())   # (wet is clamped, not rejected: graph.rs:256)
    g.add_saturator("dry", 1.0, 0.0, -3.0, *_args())
    g.add_saturator("named", 1.0, 0.0, 1.0, "soft", 0.0, 0.0, 0.0, 2)
    assert g.connect("in", "w1") and g.set_output("w1") and g.check_graph()
    assert g.device_bytes() == 0   # (the line is allocated when the vertex is first rendered)


def _lua(line):
    return fx_rig._lua(line, "w")


LUA_BAD = [(k, v) for k, v in BAD if k != "kind" and math.isfinite(v)]


@pytest.mark.parametrize("name,value", LUA_BAD)
def test_lua_rejects_the_same_ranges(api, name, value):
    s = api.State("", 48000, 64)
    _, d, b, o, R = _args(**{name: value})
    assert not s.refresh(_lua('add_saturator("w", 1.0, 0.0, 1.0, "cubic", %r, %r, %r, %r);' % (d, b, o, R)))
    assert name in api.last_error() and "line 2" in api.last_error(), api.last_error()


def test_lua_rejects_an_unknown_kind(api):
    s = api.State("", 48000, 64)
    assert not s.refresh(_lua('add_saturator("w", 1.0, 0.0, 1.0, "tanh", 0, 0, 0, 2);'))
    assert "kind" in api.last_error() and "line 2" in api.last_error(), api.last_error()


def test_lua_accepts_and_dumps_the_canonical_line(api):
    s = api.State("", 48000, 64)
    assert s.refresh(_lua('add_saturator("w", 0.5, -30, 1, "soft", 1, 0.5, -30, 4);')), api.last_error()
    dump = s.dump_calls()
    band = api.State("", 48000, 64)
    assert band.refresh('add_sum("in", 1.0, 0.0);\nadd_bandpass("b", 0.5, -30, 1, 100.5, 4, true);\nconnect("in", "b");\nset_output("b");\n'), api.last_error()
    # the numbers print as add_bandpass prints the same values
    half, m30, one = band.dump_calls().split('add_bandpass("b",')[1].split(")")[0].split(",")[:3]
    line = [ln for ln in dump.splitlines() if ln.startswith("add_saturator(")]
    assert len(line) == 1
    args = line[0][len("add_saturator("):-1].split(",")
    assert args == ['"w"', half, m30, one, '"soft"', one, half, m30, "4"] and " " not in line[0], line
    # ... and the dumped line is a project line again: it round-trips
    again = api.State("", 48000, 64)
    assert again.refresh(_lua(line[0] + ";")), api.last_error()
    assert [ln for ln in again.dump_calls().splitlines() if ln.startswith("add_saturator(")] == line


def test_project_script_records_and_writes_the_call(tmp_path):
    p = W.ProjectScript(48000, 64)
    p.add_sum("in", 1.0, 0.0)
    p.add_saturator("w", 1.0, 0.0, 1.0, "hard", 12.0, 0.25, -3.0, 8)
    p.connect("in", "w")
    p.set_output("w")
    assert p.calls["add_saturator"] == [("w", 1.0, 0.0, 1.0, "hard", 12.0, 0.25, -3.0, 8)]
    assert 'add_saturator("w", 1.0, 0.0, 1.0, "hard", 12.0, 0.25, -3.0, 8);' in p.to_lua(str(tmp_path))


# ---- the host engine under sanitizers ----


@pytest.fixture(scope="module")
def asan_exe(tmp_path_factory):
    return fx_rig.asan_exe(tmp_path_factory, "asan_sat", ["mock_guard.cpp", "mock_sat.cpp", "asan_fx.cpp"])


def test_saturator_projects_under_sanitizers(asan_exe, tmp_path):
    n = int(os.environ.get("TD_ASAN_SAT_SEEDS", "32"))
    workers = max(1, min(8, os.cpu_count() or 1))
    seeds = list(range(n))
    base = str(tmp_path / "p")
    with multiprocessing.Pool(workers) as pool:
        lists = pool.map(SP.write_projects, [(base, seeds[i::workers]) for i in range(workers) if seeds[i::workers]])
    procs = [subprocess.Popen([asan_exe] + lst, env=dict(os.environ, **ENV), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for lst in lists]
    tot = dict(sat=0, vertices=0, single=0, fresh=0, carried=0, summed=0, sat1=0, rejected=0, restarts=0, short=0)
    for p in procs:
        out, err = p.communicate(timeout=1800)
        assert p.returncode == 0, (out[-800:], err[-4000:])
        tail = out.split("asan_sat done:")[1]
        tot["sat"] += int(tail.split("k_sat launches ")[1].split()[0])
        tot["vertices"] += int(tail.split("(")[1].split()[0])
        tot["single"] += int(tail.split(" one-launch")[0].split()[-1])
        tot["fresh"] += int(tail.split(" entered fresh")[0].split()[-1])
        tot["carried"] += int(tail.split(" entered with the line")[0].split()[-1])
        tot["summed"] += int(tail.split(" k_sat_sum launches")[0].split()[-1])
        tot["sat1"] += int(tail.split(" k_sat1 launches")[0].split()[-1])
        tot["restarts"] += int(tail.split(" restarts checked")[0].split()[-1])
        tot["short"] += int(tail.split(" short chunks")[0].split()[-1])
        tot["rejected"] += int(tail.split(" rejected refreshes")[0].split()[-1])
    # multi-chunk renders and block pulls enter with the line (the mock checks `filled` and the parity of every one of them); short
    # chunks and block pulls take one launch, long chunks two; blocks below 128 frames are chunks shorter than the line
    assert tot["rejected"] == 0 and tot["sat"] >= n // 2 and tot["vertices"] >= tot["sat"], tot
    assert tot["fresh"] > 0 and tot["carried"] > 0 and tot["single"] > 0 and 0 < tot["summed"] <= tot["sat"] and tot["sat1"] > 0, tot
    # the pull right behind a set_time entered with nothing of its line, for every vertex the mock saw there (it aborts otherwise)
    assert tot["restarts"] > 0 and tot["short"] > 0, tot
    print("asan_sat: %d projects clean: %s" % (n, tot))


SAT = ("cubic", 6.0, 0.1, -3.0, 4)


def _guard_project(shape, wet=0.75, bl=1024):
    return fx_rig.guard_project(shape, lambda p, name, dry: p.add_saturator(name, 1.0, 0.0, 0.00009 if dry else wet, *SAT), name="e", bl=bl)


def test_guard_modes_carry_the_estimate_through_a_saturator(api, asan_exe, tmp_path):
    """band_mode 2 / sine_mode 2 (the driver's profiled render): upstream of a saturator the scan / fast forms stay, and the
    guard's estimate at the output is the one of the same project without the vertex times (1 - wet) + wet Hsat."""
    shapes = ("band_up", "band_plain", "band_dry", "sine_up", "sine_free")
    fams, gains, _ = driver_report(asan_exe, tmp_path, {s: _guard_project(s) for s in shapes})
    exact = ("k_band_pass", "k_band_spec")
    for s in ("band_up", "band_plain", "band_dry"):
        assert "k_band_scan" in fams[s] and not any(k in fams[s] for k in exact), (s, fams[s])
    # 0.5 s in one chunk: two launches
    assert [k for k in fams["band_up"] if k.startswith("k_sat")] == ["k_sat_sum", "k_sat"] and fams["band_up"]["k_sat"] == 1, fams["band_up"]
    # wet < 0.0001 compiles to k_sum: the launch list of the project with a Sum in the saturator's place
    assert not any(k.startswith("k_sat") for k in fams["band_dry"]) and list(fams["band_dry"].items()) == list(fams["band_plain"].items()), (fams["band_dry"], fams["band_plain"])
    for s in ("sine_up", "sine_free"):
        assert "k_sine_probe" in fams[s], (s, fams[s])
    assert fams["sine_up"].get("k_sat") == 1 and not any(k.startswith("k_sat") for k in fams["sine_free"])
    # the path gain: the driver prints the audit's gain from the band-pass vertex to the output (AuditHead)
    hsat = api.saturator_params(SAT[0], SAT[4], SAT[1], SAT[2], SAT[3])[5]
    want = (1.0 - 0.75) + 0.75 * hsat
    assert 1.5 * 10.0 ** (3.0 / 20.0) <= hsat <= 1.5 * 10.0 ** (3.0 / 20.0) * 1.0001   # Lf g_in g_out, and Hup Hdown just above 1
    assert gains["band_plain"]["path"] > 0.0
    assert abs(gains["band_up"]["path"] / gains["band_plain"]["path"] - want) < 1e-6 * want, (gains, want)
    assert abs(gains["band_dry"]["path"] / gains["band_plain"]["path"] - 1.0) < 1e-6, gains


def test_a_guarded_pull_that_runs_again_enters_with_the_line_it_first_entered_with(asan_exe, tmp_path):
    """Three guarded block pulls, each told to run again (mock_sat.cpp): the first starts afresh both times and reads nothing of
    the line; the second and the third continue from it, so the guard copies both halves in front of the pull and puts them -- and
    the parity and the frame count on the host -- back in front of the second run: both runs find the same stamp in the same
    half, the one the run before them left last."""
    _, _, redo = driver_report(asan_exe, tmp_path, {"band_up": _guard_project("band_up"), "band_plain": _guard_project("band_plain")})
    assert int(redo["band_up"]["redos"]) == 3 and int(redo["band_plain"]["redos"]) == 3, redo
    e = [int(v) for v in redo["band_up"]["entries"].split(",")]
    assert len(e) == 4 and e[0] == e[1] and e[2] == e[3] and e[2] == e[0] + 2, e
    assert redo["band_plain"].get("entries", "") == ""


def test_projects_without_a_saturator_keep_their_launch_list(asan_exe, tmp_path):
    """The launch lists of drum_project, config 2 and config 4 (families and launch counts of one profiled render under the
    front-end's guard modes) as the parent commit compiled them."""
    projects = {"drums": W.drum_project(seconds=0.5), "config2": W.config2(seconds=0.5, n_src=8), "config4": W.config4(seconds=0.5, depth=6)}
    fams, _, _ = driver_report(asan_exe, tmp_path, projects)
    for name in projects:
        got = " ".join("%s=%d" % kv for kv in fams[name].items())
        assert not any(k.startswith("k_sat") for k in fams[name]) and got == PARENT_LAUNCHES[name], (name, got)
