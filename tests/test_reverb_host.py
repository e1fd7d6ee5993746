"""The reverb vertex without a GPU (td_graph_add_reverb): td_reverb_params against the formulas; the float64 twin
(tests/np_reverb.py) split anywhere, its impulse response (the 8 comb delays, an undamped decay of g per pass) and its L2 gain
against the guard's bound Hrev; the constant of the GPU test's bound from the numpy emulation of the windowed scan; ranges, the Lua
line and its dump; the host engine on random projects with reverb vertices under AddressSanitizer / UBSan against launches that
check every descriptor (tests/mock_reverb.cpp, tests/asan_fx.cpp); the guard's path gain and its backup of the state block; and
the launch lists of projects without the vertex."""
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
import np_reverb as NR  # noqa: E402
import reverb_projects as RP  # noqa: E402
from fx_rig import ENV, driver_report, PARENT_LAUNCHES, oracle_input  # noqa: E402
SR = 48000


# ---- td_reverb_params ----
def test_params_are_the_formulas(api):
    for sr in (44100, 48000, 96000):
        for c in RP.grid_cases() + [(1.0, 0.0, 1.0, 2.0), (0.25, 0.75, 0.1, 0.77)]:
            got, want = api.reverb_params(sr, *c), NR.params(sr, *c)
            assert got == want, (sr, c, got, want)
            assert got["d2"] == 1.0 - got["d1"] and got["w1"] + got["w2"] == 1.0
            assert got["Hrev"] == 0.03 * (8.0 / (1.0 - got["g"])) * ((5.0 / 3.0) ** 2) ** 2
            assert got["B"] in NR.BLOCKS and got["B"] <= min(NR.lengths(got)) and (got["B"] == 256 or 2 * got["B"] > min(NR.lengths(got)))
    # the figures the definition quotes: the tunings themselves at 44.1 kHz and size 1, the right channel 23 frames longer
    k = api.reverb_params(44100, 0.5, 0.5, 1.0, 1.0)
    assert k["combs_l"] == list(NR.COMBS) and k["allpass_l"] == list(NR.ALLPASS)
    assert k["combs_r"] == [t + 23 for t in NR.COMBS] and k["allpass_r"] == [t + 23 for t in NR.ALLPASS]
    assert (k["g"], k["d1"], k["d2"], k["w1"], k["w2"], k["B"]) == (0.84, 0.2, 0.8, 1.0, 0.0, 128)
    assert 8 * (16 + sum(NR.lengths(k))) == 203728   # (the state block's bytes)
    # llround: 225 x 0.5 x 48000 / 44100 = 122.449; 341 x 2 x 96000 / 44100 = 1484.63; 1116 x 0.5 = 558 exactly
    assert api.reverb_params(48000, 0.5, 0.5, 1.0, 0.5)["allpass_l"][3] == 122
    assert api.reverb_params(96000, 0.5, 0.5, 1.0, 2.0)["allpass_l"][2] == 1485
    assert api.reverb_params(44100, 0.5, 0.5, 1.0, 0.5)["combs_l"][0] == 558


# ---- the twin ----
def _noise(n, seed=3, amp=0.8):
    rng = np.random.default_rng(seed)
    return (amp * (2.0 * rng.random((n, 2)) - 1.0)).astype(np.float32)


@pytest.mark.parametrize("case", [RP.CASES[0], RP.CASES[2], RP.CASES[3]])
def test_twin_split_anywhere_is_the_one_piece_result(case):
    x = _noise(9000)
    x[100, 0] = np.inf
    x[3356, 1] = np.nan
    k = NR.params(SR, *case)
    whole, end = NR.reverb(x, k)
    for cut in (1, 63, 64, 65, 200, 333, 3357, 4097):
        a, sa = NR.reverb(x[:cut], k)
        b, sb = NR.reverb(x[cut:], k, state=sa)
        got = np.concatenate([a, b])
        assert np.array_equal(np.isfinite(got), np.isfinite(whole)), cut
        ok = np.isfinite(whole)
        assert np.array_equal(got[ok].view(np.uint32), whole[ok].view(np.uint32)), cut
        assert all(np.array_equal(p, q) for p, q in zip(sb["lines"], end["lines"])) and np.array_equal(sb["f"], end["f"]) and sb["total"] == 9000
    # a non-finite sample makes its own frame non-finite (the dry leg of the lerp) and no other: it enters the lines as 0
    assert np.argwhere(~np.isfinite(whole)).tolist() == [[100, 0], [3356, 1]]
    assert all(np.isfinite(ln).all() for ln in end["lines"]) and np.isfinite(end["f"]).all()


def test_impulse_response_shows_the_comb_delays_and_an_undamped_decay_of_g_per_pass():
    """An impulse of 1 on the left at frame 5, damp 0 (f = w): comb c of either channel answers 0.015 at 5 + D_c, 0.015 g at
    5 + 2 D_c, 0.015 g^2 at 5 + 3 D_c ..., and the bank's sum S is those trains added -- nothing else is non-zero."""
    k = NR.params(44100, 0.5, 0.0, 1.0, 1.0)
    g = k["g"]
    n = 7000
    x = np.zeros((n, 2), np.float32)
    x[5, 0] = 1.0
    tap = {}
    p, _ = NR.process(x, k, tap=tap)
    S = tap["S"]
    for ch, lens in ((0, k["combs_l"]), (1, k["combs_r"])):
        want = np.zeros(n)
        for D in lens:
            for j in range(1, (n - 6) // D + 1):
                want[5 + j * D] += 0.015 * g ** (j - 1)
        first = np.flatnonzero(S[:, ch])[:8]
        assert first.tolist() == [5 + D for D in lens], (ch, first)   # (8 distinct delays, in the tunings' order)
        assert np.array_equal(S[:, ch] != 0.0, want != 0.0)
        assert np.abs(S[:, ch] - want).max() <= 4e-16
        D = lens[0]
        passes = S[5 + D::D, ch][:5]
        assert np.allclose(passes[1:] / passes[:-1], g, rtol=1e-14, atol=0.0)
    # with damping the second pass is lower than g times the first and spread over later frames (the one-pole's tail)
    kd = NR.params(44100, 0.5, 1.0, 1.0, 1.0)
    NR.process(x, kd, tap=tap)
    D = kd["combs_l"][0]
    Sd = tap["S"][:, 0]
    assert Sd[5 + D] == 0.015 and abs(Sd[5 + 2 * D] - 0.015 * kd["g"] * kd["d2"]) <= 1e-17 and abs(Sd[5 + 2 * D + 1] - 0.015 * kd["g"] * kd["d2"] * kd["d1"]) <= 1e-17
    # the all-pass chain and the output: the first frame that sounds is the first comb's delay (every all-pass passes -s at once)
    assert np.flatnonzero(p[:, 0])[0] == 5 + k["combs_l"][0] and p[5 + k["combs_l"][0], 0] == np.float32(0.015)


def test_the_twins_gain_stays_under_the_guards_bound():
    """||p|| / ||x|| (both channels) on noise, on tones, on DC and on a tone a comb resonates at, over the grid and the corners of
    the ranges: at most Hrev."""
    n = 30000
    t = np.arange(n, dtype=np.float64)
    inputs = {"noise": _noise(n, 5)}
    for hz in (50.0, 997.0, 9000.0, 23000.0):
        s = (0.7 * np.sin(2.0 * np.pi * hz * t / SR)).astype(np.float32)
        inputs["%g Hz" % hz] = np.stack([s, s], axis=1)
    inputs["dc"] = np.full((n, 2), 0.5, np.float32)   # (every comb and the one-pole have their largest gain at 0 Hz)
    cases = RP.grid_cases() + [(1.0, 0.0, 1.0, 0.5), (1.0, 0.0, 0.0, 2.0), (1.0, 1.0, 1.0, 1.0), (0.0, 1.0, 0.0, 1.0)]
    worst = (0.0, None, None)
    for c in cases:
        k = NR.params(SR, *c)
        D = k["combs_l"][0]
        s = (0.7 * np.cos(2.0 * np.pi * t / D)).astype(np.float32)   # a period of the first comb's line
        for name, x in list(inputs.items()) + [("comb 0's period", np.stack([s, s], axis=1))]:
            p, _ = NR.process(x, k, raw=True)
            r = float(np.linalg.norm(p) / np.linalg.norm(x.astype(np.float64))) / k["Hrev"]
            if r > worst[0]:
                worst = (r, c, name)
    print("reverb L2 gain: worst ||p|| / ||x|| = %.4f of Hrev (%s on %s)" % worst)
    assert 0.0 < worst[0] <= 1.0


def test_the_constants_of_the_bound():
    """Stage by stage on the unit circle: the damping one-pole |d2 / (1 - d1 z)| <= 1, a comb |z^D / (1 - g F z^D)| <= 1 / (1 - g),
    an all-pass |(-1 + 1.5 z) / (1 - 0.5 z)| <= 5/3 (reached at z = -1), the output mix's matrix [[w1, w2], [w2, w1]] of norm w1 + w2
    = 1, the input mix (xl, xr) -> (in, in) of norm 0.015 x 2."""
    z = np.exp(1j * np.linspace(0.0, 2.0 * np.pi, 200001))
    ap = np.abs((-1.0 + 1.5 * z) / (1.0 - 0.5 * z))
    assert abs(ap.max() - 5.0 / 3.0) <= 1e-12 and abs(ap[100000] - 5.0 / 3.0) <= 1e-12   # (z = -1)
    for damp in (0.0, 0.3, 1.0):
        d1 = 0.4 * damp
        F = (1.0 - d1) / (1.0 - d1 * z)
        assert np.abs(F).max() <= 1.0 + 1e-12
        for g in (0.7, 0.98):
            for zz in (z, z ** 7):   # (z^D takes every phase whatever F's is: sweep them independently)
                assert (np.abs(1.0 / (1.0 - g * F * zz)) <= 1.0 / (1.0 - g) + 1e-9).all()
    for width in (0.0, 0.4, 1.0):
        w1, w2 = (1.0 + width) / 2.0, (1.0 - width) / 2.0
        assert abs(np.linalg.norm(np.array([[w1, w2], [w2, w1]]), 2) - 1.0) <= 1e-12
    assert abs(np.linalg.norm(0.015 * np.ones((2, 2)), 2) - 0.03) <= 1e-15
    assert NR.hrev(0.98) == 0.03 * (8.0 / (1.0 - 0.98)) * ((5.0 / 3.0) ** 2) ** 2 and 92.0 < NR.hrev(0.98) < 93.0


# ---- the bound of tests/test_gpu_reverb.py ----
def test_the_emulated_scan_stays_inside_the_committed_constant():
    """E = 8 x the worst max|scan - serial| / max|serial| of the numpy emulation over the GPU test's own grid and inputs, with
    every candidate window length; this recomputes that worst figure and fails above E / 8.  Also: damp 0 is bit-identical (the
    scan adds only zeros), and every grid case moves its input by far more than the bound (so the GPU test cannot pass on a
    vertex that does nothing)."""
    worst, weakest, runs = (0.0, None), (9e9, None), 0
    for sr in RP.RATES:
        for kind in RP.INPUTS:
            x = oracle_input(kind, sr)
            assert np.abs(x).max() > 0.05
            for c in RP.grid_cases():
                k = NR.params(sr, *c)
                ser, _ = NR.process(x, k, raw=True)
                peak = np.abs(ser).max()
                for B in NR.BLOCKS:
                    if B > min(NR.lengths(k)):
                        continue
                    sc, _ = NR.process(x, k, form=1, B=B, raw=True)
                    runs += 1
                    r = float(np.abs(sc - ser).max() / peak)
                    if k["d1"] == 0.0:
                        assert np.array_equal(sc, ser), (c, sr, kind, B)
                    if r > worst[0]:
                        worst = (r, (c, sr, kind, B))
                acts = float(np.abs(ser - x.astype(np.float64)).max() / (peak * (2.0 ** -23 + RP.E)))
                if acts < weakest[0]:
                    weakest = (acts, (c, sr, kind))
    print("emulated scan, %d runs: worst %.3g = 2^%.1f of the peak at %s; the weakest case moves its input by %.3g bounds (%s)"
          % (runs, worst[0], math.log2(worst[0]), worst[1], weakest[0], weakest[1]))
    assert runs >= 60
    assert 0.0 < worst[0] <= RP.E_EMULATED and RP.E == 8.0 * RP.E_EMULATED and RP.E <= 2.0 ** -28
    assert weakest[0] > 64.0


def test_the_scan_in_chunks_is_inside_the_same_constant():
    """The windows start at a chunk's first frame: chunks of 63, 333 and 4 097 frames (shorter than a window, no multiple of one,
    longer than the longest line) against the one-piece serial twin."""
    x = _noise(12000, 9, 0.5)
    k = NR.params(44100, 1.0, 1.0, 0.5, 2.0)
    ser, _ = NR.process(x, k, raw=True)
    for B in NR.BLOCKS:
        for step in (63, 333, 4097):
            st, parts = None, []
            for a in range(0, len(x), step):
                p, st = NR.process(x[a:a + step], k, state=st, form=1, B=B, raw=True)
                parts.append(p)
            assert np.abs(np.concatenate(parts) - ser).max() <= RP.E_EMULATED * np.abs(ser).max(), (B, step)


# ---- ranges ----
GOOD = dict(room=0.5, damp=0.5, width=1.0, size=1.0)
NAN, INF = float("nan"), float("inf")
BAD = [("room", dict(room=-0.01)), ("room", dict(room=1.01)), ("room", dict(room=NAN)), ("room", dict(room=INF)),
       ("damp", dict(damp=-0.01)), ("damp", dict(damp=1.5)), ("damp", dict(damp=NAN)),
       ("width", dict(width=-0.5)), ("width", dict(width=1.001)), ("width", dict(width=NAN)),
       ("size", dict(size=0.49)), ("size", dict(size=2.01)), ("size", dict(size=NAN)), ("size", dict(size=INF)), ("size", dict(size=-1.0))]


def _args(**kw):
    d = dict(GOOD, **kw)
    return d["room"], d["damp"], d["width"], d["size"]


@pytest.mark.parametrize("name,change", BAD)
def test_out_of_range_parameters_are_rejected_by_name(api, name, change):
    g = api.Graph(64, SR)
    with pytest.raises(api.TermdawError, match=name):
        g.add_reverb("w", 1.0, 0.0, 1.0, *_args(**change))
    with pytest.raises(api.TermdawError, match=name):
        api.reverb_params(SR, *_args(**change))
    g.add_sum("in", 1.0, 0.0)
    assert not g.set_output("w")   # (nothing was added)


def test_a_low_rate_is_rejected_through_size(api):
    """The shortest line, llround(225 size sr / 44100), must be at least 64 frames: at 22.05 kHz size 0.5 gives 56 and 0.57 gives 64."""
    g = api.Graph(64, 22050)
    with pytest.raises(api.TermdawError, match="size"):
        g.add_reverb("w", 1.0, 0.0, 1.0, 0.5, 0.5, 1.0, 0.5)
    with pytest.raises(api.TermdawError, match="size"):
        api.reverb_params(22050, 0.5, 0.5, 1.0, 0.5)
    g.add_reverb("w", 1.0, 0.0, 1.0, 0.5, 0.5, 1.0, 0.57)
    assert min(NR.lengths(api.reverb_params(22050, 0.5, 0.5, 1.0, 0.57))) == 64
    with pytest.raises(api.TermdawError, match="size"):
        api.reverb_params(8000, 0.5, 0.5, 1.0, 1.0)


def test_range_ends_are_accepted_and_wet_is_clamped(api):
    g = api.Graph(64, SR)
    g.add_sum("in", 1.0, 0.0)
    for i, a in enumerate(((0.0, 0.0, 0.0, 0.5), (1.0, 1.0, 1.0, 2.0))):
        g.add_reverb("w%d" % i, 1.0, 0.0, 1.0, *a)
    g.add_reverb("wet", 1.0, 0.0, 7.0, *_args())   # (wet is clamped, not rejected: graph.rs:256)
    g.add_reverb("dry", 1.0, 0.0, -3.0, *_args())
    assert g.connect("in", "w1") and g.set_output("w1") and g.check_graph()
    assert g.device_bytes() == 0   # (the state block is allocated when the vertex is first rendered)


def test_the_debug_options_take_their_values_only(api):
    g = api.Graph(64, SR)
    assert g.get_option("debug.reverb_form") in (0, 1) and g.get_option("debug.reverb_block") in NR.BLOCKS
    for key, good, bad in (("debug.reverb_form", (0, 1), (2, -1)), ("debug.reverb_block", NR.BLOCKS, (0, 32, 100, 512))):
        for v in good:
            g.set_option(key, v)
            assert g.get_option(key) == v
        for v in bad:
            with pytest.raises(api.TermdawError, match=key):
                g.set_option(key, v)


def _lua(line):
    return fx_rig._lua(line, "w")


LUA_BAD = [(k, c) for k, c in BAD if all(math.isfinite(v) for v in c.values())]


@pytest.mark.parametrize("name,change", LUA_BAD)
def test_lua_rejects_the_same_ranges(api, name, change):
    s = api.State("", SR, 64)
    assert not s.refresh(_lua('add_reverb("w", 1.0, 0.0, 1.0, %r, %r, %r, %r);' % _args(**change)))
    assert name in api.last_error() and "line 2" in api.last_error(), api.last_error()


def test_lua_accepts_and_dumps_the_canonical_line(api):
    s = api.State("", SR, 64)
    assert s.refresh(_lua('add_reverb("w", 0.5, -30, 1, 1, 0.5, 1, 0.5);')), api.last_error()
    dump = s.dump_calls()
    band = api.State("", SR, 64)
    assert band.refresh('add_sum("in", 1.0, 0.0);\nadd_bandpass("b", 0.5, -30, 1, 100.5, 4, true);\nconnect("in", "b");\nset_output("b");\n'), api.last_error()
    # the numbers print as add_bandpass prints the same values
    half, m30, one = band.dump_calls().split('add_bandpass("b",')[1].split(")")[0].split(",")[:3]
    line = [ln for ln in dump.splitlines() if ln.startswith("add_reverb(")]
    assert len(line) == 1
    args = line[0][len("add_reverb("):-1].split(",")
    assert args == ['"w"', half, m30, one, one, half, one, half] and " " not in line[0], line
    # ... and the dumped line is a project line again: it round-trips
    again = api.State("", SR, 64)
    assert again.refresh(_lua(line[0] + ";")), api.last_error()
    assert [ln for ln in again.dump_calls().splitlines() if ln.startswith("add_reverb(")] == line


def test_project_script_records_and_writes_the_call(tmp_path):
    p = W.ProjectScript(SR, 64)
    p.add_sum("in", 1.0, 0.0)
    p.add_reverb("w", 1.0, 0.0, 0.5, 0.84, 0.2, 1.0, 1.5)
    p.connect("in", "w")
    p.set_output("w")
    assert p.calls["add_reverb"] == [("w", 1.0, 0.0, 0.5, 0.84, 0.2, 1.0, 1.5)]
    assert 'add_reverb("w", 1.0, 0.0, 0.5, 0.84, 0.2, 1.0, 1.5);' in p.to_lua(str(tmp_path))


# ---- the host engine under sanitizers ----


@pytest.fixture(scope="module")
def asan_exe(tmp_path_factory):
    return fx_rig.asan_exe(tmp_path_factory, "asan_reverb", ["mock_guard.cpp", "mock_reverb.cpp", "asan_fx.cpp"])


def test_reverb_projects_under_sanitizers(asan_exe, tmp_path):
    n = int(os.environ.get("TD_ASAN_REVERB_SEEDS", "32"))
    workers = max(1, min(8, os.cpu_count() or 1))
    seeds = list(range(n))
    base = str(tmp_path / "p")
    with multiprocessing.Pool(workers) as pool:
        lists = pool.map(RP.write_projects, [(base, seeds[i::workers]) for i in range(workers) if seeds[i::workers]])
    procs = [subprocess.Popen([asan_exe] + lst, env=dict(os.environ, **ENV), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for lst in lists]
    tot = dict(reverb=0, vertices=0, serial=0, fresh=0, carried=0, summed=0, rejected=0, restarts=0, short=0)
    for p in procs:
        out, err = p.communicate(timeout=1800)
        assert p.returncode == 0, (out[-800:], err[-4000:])
        tail = out.split("asan_reverb done:")[1]
        tot["reverb"] += int(tail.split("k_reverb launches ")[1].split()[0])
        tot["vertices"] += int(tail.split("(")[1].split()[0])
        tot["serial"] += int(tail.split(" serial-form")[0].split()[-1])
        tot["fresh"] += int(tail.split(" entered fresh")[0].split()[-1])
        tot["carried"] += int(tail.split(" entered with the state")[0].split()[-1])
        tot["summed"] += int(tail.split(" k_reverb_sum launches")[0].split()[-1])
        tot["restarts"] += int(tail.split(" restarts checked")[0].split()[-1])
        tot["short"] += int(tail.split(" short chunks")[0].split()[-1])
        tot["rejected"] += int(tail.split(" rejected refreshes")[0].split()[-1])
    # multi-chunk renders and block pulls enter with the state (the mock checks the books of all 24 lines of every one of them);
    # every k_reverb follows its k_reverb_sum; both forms were compiled
    assert tot["rejected"] == 0 and tot["reverb"] >= n // 2 and tot["vertices"] >= tot["reverb"], tot
    assert tot["fresh"] > 0 and tot["carried"] > 0 and 0 < tot["serial"] < tot["vertices"] and tot["summed"] == tot["reverb"], tot
    # the pull right behind a set_time entered with nothing of its state, for every vertex the mock saw there (it aborts otherwise)
    assert tot["restarts"] > 0 and tot["short"] > 0, tot
    print("asan_reverb: %d projects clean: %s" % (n, tot))


REV = (0.84, 0.2, 1.0, 1.0)


def _guard_project(shape, wet=0.75, bl=1024):
    return fx_rig.guard_project(shape, lambda p, name, dry: p.add_reverb(name, 1.0, 0.0, 0.00009 if dry else wet, *REV), name="e", sr=SR, bl=bl)


def test_guard_modes_carry_the_estimate_through_a_reverb(api, asan_exe, tmp_path):
    """band_mode 2 / sine_mode 2 (the driver's profiled render): upstream of a reverb the scan / fast forms stay, and the guard's
    estimate at the output is the one of the same project without the vertex times (1 - wet) + wet Hrev."""
    shapes = ("band_up", "band_plain", "band_dry", "sine_up", "sine_free")
    fams, gains, _ = driver_report(asan_exe, tmp_path, {s: _guard_project(s) for s in shapes})
    exact = ("k_band_pass", "k_band_spec")
    for s in ("band_up", "band_plain", "band_dry"):
        assert "k_band_scan" in fams[s] and not any(k in fams[s] for k in exact), (s, fams[s])
    # 0.5 s in one chunk: two launches
    assert [k for k in fams["band_up"] if k.startswith("k_reverb")] == ["k_reverb_sum", "k_reverb"] and fams["band_up"]["k_reverb"] == 1, fams["band_up"]
    # wet < 0.0001 compiles to k_sum: the launch list of the project with a Sum in the reverb's place
    assert not any(k.startswith("k_reverb") for k in fams["band_dry"]) and list(fams["band_dry"].items()) == list(fams["band_plain"].items()), (fams["band_dry"], fams["band_plain"])
    for s in ("sine_up", "sine_free"):
        assert "k_sine_probe" in fams[s], (s, fams[s])
    assert fams["sine_up"].get("k_reverb") == 1 and not any(k.startswith("k_reverb") for k in fams["sine_free"])
    # the path gain: the driver prints the audit's gain from the band-pass vertex to the output (AuditHead)
    h = api.reverb_params(SR, *REV)["Hrev"]
    want = (1.0 - 0.75) + 0.75 * h
    assert h == NR.hrev(0.7 + 0.28 * float(np.float32(0.84)))
    assert gains["band_plain"]["path"] > 0.0
    assert abs(gains["band_up"]["path"] / gains["band_plain"]["path"] - want) < 1e-6 * want, (gains, want)
    assert abs(gains["band_dry"]["path"] / gains["band_plain"]["path"] - 1.0) < 1e-6, gains


def test_a_guarded_pull_that_runs_again_enters_with_the_state_it_first_entered_with(asan_exe, tmp_path):
    """Three guarded block pulls, each told to run again (mock_reverb.cpp): the first starts afresh both times and reads nothing of
    the state block; the second and the third continue from it, so the guard copies the block in front of the pull and puts it
    -- and the frame count on the host -- back in front of the second run: both runs find the same stamp, the one the run before
    them left last."""
    _, _, redo = driver_report(asan_exe, tmp_path, {"band_up": _guard_project("band_up"), "band_plain": _guard_project("band_plain")})
    assert int(redo["band_up"]["redos"]) == 3 and int(redo["band_plain"]["redos"]) == 3, redo
    e = [int(v) for v in redo["band_up"]["entries"].split(",")]
    assert len(e) == 4 and e[0] == e[1] and e[2] == e[3] and e[2] == e[0] + 2, e
    assert redo["band_plain"].get("entries", "") == ""


def test_projects_without_a_reverb_keep_their_launch_list(asan_exe, tmp_path):
    """The launch lists of drum_project, config 2 and config 4 (families and launch counts of one profiled render under the
    front-end's guard modes) as the parent commit compiled them."""
    projects = {"drums": W.drum_project(seconds=0.5), "config2": W.config2(seconds=0.5, n_src=8), "config4": W.config4(seconds=0.5, depth=6)}
    fams, _, _ = driver_report(asan_exe, tmp_path, projects)
    for name in projects:
        got = " ".join("%s=%d" % kv for kv in fams[name].items())
        assert not any(k.startswith("k_reverb") for k in fams[name]) and got == PARENT_LAUNCHES[name], (name, got)
