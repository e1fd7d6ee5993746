"""Key edges on the host, no GPU (include/termdaw_amd.h td_graph_connect_key): what td_graph_connect_key rejects,
by message, through the C ABI; the Lua line and the project script; facts of the keyed twin (tests/np_key.py) that can be derived
by hand, and that the ducking project of tests/test_gpu_key.py is not vacuous; the host engine on random projects with key edges
under AddressSanitizer / UBSan as a stand-alone program (tests/asan_comp.cpp as it is, against tests/mock_hip.cpp +
tests/mock_key.cpp, whose mock launches check the key term tables, the class words and which entry point a descriptor came
through); and the guard rule, read from the launch families the mock build reports."""
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
import gate_projects as GP  # noqa: E402
import key_projects as KP  # noqa: E402
import np_compressor as NC  # noqa: E402
import np_gate as NG  # noqa: E402
import np_key as NK  # noqa: E402
from fx_rig import ENV, PARENT_LAUNCHES, _families  # noqa: E402
GATE = (-30.0, 6.0, 10.0, 1.0, 100.0, -20.0)
COMP = (-30.0, 4.0, 1.0, 20.0, 6.0, 0.0)


# ---- td_graph_connect_key ----
def _graph(api):
    g = api.Graph(64, 48000)
    g.add_sum("a", 1.0, 0.0)
    g.add_sum("b", 1.0, 0.0)
    g.add_gate("g", 1.0, 0.0, 1.0, *GATE)
    g.add_compressor("c", 1.0, 0.0, 1.0, *COMP)
    return g


def test_unknown_names_are_rejected_with_connects_messages(api):
    g = _graph(api)
    assert not g.connect_key("nope", "g")
    assert 'vertex "nope" cannot be found and thus can\'t be connected.' in api.last_error()
    assert not g.connect_key("a", "nope")
    assert 'vertex "nope" cannot be found and thus can\'t be connected to.' in api.last_error()
    assert g.connect_key("a", "g") and g.connect_key("a", "c") and g.connect_key("a", "g")   # (a duplicate is an edge of its own)


def test_only_a_compressor_or_a_gate_takes_a_key(api):
    g = api.Graph(64, 48000)
    g.add_sum("src", 1.0, 0.0)
    g.add_sum("sum", 1.0, 0.0)
    g.add_normalize("norm", 1.0, 0.0)
    g.add_sampleloop("loop", 1.0, 0.0, 0)
    g.add_sample_multi("multi", 1.0, 0.0, 0, 0, -1)
    g.add_sample_lerp("lerp", 1.0, 0.0, 0, 0, -1, 10)
    g.add_debug_sine("sine", 1.0, 0.0, 0)
    g.add_synth("synth", 1.0, 0.0, 0, 0.4, 0.3, W.HIT_ADSR, 1.0, 0.8, W.NOTE_ADSR, 0.5, W.STD_ADSR)
    g.add_adsr("adsr", 1.0, 0.0, 1.0, 0, False, True, -1, W.NOTE_ADSR)
    g.add_bandpass("band", 1.0, 0.0, 1.0, 300.0, 5000.0, True)
    g.add_eq("eq", 1.0, 0.0, 1.0, "peak", 900.0, 2.5, 9.0)
    g.add_delay("delay", 1.0, 0.0, 0.5, 120.0, 0.3, 0.0)
    g.add_saturator("sat", 1.0, 0.0, 1.0, "soft", 6.0, 0.0, 0.0, 2)
    g.add_chorus("chorus", 1.0, 0.0, 0.5, 2, 10.0, 2.0, 0.5, 0.5, "sine")
    g.add_reverb("reverb", 1.0, 0.0, 0.3, 0.5, 0.5, 1.0, 1.0)
    others = ("sum", "norm", "loop", "multi", "lerp", "sine", "synth", "adsr", "band", "eq", "delay", "sat", "chorus", "reverb")
    for name in others:
        assert not g.connect_key("src", name), name
        assert api.last_error() == "connect_key: %s takes no key input" % name, api.last_error()
    g.add_gate("g", 1.0, 0.0, 1.0, *GATE)
    g.add_compressor("c", 1.0, 0.0, 1.0, *COMP)
    for name in others:   # ... and any vertex may BE the key
        assert g.connect_key(name, "g") and g.connect_key(name, "c"), (name, api.last_error())


def test_loops_are_found_over_input_and_key_edges_together(api):
    g = _graph(api)
    # a loop closed by a key edge: g -> a (input), a -> g (key)
    assert g.connect("g", "a")
    assert not g.connect_key("a", "g") and api.last_error() == "connect_key: edge would close a loop"
    assert not g.connect_key("g", "g") and "connect_key" in api.last_error()
    # a loop closed by an input edge through a key edge that is there: b -> c (key), then c -> b (input)
    assert g.connect_key("b", "c")
    assert not g.connect("c", "b") and api.last_error() == "connect: edge would close a loop"
    # ... and through both kinds: a -> c is fine, c -> g is fine, g -> a exists: a -> c -> g -> a needs one more edge
    assert g.connect("a", "c") and not g.connect_key("c", "g") and api.last_error() == "connect_key: edge would close a loop"


def test_reset_clears_key_edges(api):
    g = _graph(api)
    assert g.connect("g", "a") and not g.connect_key("a", "g")
    assert g.connect_key("b", "g")
    api.lib().td_graph_reset(g.h)
    g.add_sum("a", 1.0, 0.0)
    g.add_sum("b", 1.0, 0.0)
    g.add_gate("g", 1.0, 0.0, 1.0, *GATE)
    # the edges of before are gone: what was a loop then is none now, in either kind
    assert g.connect_key("a", "g"), api.last_error()
    assert g.connect("g", "b"), api.last_error()


def test_a_key_is_not_an_input_for_check_graph(api):
    g = _graph(api)
    assert g.connect_key("a", "g") and g.set_output("g")
    assert not g.check_graph() and "output receives no inputs" in api.last_error()
    assert g.connect("b", "g") and g.check_graph()


# ---- the Lua line, the project script ----
LUA = ('add_sum("in", 1.0, 0.0);\nadd_sum("k", 1.0, 0.0);\nadd_gate("g", 1.0, 0.0, 1.0, -30, 6, 10, 1, 100, -20);\n'
       'add_compressor("c", 1.0, 0.0, 1.0, -30, 4, 1, 20, 6, 0);\n%s\nconnect("in", "g");\nconnect("g", "c");\nset_output("c");\n')


def test_lua_accepts_connect_key_and_dumps_the_canonical_line(api):
    s = api.State("", 48000, 64)
    assert s.refresh(LUA % 'connect_key( "k" , "g" );\nconnect_key("k","c");'), api.last_error()
    lines = [ln for ln in s.dump_calls().splitlines() if ln.startswith("connect_key(")]
    assert lines == ['connect_key("k","g")', 'connect_key("k","c")'], lines


def test_lua_warns_on_a_bad_connect_key_and_renders_on(api):
    """Like a bad connect: the refresh succeeds, the graph is the one without that edge."""
    s = api.State("", 48000, 64)
    # (written in front of the connect calls and applied behind them: the loop is found)
    assert s.refresh(LUA % 'connect_key("c", "g");\nconnect_key("k", "in");\nconnect_key("nope", "g");'), api.last_error()
    assert 'connect_key("k","in")' in s.dump_calls()
    t = api.State("", 48000, 64)
    assert t.refresh(LUA % "")


def test_project_script_records_and_writes_the_call(tmp_path):
    p = W.ProjectScript(48000, 64)
    p.add_sum("in", 1.0, 0.0)
    p.add_sum("k", 1.0, 0.0)
    p.add_gate("g", 1.0, 0.0, 1.0, *GATE)
    p.connect("in", "g")
    p.connect_key("k", "g")
    p.set_output("g")
    assert p.calls["connect_key"] == [("k", "g")] and ("connect_key", ("k", "g")) in p.script_order
    assert 'connect_key("k", "g");' in p.to_lua(str(tmp_path))


def test_project_script_applies_key_edges_to_the_graph(api):
    p = W.ProjectScript(48000, 64)
    p.add_sum("in", 1.0, 0.0)
    p.add_gate("g", 1.0, 0.0, 1.0, *GATE)
    p.connect_key("g", "g")   # (rejected by the graph: build goes on, as the front-end does)
    p.connect("in", "g")
    p.set_output("g")
    sb, fb, g = p.build(api)
    assert not g.connect_key("g", "g") and g.connect_key("in", "g")


# ---- facts of the twin ----
def _xk(n=6000):
    g = GP.gated_frames()
    rng = np.random.default_rng(11)
    x = (0.5 * rng.uniform(-1.0, 1.0, (n, 2))).astype(np.float32)
    return x, np.tile(g, (n // len(g) + 1, 1))[:n]


def test_key_equal_to_the_input_is_the_unkeyed_twin_bitwise(api):
    x, k = _xk()
    c = api.gate_params(48000, *GATE)
    for kw in (dict(), dict(wet=0.7, gain=1.7, angle=30.0), dict(wet=0.0, gain=0.5)):
        a, ea = NK.gate(k, k, c, **kw)
        b, eb = NG.process(k, c, **kw)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) and ea == eb
        a, ea = NK.compressor(k, k, 48000, *COMP, **kw)
        b, eb = NC.compress(k, 48000, *COMP, **kw)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) and ea == eb


def test_twin_splits_give_the_one_piece_result_bitwise(api):
    x, k = _xk()
    c = api.gate_params(48000, *GATE)
    kw = dict(wet=0.7, gain=1.7, angle=30.0)
    gw, ge = NK.gate(x, k, c, **kw)
    cw, ce = NK.compressor(x, k, 48000, *COMP, **kw)
    for cut in (1, 777, 2048, 4999):
        a, st = NK.gate(x[:cut], k[:cut], c, **kw)
        b, st = NK.gate(x[cut:], k[cut:], c, state=st, **kw)
        assert np.array_equal(np.concatenate([a, b]).view(np.uint32), gw.view(np.uint32)) and st == ge, cut
        a, st = NK.compressor(x[:cut], k[:cut], 48000, *COMP, **kw)
        b, st = NK.compressor(x[cut:], k[cut:], 48000, *COMP, state=st, **kw)
        assert np.array_equal(np.concatenate([a, b]).view(np.uint32), cw.view(np.uint32)) and st == ce, cut


def test_a_non_finite_key_frame_leaves_the_state_where_a_finite_input_frame_does_not(api):
    """The rule is applied to the KEY frame: a NaN / infinite key sample stays out of the compressor's state and forces nothing in
    the gate, while the (finite) input frame beside it is processed; a non-finite INPUT frame under a finite key changes no state
    at all and comes out as what IEEE makes of it, at that frame only."""
    c = api.gate_params(48000, *GATE)
    loud = np.full((64, 2), np.float32(0.25))
    quiet = np.full((64, 2), np.float32(1e-4))
    for bad in (float("nan"), float("inf"), float("-inf")):
        k = quiet.copy()
        k[20, 0] = bad
        out, end = NK.gate(loud, k, c)
        assert end == NG.closed(c[2]) and np.isfinite(out).all()                     # an infinite key sample did not open it
        assert NK.gate(loud, loud, c)[1][1] == 1                                      # (the same frames as the key do)
        yl, st = NK.compressor_yl(k, 48000, *COMP[:5])
        assert st == (0.0, 0.0) and not yl.any()
        assert NK.compressor(loud, k, 48000, *COMP)[0].tobytes() == loud.tobytes()    # G = 1: nothing entered the state
        # the other way round: the state is the finite key's, the bad input frame alone comes out non-finite
        x = loud.copy()
        x[20, 1] = bad
        out, end = NK.gate(x, loud, c)
        assert end == NK.gate(loud, loud, c)[1] and (~np.isfinite(out)).sum() == 1 and not np.isfinite(out[20, 1])
        out, end = NK.compressor(x, loud, 48000, *COMP)
        assert end == NK.compressor(loud, loud, 48000, *COMP)[1] and (~np.isfinite(out)).sum() == 1


def test_the_ducking_project_is_not_vacuous(api):
    """From the twin alone: x the noise bus' level, k `gated` as its loop plays it (gate_projects.gated_frames)."""
    k = GP.gated_frames()
    rng = np.random.default_rng(5)
    x = (0.5 * rng.uniform(-1.0, 1.0, (len(k), 2))).astype(np.float32)
    for case in KP.gate_grid():
        c = api.gate_params(48000, *case)
        t, env, _ = NK.gate_env(k, c)
        ups = int(np.sum(np.diff(np.concatenate([[0], t]).astype(np.int8)) == 1))
        downs = int(np.sum(np.diff(t.astype(np.int8)) == -1))
        assert ups >= 3 and downs >= 3, (case, ups, downs)
        keyed, unkeyed = NK.gate(x, k, c)[0], NG.process(x, c)[0]
        assert np.abs(keyed.astype(np.float64) - unkeyed).max() > 1e-3, case
    # the compressor: the loud segments sit 18 dB over the threshold -- 0.75 x 18 = 13.5 dB wanted; the first loud segment ends at
    # frame 3 000, and 6 000 quiet frames (6 time constants of 20 ms) lie between frames 6 700 and 12 700
    yl, _ = NK.compressor_yl(k, 48000, *KP.COMP_CASE[:5])
    assert yl[:3000].max() >= 10.0 and yl[3000:12700].min() <= 0.5, (yl[:3000].max(), yl[3000:12700].min())
    keyed, unkeyed = NK.compressor(x, k, 48000, *KP.COMP_CASE)[0], NC.compress(x, 48000, *KP.COMP_CASE)[0]
    assert np.abs(keyed.astype(np.float64) - unkeyed).max() > 1e-3


def test_random_key_projects_key_from_upstream_or_aside_only():
    for seed in range(24):
        p = KP.random_key_project(seed)
        assert 1 <= len(p.calls["connect_key"]) <= 3 and p.keyed
        dynamics = {c[0] for c in p.calls["add_gate"] + p.calls["add_compressor"]}
        for a, b in p.calls["connect_key"]:
            assert b in dynamics and a != b, (seed, a, b)
        keys = p.calls["connect_key"]
        for i, (a, b) in enumerate(keys):   # no key source lies downstream of the vertex it keys, over both kinds of edge
            rest = p.calls["connect"] + keys[:i] + keys[i + 1:]
            assert a not in KP.downstream(p, b, rest), (seed, a, b)


# ---- the host engine under sanitizers: a stand-alone program ----
@pytest.fixture(scope="module")
def asan_exe(tmp_path_factory):
    return fx_rig.asan_exe(tmp_path_factory, "asan_key", ["mock_key.cpp", "asan_comp.cpp"])


def test_key_projects_under_sanitizers(asan_exe, tmp_path):
    """Whole, chunked and pulled renders, a batch, every band / sine mode (the driver's loops) over random projects with key edges."""
    n = int(os.environ.get("TD_ASAN_KEY_SEEDS", "24"))
    workers = max(1, min(8, os.cpu_count() or 1))
    seeds = list(range(n))
    base = str(tmp_path / "p")
    with multiprocessing.Pool(workers) as pool:
        lists = pool.map(KP.write_projects, [(base, seeds[i::workers]) for i in range(workers) if seeds[i::workers]])
    procs = [subprocess.Popen([asan_exe] + lst, env=dict(os.environ, **ENV), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for lst in lists]
    steps = vertices = carried = fresh = keyed = 0
    for p in procs:
        out, err = p.communicate(timeout=1800)
        assert p.returncode == 0, (out[-800:], err[-4000:])
        tail = out.split("asan_comp done:")[1]
        assert " 0 failed calls" in tail and " 0 rejected refreshes" in tail, tail
        steps += int(tail.split("k_comp launches ")[1].split()[0])
        vertices += int(tail.split("(")[1].split()[0])
        fresh += int(tail.split(" entered fresh")[0].split()[-1])
        carried += int(tail.split(" entered with carried state")[0].split()[-1])
        keyed += int(out.split("mock_key: ")[1].split()[0])
    # every vertex went through each of its five steps; keyed descriptors were among them, fresh and carried
    assert steps == vertices and vertices >= n and fresh > 0 and carried > 0 and keyed >= n // 2, (steps, vertices, fresh, carried, keyed)
    print("asan_key: %d projects, %d vertices (%d fresh, %d carried), %d of them keyed: clean" % (n, vertices, fresh, carried, keyed))


def _guard_project(shape):
    """`up`: a band-pass and a synth upstream of a key edge; `dry`: the same with the keyed vertex dry; `plain`: no key edge."""
    kind, wet = shape.split("_")
    p = W.ProjectScript(48000, 1024)
    p.set_length(0.5)
    p.assets["a"] = W.Asset(W.noise_int16(7, 9000))
    p.load_sample("a", "a", "")
    p.event_files["f"] = np.array([(0.01, 60.0, 0.8), (0.2, 60.0, 0.0), (0.25, 62.0, 0.6)], np.float32)
    p.load_midi_floww("f", "f")
    p.add_sampleloop("s", 1.0, 0.0, "a")
    p.add_sampleloop("in", 0.5, 0.0, "a")
    p.add_bandpass("b", 1.0, 0.0, 1.0, 300.0, 5000.0, True)
    p.add_synth("y", 1.0, 0.0, "f", 0.4, 0.3, W.HIT_ADSR, 1.0, 0.8, W.NOTE_ADSR, 0.5, W.STD_ADSR)
    p.add_sum("kb", 1.0, 0.0)
    p.connect("s", "b"); p.connect("b", "kb"); p.connect("y", "kb")
    w = {"wet": 1.0, "dry": 0.0, "plain": 1.0}[wet]
    if kind == "gate":
        p.add_gate("v", 1.0, 0.0, w, *GATE)
    else:
        p.add_compressor("v", 1.0, 0.0, w, *COMP)
    p.connect("in", "v")
    # the output sums the keyed vertex and the key bus: the band-pass and the synth reach it by an input path too, so that the
    # guard has an estimate to carry where the key does not forbid it
    p.add_sum("out", 1.0, 0.0)
    p.connect("v", "out"); p.connect("kb", "out")
    if wet != "plain":
        p.connect_key("kb", "v")
    p.set_output("out")
    return p


def test_guard_modes_keep_the_exact_forms_upstream_of_a_key(asan_exe, tmp_path):
    """band_mode 2 / sine_mode 2 (the driver's profiled render): the launch families each shape went through."""
    shapes = [k + "_" + w for k in ("gate", "comp") for w in ("wet", "dry", "plain")]
    fams = _families(asan_exe, tmp_path, {name: _guard_project(name) for name in shapes})
    exact = ("k_band_pass", "k_band_spec")
    for kind in ("gate", "comp"):
        wet, dry, plain = fams[kind + "_wet"], fams[kind + "_dry"], fams[kind + "_plain"]
        # upstream of a key edge into a vertex that is not dry: the exact families, no probe
        assert "k_band_scan" not in wet and any(k in wet for k in exact) and "k_sine_probe" not in wet and "k_synth" in wet, wet
        # a dry keyed vertex ignores its key: the launch list of the same project without the edge
        assert "k_band_scan" in plain and "k_sine_probe" in plain and not any(k in plain for k in exact), plain
        assert list(dry.items()) != [] and "k_band_scan" in dry and "k_sine_probe" in dry and not any(k in dry for k in exact), dry
        assert not any(k.startswith(("k_gate", "k_comp")) for k in dry), dry


def test_projects_without_a_key_keep_their_launch_list(asan_exe, tmp_path):
    projects = {"drums": W.drum_project(seconds=0.5), "config2": W.config2(seconds=0.5, n_src=8), "config4": W.config4(seconds=0.5, depth=6)}
    dirs = {name: EP.write_project(p, str(tmp_path / name)) for name, p in projects.items()}
    r = subprocess.run([asan_exe] + list(dirs.values()), env=dict(os.environ, **ENV), capture_output=True, text=True, timeout=1800)
    assert r.returncode == 0, (r.stdout[-800:], r.stderr[-4000:])
    back = {d: name for name, d in dirs.items()}
    for ln in r.stdout.splitlines():
        if ln.startswith("launches "):
            d, rest = ln[len("launches "):].split(":", 1)
            assert rest.strip() == PARENT_LAUNCHES[back[d]], (back[d], rest)
    assert "mock_key: 0 keyed descriptors" in r.stdout
