"""The rig the effect kinds' tests share.  A plain module, neither a test module nor a conftest: the test modules and the
*_projects.py files reach it through the sys.path.insert(0, tests dir) idiom they already use.

  - the helpers of the GPU tests: build / render_f32 / _pull_all, the bounds assert_close and mix_bound, MIX, _quantise16, the
    project directory of the front end (_write_project);
  - splice_project / write_projects: the one generator behind every random_<kind>_project;
  - asan_exe: one sanitizer build of the host engine per process, every driver linked against the same objects; ENV, _families,
    PARENT_LAUNCHES, the guard's shapes and the bodies of the range / Lua tests of the host modules;
  - FxKind and the bodies of the GPU placement tests, each a function of (gpu_api, kind record, ...): a test_gpu_<kind>.py keeps
    a test of the same name whose body is the one call.

A new kind brings a record, its *_projects.py grid and parameter draw, its twin, its mock and the tests only it has."""
import collections
import os
import shutil
import subprocess
import sys
import wave
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from termdaw_amd import workloads as W

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from np_twin import pan_gain  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "termdaw_amd", "csrc")
TESTS = os.path.join(ROOT, "tests")

REL = 2.0 ** -23
F32_TINY = float(np.float32(2.0) ** -149)
MIX = [(0.3, 0.5, 30.0), (0.75, 1.7, -75.0), (0.5, -0.8, 0.0), (0.999, 1.0, 90.0), (0.0001, 1.0005, 0.0009)]


# ---- renders of a built project ----
def build(api, p):
    """The built project after one discarded render of `bus`: the sample_multi vertices keep voices that are still sounding when
    a render ends (the reference's carried state), so only from the second render on does every render see the same input."""
    built = p.build(api)
    render_f32(api, built, "bus", p.cs)
    return built


def render_f32(api, built, out, cs, **opts):
    sb, fb, g = built
    for k, v in opts.items():
        g.set_option(k, v)
    assert g.set_output(out)
    fb.set_time(0)
    g.set_time(0)
    g.reset_normalize_vertices()
    return g.render_all(sb, fb, cs, 16, want_pcm=False)[1]


def _pull_all(api, built, out, cs):
    sb, fb, g = built
    assert g.set_output(out)
    fb.set_time(0)
    g.set_time(0)
    g.reset_normalize_vertices()
    blocks = []
    for _ in range(cs):
        l, r = g.render(sb, fb)
        fb.set_time_to_next_block()   # (the caller moves the events on, as the reference's pull loop does)
        blocks.append(np.stack([l, r], axis=1))
    return np.concatenate(blocks)


def _quantise16(x):
    v = x.astype(np.float32) * np.float32(32767.0)
    return np.clip(np.trunc(v.astype(np.float64)), -32768, 32767).astype(np.int64)


def _write_project(p, d):
    """The project directory the front end opens: project.lua + assets, project.toml."""
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, "project.lua"), "w") as f:
        f.write(p.to_lua(os.path.join(d, "assets")))
    with open(os.path.join(d, "project.toml"), "w") as f:
        f.write('[settings]\nmain = "project.lua"\nbuffer_length = %d\nproject_samplerate = %d\n' % (p.bl, p.psr))


# ---- the bounds ----
def over_bound(y, want, E):
    """The worst |y - want| over 2^-23 |want| + E max|want|, and where."""
    y64, w64 = y.astype(np.float64), want.astype(np.float64)
    lim = REL * np.abs(w64) + E * np.abs(w64).max()
    r = np.abs(y64 - w64) / lim
    r = np.where(np.isnan(r), np.inf, r)
    i = np.unravel_index(int(r.argmax()), r.shape)
    return float(r[i]), i


def _f32_up(v):
    r = v.astype(np.float32)
    return np.where(r.astype(np.float64) < v, np.nextafter(r, np.float32(np.inf)), r).astype(np.float32)


def _f32_down(v):
    r = v.astype(np.float32)
    return np.where(r.astype(np.float64) > v, np.nextafter(r, np.float32(-np.inf)), r).astype(np.float32)


def assert_close(y, x, p, what="", E=None):
    """wet = 1, no pan, no gain.  The bound is on p, the filtered signal rounded once to f32, where the definition puts that
    rounding: |p' - p| <= 2^-23 |p| + E max|p| for the device's p' against the twin's p.  What the vertex hands on is the
    definition's f32 lerp of it, out = x + 1 (p' - x), and that lerp is not the identity: where |x| is much larger than |p| --
    a 10 Hz low-pass on a drum bus -- p' - x rounds to an ulp of x, so one flipped rounding of p moves `out` by an ulp of x,
    many times 2^-23 |out|.  So the check goes through the lerp, which is monotone in p': with p_lo / p_hi the f32 ends of the
    allowed interval, lerp(p_lo) <= y <= lerp(p_hi).  Returns the largest |y - lerp(p)| in units of the plain form of the bound
    on `out` (a figure to print, not asserted: above 1 only where the lerp magnifies a flip).  E defaults to the EQ's."""
    if E is None:
        import eq_projects
        E = eq_projects.E
    assert y.shape == x.shape == p.shape
    one = np.float32(1.0)
    p64 = p.astype(np.float64)
    lim = REL * np.abs(p64) + E * np.abs(p64).max()
    lo = x + one * (_f32_up(p64 - lim) - x)
    hi = x + one * (_f32_down(p64 + lim) - x)
    want = x + one * (p - x)
    plain, at = over_bound(y, want, E)
    same = float(np.mean(y.view(np.uint32) == want.view(np.uint32)))
    bad = ~((lo <= y) & (y <= hi))
    print("%s: %.4f of the values bit-identical to the twin, worst |y - want| %.3g x the plain bound, %d outside" % (what, same, plain, int(bad.sum())))
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:4].tolist(), y[bad][:4], lo[bad][:4], hi[bad][:4])
    return plain


def assert_close_f32(y, want, what=""):
    """The compressor's bound, on the output as it stands: |y - want| <= 2^-23 |want| + the smallest subnormal, per value."""
    y64, w64 = y.astype(np.float64), want.astype(np.float64)
    err = np.abs(y64 - w64)
    lim = REL * np.abs(w64) + F32_TINY
    bad = ~(err <= lim)
    worst = float(np.max(np.where(w64 != 0, err / np.maximum(np.abs(w64), 1e-300), 0.0))) if len(y) else 0.0
    print("%s: worst relative error %.3g x 2^-23" % (what, worst / REL))
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:4].tolist(), y[bad][:4], want[bad][:4])


def mix_bound(x, proc, gain, angle):
    al, ar = pan_gain(np.ones(1, np.float32), np.ones(1, np.float32), gain, angle)
    amp = np.abs(np.array([float(al[0]), float(ar[0])]))
    return 4.0 * REL * np.maximum(np.abs(x), np.abs(proc)).astype(np.float64) * amp[None, :] + F32_TINY


# ---- random projects with effect vertices spliced in ----
def write_project(p, d):
    """The project directory the sanitizer drivers open: project.lua + assets, meta.txt (the block length)."""
    lua = p.to_lua(os.path.join(d, "assets"))
    with open(os.path.join(d, "project.lua"), "w") as f:
        f.write(lua)
    with open(os.path.join(d, "meta.txt"), "w") as f:
        f.write(str(p.bl))
    return d


def splice_project(seed, allow_sinf, *, rng_offset, prefix, add_call, draw, as_output=True, draw_keys=None):
    """A project of tests/test_gpu_fuzz.py with one to three `add_call` vertices spliced into edges of it, named prefix + "0"..,
    and (as_output) sometimes one more, prefix + "out", behind whatever the output was.  draw(rng, p) gives a vertex' arguments
    behind (name, gain, angle).  draw_keys(rng, order, name), for the kinds with a key input, gives the key edges of one spliced
    vertex, drawn right behind its arguments; `order` is the script as it was before anything was spliced.  One rng stream,
    default_rng(rng_offset + seed), drawn from in this order: the projects are pinned by tests/golden/fx_random_projects.json."""
    import test_gpu_fuzz as F
    p = F.random_project(seed, allow_sinf=allow_sinf)
    rng = np.random.default_rng(rng_offset + seed)
    gains, angles = [1.0, 1.0005, 0.5, 1.7, -0.8], [0.0, 0.0009, 30.0, -75.0, 120.0]
    edges = [i for i, (fn, a) in enumerate(p.script_order) if fn == "connect" and a[0] != a[1]]
    picks = sorted(set(int(i) for i in rng.choice(edges, size=min(len(edges), int(rng.integers(1, 4))), replace=False)), reverse=True)
    first_add = min(i for i, (fn, _) in enumerate(p.script_order) if fn.startswith("add_"))
    order = list(p.script_order)
    made, keys = [], []
    for k, i in enumerate(picks):   # (from the back: the indices in front stay valid)
        a, b = p.script_order[i][1]
        nm = "%s%d" % (prefix, k)
        ci = p.calls["connect"].index((a, b))
        p.calls["connect"][ci:ci + 1] = [(a, nm), (nm, b)]
        p.script_order[i:i + 1] = [("connect", (a, nm)), ("connect", (nm, b))]
        made.append((nm, float(rng.choice(gains)), float(rng.choice(angles))) + tuple(draw(rng, p)))
        if draw_keys is not None:
            keys += draw_keys(rng, order, nm)
    if as_output and rng.random() < 0.3:   # ... and one as the output, behind whatever the output was
        nm = prefix + "out"
        made.append((nm, 1.0, 0.0) + tuple(draw(rng, p)))
        p.calls["connect"].append((p.output_vertex, nm))
        oi = max(i for i, (fn, _) in enumerate(p.script_order) if fn == "set_output")
        p.script_order[oi:oi + 1] = [("connect", (p.output_vertex, nm)), ("set_output", (nm,))]
        p.output_vertex = nm
    for c in made:
        p.calls[add_call].append(c)
        p.script_order.insert(first_add, (add_call, c))
    oi = max(i for i, (fn, _) in enumerate(p.script_order) if fn == "set_output")
    for e in keys:   # (an edge that would close a loop only warns: the front end goes on without it)
        p.calls["connect_key"].append(e)
        p.script_order.insert(oi, ("connect_key", e))
    return p


def write_projects(random_project, args):
    """(base dir, seeds) -> the project dirs written."""
    base, seeds = args
    return [write_project(random_project(seed), os.path.join(base, "s%d" % seed)) for seed in seeds]


def oracle_input(kind, sr, base_project=None):
    """A grid's input as the GPU test sees it: the second render of `bus` (the first leaves the sample_multi voices sounding),
    here by the CPU oracle -- the engine's own render is the oracle's, bit for bit.  base_project defaults to the EQ's."""
    from oracle import binding as oracle
    if base_project is None:
        from eq_projects import base_project
    p = base_project(kind, sr=sr)
    sb, fb, g = p.build(oracle)
    g.render_all(sb, fb, p.cs, 16)
    fb.set_time(0)
    g.set_time(0)
    g.reset_normalize_vertices()
    return g.render_all(sb, fb, p.cs, 16)[1]


# ---- the host engine under sanitizers: stand-alone programs, one build of the engine per process ----
SOURCES = ["engine.cpp", "compile.cpp", "devmem.cpp", "comm.cpp", "project.cpp", "lua_subset.cpp", "wav.cpp", "midi.cpp"]
ASAN_FLAGS = ["-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-ffp-contract=off",
              "-D__HIP_PLATFORM_AMD__", "-I", "/opt/rocm/include", "-I", CSRC, "-I", os.path.join(ROOT, "include")]
# (mock_guard.cpp listens to the guard's launches of mock_hip.cpp: ld --wrap)
WRAPS = ["-Wl,--wrap=_ZN3tdk17launch_band_auditEPKNS_9AuditHeadEiP12ihipStream_t",
         "-Wl,--wrap=_ZN3tdk17launch_band_chainEPKNS_12BandScanDescEijjbP12ihipStream_t"]
ENV = dict(ASAN_OPTIONS="detect_leaks=0:allocator_may_return_null=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1", TD_ALLOC_CACHE_MB="0")
MAX_COMPILES = 16
_objects = {}   # source path -> object file, all compiled with ASAN_FLAGS (every driver's _build had this one flag list)
_obj_dir = None


def _compile(sources):
    """The objects of `sources`, compiling (at most MAX_COMPILES at a time) those that no call before has."""
    todo = [(s, os.path.join(_obj_dir, os.path.basename(s) + ".o")) for s in dict.fromkeys(sources) if s not in _objects]
    with ThreadPoolExecutor(MAX_COMPILES) as pool:
        codes = list(pool.map(lambda j: subprocess.call(["g++"] + ASAN_FLAGS + ["-c", j[0], "-o", j[1]]), todo))
    assert not any(codes), [s for (s, _), c in zip(todo, codes) if c]
    _objects.update(todo)
    return [_objects[s] for s in sources]


def asan_exe(tmp_path_factory, name, extra_sources):
    """The program `name`: the host engine, tests/mock_hip.cpp and the files of tests/ in extra_sources (the kind's mock and its
    driver, which has the main), under ASan / UBSan.  The first call compiles the engine and the mocks the effect kinds link,
    every call what of its own files no call before it has; then it links.  mock_guard.cpp among the extras links it in, with
    the wraps it needs."""
    global _obj_dir
    if shutil.which("g++") is None or not os.path.exists("/opt/rocm/include/hip/hip_runtime_api.h"):
        pytest.skip("needs g++ and the HIP headers")
    if _obj_dir is None:
        _obj_dir = str(tmp_path_factory.mktemp("asan_objects"))
    linked = [os.path.join(CSRC, f) for f in SOURCES] + [os.path.join(TESTS, f) for f in ["mock_hip.cpp"] + list(extra_sources)]
    objs = _compile(linked + [os.path.join(TESTS, "mock_guard.cpp")])[:len(linked)]
    exe = os.path.join(str(tmp_path_factory.mktemp(name)), name)
    wraps = WRAPS if "mock_guard.cpp" in extra_sources else []
    subprocess.check_call(["g++", "-fsanitize=address,undefined", "-o", exe] + wraps + objs + ["-lpthread", "-ldl"])
    return exe


def driver_report(asan_exe, tmp_path, projects):
    """One run of a driver over the projects (name -> ProjectScript), by what it prints per project: the launch families of its
    profiled render {family: launches}, the guard's path gains {word: value}, the guard's redo words {word: text}."""
    dirs = {name: write_project(p, str(tmp_path / name)) for name, p in projects.items()}
    r = subprocess.run([asan_exe] + list(dirs.values()), env=dict(os.environ, **ENV), capture_output=True, text=True, timeout=1800)
    assert r.returncode == 0, (r.stdout[-800:], r.stderr[-4000:])
    back = {d: name for name, d in dirs.items()}
    fams, gains, redo = {}, {}, {}
    for ln in r.stdout.splitlines():
        for tag, store, value in (("launches ", fams, int), ("guard ", gains, float), ("redo ", redo, str)):
            if ln.startswith(tag):
                d, rest = ln[len(tag):].split(":", 1)
                store[back[d]] = dict((kv.split("=")[0], value(kv.split("=")[1])) for kv in rest.split())   # (dicts keep the driver's order)
    return fams, gains, redo


def _families(asan_exe, tmp_path, projects):
    return driver_report(asan_exe, tmp_path, projects)[0]


# (recorded on the EQ's parent commit with its own driver of the same form, tests/asan_comp.cpp, on these project directories)
PARENT_LAUNCHES = {
    "drums": "k_sample_multi=1 k_sum=1 k_band_scan=2 k_band_audit=1 k_sources=1",
    "config2": "k_sum=1",
    "config4": "k_band_scan=1 k_sources=1",
}


def parent_projects():
    return {"drums": W.drum_project(seconds=0.5), "config2": W.config2(seconds=0.5, n_src=8), "config4": W.config4(seconds=0.5, depth=6)}


def check_parent_launches(asan_exe, tmp_path, prefix):
    """The launch lists of drum_project, config 2 and config 4 (families and launch counts of one profiled render under the
    front-end's guard modes) as the parent commit compiled them, and none of the kind's kernels among them."""
    projects = parent_projects()
    fams = _families(asan_exe, tmp_path, projects)
    for name in projects:
        got = " ".join("%s=%d" % kv for kv in fams[name].items())
        assert not any(k.startswith(prefix) for k in fams[name]) and got == PARENT_LAUNCHES[name], (name, got)


# ---- the guard's shapes of the host modules ----
def guard_project(shape, add_vertex, name="c", sr=48000, bl=1024, seconds=0.5):
    """The guard's shapes: `b` / `y` is what the guard would speed up (a band-pass under band_mode 2, a synth under sine_mode 2).
    add_vertex(p, name, dry) adds the kind's vertex; a Sum stands in its place in band_plain and sine_free, the controls."""
    p = W.ProjectScript(sr, bl)
    p.set_length(seconds)
    p.assets["a"] = W.Asset(W.noise_int16(7, 9000))
    p.load_sample("a", "a", "")
    p.event_files["f"] = np.array([(0.01, 60.0, 0.8), (0.2, 60.0, 0.0), (0.25, 62.0, 0.6)], np.float32)
    p.load_midi_floww("f", "f")
    if shape == "band_up":       # loop -> band-pass -> vertex
        p.add_sampleloop("s", 1.0, 0.0, "a")
        p.add_bandpass("b", 1.0, 0.0, 1.0, 300.0, 5000.0, True)
        add_vertex(p, name, False)
        p.connect("s", "b"); p.connect("b", name); p.set_output(name)
    elif shape == "band_down":   # loop -> vertex -> band-pass
        p.add_sampleloop("s", 1.0, 0.0, "a")
        add_vertex(p, name, False)
        p.add_bandpass("b", 1.0, 0.0, 1.0, 300.0, 5000.0, True)
        p.connect("s", name); p.connect(name, "b"); p.set_output("b")
    elif shape == "band_both":   # loop -> band-pass -> vertex -> band-pass
        p.add_sampleloop("s", 1.0, 0.0, "a")
        p.add_bandpass("b", 1.0, 0.0, 1.0, 300.0, 5000.0, True)
        add_vertex(p, name, False)
        p.add_bandpass("b2", 1.0, 0.0, 1.0, 300.0, 5000.0, True)
        p.connect("s", "b"); p.connect("b", name); p.connect(name, "b2"); p.set_output("b2")
    elif shape in ("band_dry", "band_plain"):   # loop -> band-pass -> a dry vertex (a k_sum launch, gain 1) / a Sum in its place
        p.add_sampleloop("s", 1.0, 0.0, "a")
        p.add_bandpass("b", 1.0, 0.0, 1.0, 300.0, 5000.0, True)
        if shape == "band_dry":
            add_vertex(p, name, True)
        else:
            p.add_sum(name, 1.0, 0.0)
        p.connect("s", "b"); p.connect("b", name); p.set_output(name)
    elif shape in ("sine_up", "one_tile"):      # synth -> vertex (one_tile: a render of 2 048 frames, by `seconds`)
        p.add_synth("y", 1.0, 0.0, "f", 0.4, 0.3, W.HIT_ADSR, 1.0, 0.8, W.NOTE_ADSR, 0.5, W.STD_ADSR)
        add_vertex(p, name, False)
        p.connect("y", name); p.set_output(name)
    else:                        # synth -> sum: the control
        assert shape == "sine_free", shape
        p.add_synth("y", 1.0, 0.0, "f", 0.4, 0.3, W.HIT_ADSR, 1.0, 0.8, W.NOTE_ADSR, 0.5, W.STD_ADSR)
        p.add_sum(name, 1.0, 0.0)
        p.connect("y", name); p.set_output(name)
    return p


# ---- the range and Lua tests of the host modules, driven by a file's GOOD / RANGES / ORDER / BAD ----
def _args(good, order, as_float=False, **kw):
    """The kind's arguments behind `wet`, in `order`: `good` with kw laid over it."""
    a = dict(good, **kw)
    return [float(a[k]) if as_float else a[k] for k in order]


def _lua(line, vertex="g", key=None):
    """A script of a Sum `in` into the vertex that `line` adds, the output; key: its key edge's source, `in` or a second Sum."""
    head = 'add_sum("in", 1.0, 0.0);\n' + ('add_sum("%s", 1.0, 0.0);\n' % key if key not in (None, "in") else "")
    edge = 'connect_key("%s", "%s");\n' % (key, vertex) if key else ""
    return '%s%s\nconnect("in", "%s");\n%sset_output("%s");\n' % (head, line, vertex, edge, vertex)


def out_of_range_is_rejected_by_name(api, sr, add, params, args, name):
    """add(graph, *args) and params(sr, *args), the kind's td_graph_add_* and td_*_params (None: it has none), name the parameter."""
    g = api.Graph(64, sr)
    with pytest.raises(api.TermdawError, match=name):
        add(g, *args)
    if params is not None:
        with pytest.raises(api.TermdawError, match=name):
            params(sr, *args)


def range_ends_are_accepted(api, sr, add, vertex, ranges, order, good_args):
    """Both ends of every range at once, wet clamped and not rejected; returns the graph."""
    g = api.Graph(64, sr)
    g.add_sum("in", 1.0, 0.0)
    for i, end in enumerate((0, 1)):
        add(g, "%s%d" % (vertex, i), 1.0, 0.0, 1.0, *[ranges[k][end] for k in order])
        assert g.connect("in", "%s%d" % (vertex, i))
    add(g, "wet", 1.0, 0.0, 7.0, *good_args)   # (wet is clamped, not rejected: graph.rs:256)
    add(g, "dry", 1.0, 0.0, -3.0, *good_args)
    assert g.set_output(vertex + "1") and g.check_graph()
    return g


def lua_rejects_the_same_ranges(api, sr, call, args, name, lua=_lua):
    s = api.State("", sr, 64)
    line = '%s("g", 1.0, 0.0, 1.0, %s);' % (call, ", ".join(repr(float(v)) for v in args))
    assert not s.refresh(lua(line))
    assert name in api.last_error(), api.last_error()


# ---- the placement tests of the GPU modules ----
# What a kind's test module says of the kind, for the bodies below:
#   word, prefix, launches   the kind in a sentence ("gate"), its kernels' common prefix ("k_gate") and the launches of a whole render
#   add                      add(p, name, src, case, wet=1.0, gain=1.0, angle=0.0): the *_projects.py function
#   base_project             base_project(input, sr=, bl=, seconds=, seed=): sources -> Sum `bus`
#   case, case2              the file's CASE and the second vertex of the series test
#   E                        the constant of the bound (assert_close)
#   twin                     twin(api, sr, case, x) -> (p, xd): the wet path in f32 and the input it is mixed with (x itself for a
#                            kind without latency, the delayed input otherwise)
#   mix                      mix(api, sr, case, x, wet=, gain=, angle=) -> what the vertex hands on, by the twin
#   acts                     acts(proc, xd) -> bool, for a kind whose proof that the vertex does something is not the plain
#                            |want - x| > 1e-3 wet (the limiter's, on the delayed input); also asserted on the series' second vertex
FxKind = collections.namedtuple("FxKind", "word prefix launches add base_project case case2 E twin mix acts", defaults=(None,))


def _close(kind, y, xd, p, what):
    return assert_close(y, xd, p, what, kind.E)


def _launches(kind, names):
    return [n for n in names if n.startswith(kind.prefix)]


def wet_pan_and_gain(gpu_api, kind, wet, gain, angle, vertex="v", **project_kw):
    p = kind.base_project("drums", **project_kw)
    kind.add(p, vertex, "bus", kind.case, wet=wet, gain=gain, angle=angle)
    built = build(gpu_api, p)
    x = render_f32(gpu_api, built, "bus", p.cs)
    y = render_f32(gpu_api, built, vertex, p.cs)
    want = kind.mix(gpu_api, 48000, kind.case, x, wet=wet, gain=gain, angle=angle)
    proc, xd = kind.twin(gpu_api, 48000, kind.case, x)
    lim = mix_bound(xd, proc, gain, angle)
    err = np.abs(y.astype(np.float64) - want.astype(np.float64))
    print("wet %g gain %g angle %g: worst error / bound %.3g" % (wet, gain, angle, float(np.max(err / lim))))
    assert (err <= lim).all(), (float(np.max(err / lim)), np.argwhere(err > lim)[:4].tolist())
    if kind.acts is not None:
        assert kind.acts(proc, xd)               # (the vertex does something)
    else:
        assert np.abs(want - x).max() > 1e-3 * wet   # (the vertex does something, in proportion to the mix)


def dry_passes_the_input_through(gpu_api, kind, live=None, **project_kw):
    """wet 0 and wet just under 0.0001 hand the input on, undelayed, as a plain sum launch; a vertex that is not dry launches the
    kind's kernels.  live: (name, case) of a vertex that is not dry and hands its input on all the same (the gate's range_db 0)."""
    p = kind.base_project("drums", **project_kw)
    kind.add(p, "dry", "bus", kind.case, wet=0.0)
    kind.add(p, "almost", "bus", kind.case, wet=0.00009)
    kind.add(p, *(("wet", "bus", kind.case) if live is None else (live[0], "bus", live[1])))
    built = build(gpu_api, p)
    x = render_f32(gpu_api, built, "bus", p.cs)
    for name in ("dry", "almost") + (() if live is None else (live[0],)):
        y = render_f32(gpu_api, built, name, p.cs)
        assert np.array_equal(y, x), (name, np.argwhere(y != x)[:4].tolist())
    g = built[2]
    g.set_profiling(1)
    render_f32(gpu_api, built, "dry", p.cs)
    names = list(g.kernel_times())
    assert not any(n.startswith(kind.prefix) for n in names) and "k_sum" in names, names   # wet < 0.0001: a plain sum launch
    render_f32(gpu_api, built, "wet" if live is None else live[0], p.cs)
    assert _launches(kind, g.kernel_times()) == kind.launches


def in_front_of_a_normalize_output(gpu_api, kind, vertex="v"):
    p = kind.base_project("drums", seconds=1.0)
    kind.add(p, vertex, "bus", kind.case)
    p.add_normalize("out", 1.0, 0.0)
    p.connect(vertex, "out")
    built = build(gpu_api, p)
    x = render_f32(gpu_api, built, "bus", p.cs)
    c = render_f32(gpu_api, built, vertex, p.cs)
    pw, xd = kind.twin(gpu_api, 48000, kind.case, x)
    _close(kind, c, xd, pw, "in front of Normalize")
    # normalize_gen (extensions.rs:321-329) on what the vertex really handed on: the running block peak from 1e-6, f32
    pk = np.abs(c).reshape(-1, p.bl * 2).max(axis=1)
    run = np.maximum.accumulate(np.concatenate([[np.float32(0.000001)], pk]).astype(np.float32))[1:]
    want = c * np.repeat(np.float32(1.0) / run, p.bl)[:, None]
    sb, fb, g = built
    g.set_output("out")
    fb.set_time(0)
    g.set_time(0)
    g.reset_normalize_vertices()
    pcm, f = g.render_all(sb, fb, p.cs, 16)
    assert (np.abs(f.astype(np.float64) - want) <= 2.0 * REL * np.abs(want) + F32_TINY).all()
    assert np.abs(pcm.astype(np.int64) - _quantise16(want)).max() <= 1


def as_a_stem_and_two_in_series(gpu_api, kind, first="v1", second="v2"):
    p = kind.base_project("drums", seconds=1.0)
    kind.add(p, first, "bus", kind.case)
    kind.add(p, second, first, kind.case2, gain=0.8, angle=-20.0)
    p.add_sum("post", 0.5, 10.0)
    p.connect(second, "post")
    built = build(gpu_api, p)
    x = render_f32(gpu_api, built, "bus", p.cs)
    y1 = render_f32(gpu_api, built, first, p.cs)
    pw, xd = kind.twin(gpu_api, 48000, kind.case, x)
    _close(kind, y1, xd, pw, "first of two")
    # the second one against the twin on what the first one really handed it
    y2 = render_f32(gpu_api, built, second, p.cs)
    w2 = kind.mix(gpu_api, 48000, kind.case2, y1, gain=0.8, angle=-20.0)
    proc, xd2 = kind.twin(gpu_api, 48000, kind.case2, y1)
    if kind.acts is not None:
        assert kind.acts(proc, xd2)
    assert (np.abs(y2.astype(np.float64) - w2) <= mix_bound(xd2, proc, 0.8, -20.0)).all()
    # both as stems of a render whose output sits downstream
    sb, fb, g = built
    g.set_output("post")
    g.set_stems([second, first])
    fb.set_time(0)
    g.set_time(0)
    g.render_all(sb, fb, p.cs, 16)
    assert np.abs(g.read_stem_pcm(0).astype(np.int64) - _quantise16(y2)).max() == 0
    assert np.abs(g.read_stem_pcm(1).astype(np.int64) - _quantise16(y1)).max() == 0
    g.set_stems([])


def fed_by_an_inlined_loop_source_and_a_gain_stage(gpu_api, kind, case, asset, vertex="v", check=None):
    """check(x): the kind's own proof that `case` works on this input."""
    p = W.ProjectScript(48000, 1024)
    p.set_length(0.5)
    p.assets["a0"] = W.Asset(asset)
    p.assets["a1"] = W.Asset(W.noise_int16(51, 9001))
    p.load_sample("a0", "a0", "")
    p.load_sample("a1", "a1", "normalize-seperate")
    p.add_sampleloop("l0", 0.7, 30.0, "a0")     # read by the vertex itself (term kinds 1 / 3)
    p.add_sampleloop("l1", 0.02, 0.0, "a1")
    p.add_sum("stage", 0.5, -45.0)              # one input: a gain / pan stage, read through (term kind 4)
    p.connect("l1", "stage")
    kind.add(p, vertex, "l0", case)
    p.connect("stage", vertex)
    p.set_output(vertex)
    built = p.build(gpu_api)
    a = render_f32(gpu_api, built, "l0", p.cs)
    b = render_f32(gpu_api, built, "stage", p.cs)
    x = (np.float32(0.0) + a) + b               # sum_inputs (extensions.rs:310-319), f32, in connect() order
    pw, xd = kind.twin(gpu_api, 48000, case, x)
    if check is not None:
        check(x)
    for packed in (1, 0):
        y = render_f32(gpu_api, built, vertex, p.cs, packed_samples=packed)
        _close(kind, y, xd, pw, "inlined terms, packed_samples %d" % packed)


def batch_matches_own_renders(gpu_api, projects, distinct=True):
    """Every member of a batch of the projects has the words of its own render, twice over."""
    cs = projects[0].cs
    own = []   # per project: its first and its second render (the second starts with the voices the first left sounding)
    for p in projects:
        sb, fb, g = p.build(gpu_api)
        first = g.render_all(sb, fb, cs, 16, want_f32=False)[0]
        g.reset_normalize_vertices()
        fb.set_time(0)
        g.set_time(0)
        own.append((first, g.render_all(sb, fb, cs, 16, want_f32=False)[0]))
    if distinct:
        assert len({o[0].tobytes() for o in own}) == len(projects)
    batch = gpu_api.Batch()
    for p in projects:
        batch.add(*p.build(gpu_api))
    for rep in range(2):
        batch.rewind()
        assert batch.render_all(cs, 16) == cs * 1024
        for i in range(len(projects)):
            assert np.array_equal(batch.read_pcm(i, cs), own[i][rep]), (rep, i)


def batch_members_are_bitwise_their_own_renders(gpu_api, kind, inputs, cases, vertex="v"):
    projects = []
    for i in range(8):
        p = kind.base_project(inputs[i % 3], seconds=1.0, seed=i)
        c = cases[(13 * i + 5) % len(cases)]
        kind.add(p, vertex, "bus", c, wet=[1.0, 0.6][i % 2], gain=[1.0, 0.7][(i // 4) % 2])
        if i % 4 == 1:     # a second one in series, as the output
            kind.add(p, vertex + "2", vertex, cases[(29 * i + 1) % len(cases)])
            p.set_output(vertex + "2")
        elif i % 4 == 2:   # in front of a Normalize output
            p.add_normalize("out", 1.0, 0.0)
            p.connect(vertex, "out")
            p.set_output("out")
        else:
            p.set_output(vertex)
        projects.append(p)
    batch_matches_own_renders(gpu_api, projects)


def projects_without_the_kind_launch_no_kernel_of_it(gpu_api, prefix):
    for p in (W.drum_project(seconds=1.0), W.config2(seconds=1.0, n_src=8)):
        sb, fb, g = p.build(gpu_api)
        g.set_profiling(1)
        g.render_all(sb, fb, p.cs, 16, want_f32=False)
        names = list(g.kernel_times())
        assert names and not any(n.startswith(prefix) for n in names), names


def a_whole_render_launches_the_kinds_kernels(gpu_api, kind, vertex="v"):
    """... and returns the built project, profiling on."""
    p = kind.base_project("drums")
    kind.add(p, vertex, "bus", kind.case)
    p.set_output(vertex)
    sb, fb, g = p.build(gpu_api)
    g.set_profiling(1)
    g.render_all(sb, fb, p.cs, 16, want_f32=False)
    assert _launches(kind, g.kernel_times()) == kind.launches
    return sb, fb, g


# ---- the guard modes ----
def gpu_guard_base(bl=1024, seconds=1.0, notes=((0.01, 60.0, 0.8), (0.4, 60.0, 0.0), (0.5, 64.0, 0.6), (0.9, 64.0, 0.0))):
    """A loop `s`, two band-pass vertices `b1` `b2`, a synth `y` playing `notes` and a Sum `bus`, unconnected: what the guard
    would speed up."""
    p = W.ProjectScript(48000, bl)
    p.set_length(seconds)
    p.assets["a"] = W.Asset(W.noise_int16(7, 9000))
    p.load_sample("a", "a", "")
    p.event_files["f"] = np.array(notes, np.float32)
    p.load_midi_floww("f", "f")
    p.add_sampleloop("s", 0.5, 0.0, "a")
    p.add_bandpass("b1", 1.0, 0.0, 1.0, 300.0, 5000.0, True)
    p.add_bandpass("b2", 1.0, 10.0, 1.0, 200.0, 8000.0, True)
    p.add_synth("y", 0.5, 0.0, "f", 0.4, 0.3, W.HIT_ADSR, 1.0, 0.8, W.NOTE_ADSR, 0.5, W.STD_ADSR)
    p.add_sum("bus", 1.0, 0.0)
    return p


SHORT_NOTES = ((0.01, 60.0, 0.8), (0.1, 60.0, 0.0), (0.12, 64.0, 0.6), (0.22, 64.0, 0.0))   # (for renders of a quarter of a second)


def gpu_guard_project(call, vertex, args, vertex_first, wet=1.0, **base_kw):
    p = gpu_guard_base(**base_kw)
    getattr(p, call)(vertex, 1.0, 0.0, wet, *args)
    if vertex_first:   # loop -> vertex -> band-pass chain; the synth joins behind the vertex
        p.connect("s", vertex); p.connect(vertex, "b1"); p.connect("b1", "b2"); p.connect("b2", "bus"); p.connect("y", "bus")
        p.set_output("bus")
    else:              # band-pass chain and synth -> bus -> vertex
        p.connect("s", "b1"); p.connect("b1", "b2"); p.connect("b2", "bus"); p.connect("y", "bus"); p.connect("bus", vertex)
        p.set_output(vertex)
    return p


def _guard_renders(gpu_api, p):
    outs, names = {}, {}
    for mode, (bm, sm) in (("guard", (2, 2)), ("exact", (0, 1))):
        sb, fb, g = p.build(gpu_api)
        g.set_option("band_mode", bm)
        g.set_option("sine_mode", sm)
        g.set_profiling(1)
        outs[mode] = g.render_all(sb, fb, p.cs, 16, want_pcm=False)[1]
        names[mode] = list(g.kernel_times())
    return outs, names


def guard_keeps_the_scan_and_fast_sines_downstream(gpu_api, p, word, prefix, launches):
    outs, names = _guard_renders(gpu_api, p)
    rms = float(np.sqrt(np.mean((outs["guard"].astype(np.float64) - outs["exact"].astype(np.float64)) ** 2)))
    print("guarded scan + fast sines downstream of a %s: rms %.3g against the exact forms" % (word, rms))
    assert rms <= 1e-6 and np.abs(outs["exact"]).max() > 0.05
    assert "k_band_scan" in names["guard"] and "k_sine_probe" in names["guard"], names["guard"]
    assert not any(n in names["guard"] for n in ("k_band_pass", "k_band_spec")), names["guard"]
    assert [n for n in names["guard"] if n.startswith(prefix)] == launches


def guard_renders_the_exact_forms_upstream(gpu_api, p, floor=0.05):
    outs, names = _guard_renders(gpu_api, p)
    assert np.array_equal(outs["guard"].view(np.uint32), outs["exact"].view(np.uint32)) and np.abs(outs["exact"]).max() > floor
    assert "k_band_scan" not in names["guard"] and "k_sine_probe" not in names["guard"], names["guard"]
    assert any(n in names["guard"] for n in ("k_band_pass", "k_band_spec")), names["guard"]


# ---- the front end ----
def into_the_drum_bus(call, args, key=None, seconds=1.0):
    """drum_project with the vertex `args` (its add_ call's, name first) between the drum bus `drums` and the band-pass in front of
    the output; key: the source of a key edge into it."""
    name = args[0]
    p = W.drum_project(seconds=seconds)
    i = p.calls["connect"].index(("drums", "band"))
    p.calls["connect"][i:i + 1] = [("drums", name), (name, "band")]
    j = p.script_order.index(("connect", ("drums", "band")))
    p.script_order[j:j + 1] = [(call, args), ("connect", ("drums", name)), ("connect", (name, "band"))] + ([("connect_key", (key, name))] if key else [])
    p.calls[call].append(args)
    if key:
        p.calls["connect_key"].append((key, name))
    return p


def front_end_renders(gpu_api, tmp_path, p, *dumped):
    """The command line's wave file of the project has the words of State.render_to_memory, which are returned; the State's dump
    holds every string of `dumped`."""
    d = str(tmp_path / "proj")
    _write_project(p, d)
    out = str(tmp_path / "m.wav")
    r = subprocess.run([sys.executable, "-m", "termdaw_amd", d, "-o", out], env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    st = gpu_api.State(open_dir=d)
    assert st.refresh(), gpu_api.last_error()
    dump = st.dump_calls()
    assert all(s in dump for s in dumped), (dumped, dump)
    mem = st.render_to_memory()
    with wave.open(out, "rb") as w:
        words = np.frombuffer(w.readframes(w.getnframes()), np.int16).reshape(-1, 2)
    assert words.shape == mem.shape and np.array_equal(words, mem) and np.abs(mem).max() > 1000
    return mem


def front_end_words_differ(gpu_api, tmp_path, q, mem):
    """... and the vertex is really in the path: the project `q` without it (or with it dry) gives other words."""
    d2 = str(tmp_path / "plain")
    _write_project(q, d2)
    st2 = gpu_api.State(open_dir=d2)
    assert st2.refresh()
    assert not np.array_equal(st2.render_to_memory(), mem)
