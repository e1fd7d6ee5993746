"""Projects with key edges (td_graph_connect_key; TEST INFRASTRUCTURE, a generator of its own: the generators the existing tests
draw from keep producing the graphs they always did).

* ducking_project: eq_projects' `noise` bus as the signal, gate_projects' `gated` loop at GATED_GAIN as the key -- read directly (an
  inlined loop term as a key) or through a Sum `keybus` -- so that every transition of the two definitions happens at a place
  known from SEGMENTS while the gain acts on a signal that has nothing to do with it.
* random_key_project / write_projects: a comp_projects / gate_projects random project with one to three key edges into its
  dynamics vertices, their sources drawn from the vertices that are not downstream of the keyed vertex."""
import os
import sys

import numpy as np

from termdaw_amd import workloads as W

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import eq_projects as EP  # noqa: E402
import fx_rig  # noqa: E402
import gate_projects as GP  # noqa: E402

GATE_CASE = (-30.0, 6.0, 10.0, 1.0, 100.0, -20.0)   # test_gpu_gate.CASE: threshold, hysteresis, hold, attack, release, range
COMP_CASE = (-30.0, 4.0, 1.0, 20.0, 6.0, 0.0)        # threshold, ratio, attack, release, knee, makeup
VIAS = ("direct", "keybus")


def gate_grid():
    """The reduced grid: hysteresis {0, 6} x hold {0, 10} x (attack, release) {(0, 1), (1, 100), (40, 2000)}, range -20."""
    return [(-30.0, hy, ho, at, re, -20.0) for hy in (0.0, 6.0) for ho in (0.0, 10.0) for at, re in ((0.0, 1.0), (1.0, 100.0), (40.0, 2000.0))]


def comp_grid():
    """knee {0, 6} x release {20, 100, 2000} around COMP_CASE."""
    return [(-30.0, 4.0, 1.0, re, kn, 0.0) for kn in (0.0, 6.0) for re in (20.0, 100.0, 2000.0)]


def ducking_project(via="direct", sr=48000, bl=1024, seconds=0.5):
    """`bus`: the noise; the key source's name is returned beside the project ("key": the loop itself, "keybus": a Sum behind it)."""
    p = EP.base_project("noise", sr=sr, bl=bl, seconds=seconds)
    p.assets["g"] = W.Asset(GP.gated_int16(0), sr=sr)
    p.load_sample("g", "g", "")
    p.add_sampleloop("key", GP.GATED_GAIN, 0.0, "g")
    if via == "direct":
        return p, "key"
    p.add_sum("keybus", 1.0, 0.0)
    p.connect("key", "keybus")
    return p, "keybus"


def add_gate(p, name, src, key, case=GATE_CASE, wet=1.0, gain=1.0, angle=0.0):
    p.add_gate(name, gain, angle, wet, *case)
    if src:
        p.connect(src, name)
    for k in ([key] if isinstance(key, str) else key):
        p.connect_key(k, name)


def add_comp(p, name, src, key, case=COMP_CASE, wet=1.0, gain=1.0, angle=0.0):
    p.add_compressor(name, gain, angle, wet, *case)
    if src:
        p.connect(src, name)
    for k in ([key] if isinstance(key, str) else key):
        p.connect_key(k, name)


def vertex_names(p):
    return [a[0] for fn, a in p.script_order if fn.startswith("add_")]


def downstream(p, v, edges=None):
    """v and everything its frames reach, over input and key edges (every edge the script asks for, those the engine rejects
    included: an over-estimate)."""
    seen, todo = {v}, [v]
    edges = p.calls["connect"] + p.calls["connect_key"] if edges is None else edges
    while todo:
        u = todo.pop()
        for a, b in edges:
            if a == u and b not in seen:
                seen.add(b)
                todo.append(b)
    return seen


def random_key_project(seed, allow_sinf=True):
    """p.keyed: the keyed vertices, in the order their first key edge was added."""
    if seed % 2:
        import comp_projects as CP
        p = CP.random_comp_project(seed, allow_sinf=allow_sinf)
        kind = "add_compressor"
    else:
        p = GP.random_gate_project(seed, allow_sinf=allow_sinf)
        kind = "add_gate"
    rng = np.random.default_rng(1_230_000 + seed)
    targets = [c[0] for c in p.calls[kind]]
    names = sorted(set(vertex_names(p)))
    p.keyed = []
    for _ in range(int(rng.integers(1, 4))):
        b = str(rng.choice(targets))
        free = [n for n in names if n not in downstream(p, b)]
        if not free:
            continue
        p.connect_key(str(rng.choice(free)), b)
        if b not in p.keyed:
            p.keyed.append(b)
    if not p.keyed:   # (every vertex downstream of the one dynamics vertex: cannot happen while it has an input)
        raise RuntimeError("random_key_project(%d): no key source" % seed)
    return p


def write_projects(args):
    """(base dir, seeds) -> the project dirs written: project.lua + assets, meta.txt (the block length)."""
    return fx_rig.write_projects(random_key_project, args)
