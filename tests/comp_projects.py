"""Random projects that contain compressor vertices (TEST INFRASTRUCTURE, a generator of its own: the generators the existing
tests and soaks draw from keep producing the graphs they always did).  A project of tests/test_gpu_fuzz.py's generator gets
one to three compressor vertices spliced into edges it already has -- in front of Normalize vertices, behind gain stages and
inlined loop sources, in series where two land on one path -- and, now and then, one more as the output."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_fuzz as F  # noqa: E402


def random_comp_params(rng):
    return (float(rng.choice([1.0, 1.0, 0.5, 0.0])),                       # wet
            float(rng.choice([-80.0, -30.0, -18.0, -6.0, 0.0])),            # threshold_db
            float(rng.choice([1.0, 2.0, 4.0, 1000.0])),                     # ratio
            float(rng.choice([0.0, 1.0, 40.0, 1000.0])),                    # attack_ms
            float(rng.choice([1.0, 100.0, 2000.0, 10000.0])),               # release_ms
            float(rng.choice([0.0, 6.0, 40.0])),                            # knee_db
            float(rng.choice([-40.0, 0.0, 3.0, 40.0])))                     # makeup_db


def random_comp_project(seed, allow_sinf=True):
    p = F.random_project(seed, allow_sinf=allow_sinf)
    rng = np.random.default_rng(900_000 + seed)
    gains, angles = [1.0, 1.0005, 0.5, 1.7, -0.8], [0.0, 0.0009, 30.0, -75.0, 120.0]
    edges = [i for i, (fn, a) in enumerate(p.script_order) if fn == "connect" and a[0] != a[1]]
    picks = sorted(set(int(i) for i in rng.choice(edges, size=min(len(edges), int(rng.integers(1, 4))), replace=False)), reverse=True)
    first_add = min(i for i, (fn, _) in enumerate(p.script_order) if fn.startswith("add_"))
    comps = []
    for k, i in enumerate(picks):   # (from the back: the indices in front stay valid)
        a, b = p.script_order[i][1]
        nm = "c%d" % k
        ci = p.calls["connect"].index((a, b))
        p.calls["connect"][ci:ci + 1] = [(a, nm), (nm, b)]
        p.script_order[i:i + 1] = [("connect", (a, nm)), ("connect", (nm, b))]
        comps.append((nm, float(rng.choice(gains)), float(rng.choice(angles))) + random_comp_params(rng))
    if rng.random() < 0.3:   # ... and one as the output, behind whatever the output was
        nm = "cout"
        comps.append((nm, 1.0, 0.0) + random_comp_params(rng))
        p.calls["connect"].append((p.output_vertex, nm))
        oi = max(i for i, (fn, _) in enumerate(p.script_order) if fn == "set_output")
        p.script_order[oi:oi + 1] = [("connect", (p.output_vertex, nm)), ("set_output", (nm,))]
        p.output_vertex = nm
    for c in comps:
        p.calls["add_compressor"].append(c)
        p.script_order.insert(first_add, ("add_compressor", c))
    return p


def write_projects(args):
    """(base dir, seeds) -> the project dirs written: project.lua + assets, meta.txt (the block length)."""
    base, seeds = args
    out = []
    for seed in seeds:
        p = random_comp_project(seed)
        d = os.path.join(base, "s%d" % seed)
        lua = p.to_lua(os.path.join(d, "assets"))
        with open(os.path.join(d, "project.lua"), "w") as f:
            f.write(lua)
        with open(os.path.join(d, "meta.txt"), "w") as f:
            f.write(str(p.bl))
        out.append(d)
    return out
