"""The rig's one splice generator (tests/fx_rig.py splice_project) still makes the projects the per-kind generators made before
they were folded into it: tests/golden/fx_random_projects.json holds, per generator, one sha256 over seeds 0..31, recorded with
the separate bodies of the commit before."""
import hashlib
import importlib
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fx_random_projects.json")


def digest(random_project):
    h = hashlib.sha256()
    for seed in range(32):
        p = random_project(seed)
        h.update(repr((p.script_order, sorted(p.calls.items()), p.output_vertex)).encode())
    return h.hexdigest()


def test_random_projects_are_the_ones_of_the_separate_generators():
    with open(GOLDEN) as f:
        golden = json.load(f)
    assert len(golden) == 13
    got = {}
    for name in golden:
        module, fn = name.split(".")
        got[name] = digest(getattr(importlib.import_module(module), fn))
    assert got == golden, sorted(k for k in golden if got[k] != golden[k])
