"""Random projects that contain compressor vertices (TEST INFRASTRUCTURE, a generator of its own: the generators the existing
tests and soaks draw from keep producing the graphs they always did).  A project of tests/test_gpu_fuzz.py's generator gets
one to three compressor vertices spliced into edges it already has -- in front of Normalize vertices, behind gain stages and
inlined loop sources, in series where two land on one path -- and, now and then, one more as the output."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fx_rig  # noqa: E402


def random_comp_params(rng):
    return (float(rng.choice([1.0, 1.0, 0.5, 0.0])),                       # wet
            float(rng.choice([-80.0, -30.0, -18.0, -6.0, 0.0])),            # threshold_db
            float(rng.choice([1.0, 2.0, 4.0, 1000.0])),                     # ratio
            float(rng.choice([0.0, 1.0, 40.0, 1000.0])),                    # attack_ms
            float(rng.choice([1.0, 100.0, 2000.0, 10000.0])),               # release_ms
            float(rng.choice([0.0, 6.0, 40.0])),                            # knee_db
            float(rng.choice([-40.0, 0.0, 3.0, 40.0])))                     # makeup_db


def random_comp_project(seed, allow_sinf=True):
    return fx_rig.splice_project(seed, allow_sinf, rng_offset=900_000, prefix="c", add_call="add_compressor",
                                 draw=lambda rng, p: random_comp_params(rng))


def write_projects(args):
    """(base dir, seeds) -> the project dirs written: project.lua + assets, meta.txt (the block length)."""
    return fx_rig.write_projects(random_comp_project, args)
