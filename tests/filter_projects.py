"""Projects that contain filter vertices (TEST INFRASTRUCTURE, a generator of its own: the generators the existing tests and
soaks draw from keep producing the graphs they always did).

* base_project / grid_cases / E: the inputs, the parameter grid and the bound's constant that tests/test_gpu_filter.py (on the
  device) and tests/test_filter_host.py (the derivation of E, on the CPU) share.  The inputs are eq_projects': drums, noise and a
  burst between silences.
* random_filter_project / write_projects: a project of tests/test_gpu_fuzz.py's generator with one to three filter vertices
  spliced into edges it already has, now and then keyed by another vertex of the graph, and, now and then, one more as the output
  (the sanitizer run's input)."""
import itertools
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import eq_projects as EP  # noqa: E402
import fx_rig  # noqa: E402
import np_filter as NF  # noqa: E402

RATES = EP.RATES
INPUTS = EP.INPUTS
SHAPES = ("sine", "triangle")
KINDS = NF.KINDS
# The GPU test's bound, per value: |y - want| <= 2^-23 |want| + E max|want|.  E_EMULATED is the worst
# max|blocked - serial| / max|serial| that np_filter.blocked() -- the tiled scans in numpy, follower included, with the kernels'
# tile geometry and join order -- shows over grid_cases() on the three inputs at the three rates, rounded up
# (test_filter_host.py recomputes it and fails above this figure); the device's own order of the same float64 operations gets
# the project's factor 8 on top.  E must stay <= 2^-28, a sixteenth of half an f32 ulp at the render's peak.
E_EMULATED = 1.0e-11
E = min(8 * E_EMULATED, 2.0 ** -28)
assert E <= 2 ** -28

base_project = EP.base_project


def grid_cases(sr):
    """(kind, freq_hz, q, lfo_oct, rate_hz, stereo, shape, env_oct, sens_db, attack_ms, release_ms): the issue's grid at rate sr,
    108 cases -- kind x (freq, q) x (lfo_oct, rate) x the follower's set; shape and stereo alternate with the case's index, so
    that all four pairs occur."""
    out = []
    for i, (kind, (fr, q), (lo, rate), env) in enumerate(itertools.product(
            KINDS, ((20.0, 0.5), (1000.0, 5.0), (0.45 * sr, 30.0)), ((0.0, 1.0), (4.0, 0.01), (4.0, 20.0)),
            ((0.0, 12.0, 5.0, 50.0), (8.0, 30.0, 0.0, 1.0), (-8.0, 0.0, 1000.0, 10000.0)))):
        out.append((kind, fr, q, lo, rate, 0.25 * ((i // 2) % 2), SHAPES[i % 2]) + env)
    return out


def spec(api, sr, case):
    """What np_filter takes, on the engine's own constants."""
    return NF.spec(api.filter_params(sr, *case), case[0], case[5], case[6])


def add_filter(p, name, src, case, wet=1.0, gain=1.0, angle=0.0, key=None):
    p.add_filter(name, gain, angle, wet, *case)
    p.connect(src, name)
    if key is not None:
        p.connect_key(key, name)


def random_filter_params(rng):
    fr, q = [(20.0, 0.5), (1000.0, 5.0), (21600.0, 30.0), (300.0, 0.707)][int(rng.integers(0, 4))]   # (the driver opens every project at 48 kHz)
    env = [(0.0, 0.0, 0.0, 1.0), (8.0, 30.0, 0.0, 1.0), (-8.0, 0.0, 1000.0, 10000.0), (3.0, 12.0, 5.0, 120.0)][int(rng.integers(0, 4))]
    return (float(rng.choice([1.0, 1.0, 0.5, 0.0])),                     # wet
            str(rng.choice(KINDS)), fr, q,
            float(rng.choice([0.0, 2.0, 4.0])),                           # lfo_oct
            float(rng.choice([0.01, 1.0, 20.0])),                         # rate_hz
            float(rng.choice([0.0, 0.25, 0.5])),                          # stereo
            str(rng.choice(SHAPES))) + env


def _random_key(rng, order, nm):
    """Half of the time a key from somewhere else in the graph."""
    sources = sorted({a[0] for fn, a in order if fn == "connect"})
    return [(str(rng.choice(sources)), nm)] if rng.random() < 0.5 else []


def random_filter_project(seed, allow_sinf=True):
    return fx_rig.splice_project(seed, allow_sinf, rng_offset=1_030_000, prefix="fl", add_call="add_filter",
                                 draw=lambda rng, p: random_filter_params(rng), draw_keys=_random_key)


def write_projects(args):
    """(base dir, seeds) -> the project dirs written: project.lua + assets, meta.txt (the block length)."""
    return fx_rig.write_projects(random_filter_project, args)
