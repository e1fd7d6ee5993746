"""Projects that contain phaser vertices (TEST INFRASTRUCTURE, a generator of its own: the generators the existing tests and
soaks draw from keep producing the graphs they always did).

* base_project / grid_cases / E: the inputs, the parameter grid and the bound's constant that tests/test_gpu_phaser.py (on the
  device) and tests/test_phaser_host.py (the derivation of E, on the CPU) share.  The inputs are eq_projects': drums, noise and a
  burst between silences.
* random_phaser_project / write_projects: a project of tests/test_gpu_fuzz.py's generator with one to three phaser vertices
  spliced into edges it already has and, now and then, one more as the output (the sanitizer run's input)."""
import itertools
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import eq_projects as EP  # noqa: E402
import fx_rig  # noqa: E402
import np_phaser as NP  # noqa: E402

RATES = EP.RATES
INPUTS = EP.INPUTS
SHAPES = ("sine", "triangle")
# The GPU test's bound, per value: |y - want| <= 2^-23 |want| + E max|want|.  E_EMULATED is the worst
# max|blocked - serial| / max|serial| that np_phaser.blocked() -- the tiled scan in numpy, with the kernels' tile geometry and
# join order -- shows over grid_cases() on the three inputs at the three rates, rounded up (test_phaser_host.py recomputes it and
# fails above this figure); the device's own order of the same float64 operations gets the project's factor 8 on top.  E must
# stay <= 2^-28, a sixteenth of half an f32 ulp at the render's peak.
E_EMULATED = 2.0e-14
E = 8 * E_EMULATED
assert E <= 2 ** -28

base_project = EP.base_project


def grid_cases(sr):
    """(stages, lo_hz, hi_hz, rate_hz, feedback, stereo, shape): the issue's grid at rate sr, 108 cases -- stages x sweep x rate x
    feedback; shape and stereo alternate with the case's index, so that all four pairs occur."""
    out = []
    for i, (n, (lo, hi), rate, fb) in enumerate(itertools.product((2, 4, 6, 8), ((20.0, 0.45 * sr), (200.0, 2000.0), (1000.0, 1000.0)),
                                                                  (0.01, 1.0, 20.0), (-0.95, 0.0, 0.95))):
        out.append((n, lo, hi, rate, fb, 0.25 * ((i // 2) % 2), SHAPES[i % 2]))
    return out


def spec(api, sr, case):
    """What np_phaser takes, on the engine's own constants."""
    return NP.spec(api.phaser_params(sr, *case), case[5], case[6])


def add_phaser(p, name, src, case, wet=1.0, gain=1.0, angle=0.0):
    p.add_phaser(name, gain, angle, wet, *case)
    p.connect(src, name)


def random_phaser_params(rng):
    lo, hi = [(20.0, 21600.0), (200.0, 2000.0), (1000.0, 1000.0), (20.0, 20.0)][int(rng.integers(0, 4))]   # (the driver opens every project at 48 kHz)
    return (float(rng.choice([1.0, 1.0, 0.5, 0.0])),                     # wet
            int(rng.choice([2, 4, 6, 8])), lo, hi,
            float(rng.choice([0.01, 1.0, 20.0])),                         # rate_hz
            float(rng.choice([-0.95, 0.0, 0.5, 0.95])),                   # feedback
            float(rng.choice([0.0, 0.25, 0.5])),                          # stereo
            str(rng.choice(SHAPES)))


def random_phaser_project(seed, allow_sinf=True):
    return fx_rig.splice_project(seed, allow_sinf, rng_offset=990_000, prefix="ph", add_call="add_phaser",
                                 draw=lambda rng, p: random_phaser_params(rng))


def write_projects(args):
    """(base dir, seeds) -> the project dirs written: project.lua + assets, meta.txt (the block length)."""
    return fx_rig.write_projects(random_phaser_project, args)
