"""Projects that contain limiter vertices (TEST INFRASTRUCTURE, a generator of its own: the generators the existing tests and
soaks draw from keep producing the graphs they always did).

* base_project / grid_cases / E: the inputs, the parameter grid and the bound's constant that tests/test_gpu_limiter.py (on the
  device) and tests/test_limiter_host.py (the derivation of E, on the CPU) share.  The inputs are the gate's three: eq_projects'
  drums and noise, and gate_projects' `gated` (noise at a constant level per segment: loud stretches, quiet ones, and steps
  between them that a lookahead has to ramp into).
* random_limiter_project / write_projects: a project of tests/test_gpu_fuzz.py's generator with one to three limiter vertices
  spliced into edges it already has, and, now and then, one more as the output (the sanitizer run's input)."""
import itertools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fx_rig  # noqa: E402
import gate_projects as GP  # noqa: E402

RATES = GP.RATES
INPUTS = GP.INPUTS
SECONDS = 0.25   # at least 5 tiles at every rate
# The GPU test's bound, per value: |p' - p| <= 2^-23 |p| + E max|p|.  E_EMULATED is the worst max|blocked - serial| / max|serial|
# of p before its f32 rounding that np_limiter.blocked() -- the kernels' lane runs, carries and prefix sums in numpy -- shows
# against the serial twin over grid_cases() on the three inputs at the three rates, rounded up (test_limiter_host.py recomputes it
# and fails above this figure); the device's own order of the same float64 operations gets the project's factor 8 on top.  The
# largest figures come from L = 1 and 2, where G is a difference of two prefix sums hundreds of times its size, at the grid's
# deepest reduction.  E must stay <= 2^-28, the EQ's cap.
E_EMULATED = 4e-11
E = 8.0 * E_EMULATED
assert E <= 2.0 ** -28

RELEASES = (1.0, 50.0, 1000.0)
LEVELS = ((-6.0, 12.0), (-0.1, 0.0), (-24.0, 24.0))   # (ceiling_db, drive_db)


def windows(sr):
    """The grid's L: 1, 2, about 1 ms, about 10 ms, exactly 2 048 frames."""
    return (1, 2, int(round(sr / 1000.0)), int(round(sr / 100.0)), 2048)


def lookahead_ms(sr, L):
    """A lookahead_ms (as the f32 the engine gets) whose window is L frames at rate sr; 0 for L = 1."""
    return 0.0 if L == 1 else float(np.float32(L * 1000.0 / sr))


def grid_cases(sr):
    """(ceiling_db, lookahead_ms, release_ms, drive_db): the issue's grid, 45 cases, with the L each one means."""
    return [((ce, lookahead_ms(sr, L), re, dr), L) for L, re, (ce, dr) in itertools.product(windows(sr), RELEASES, LEVELS)]


def base_project(kind, sr=48000, bl=1024, seconds=SECONDS, seed=0):
    """Sources -> Sum `bus` (the vertex in front of the limiter vertices under test)."""
    return GP.base_project(kind, sr=sr, bl=bl, seconds=seconds, seed=seed)


def add_limiter(p, name, src, case, wet=1.0, gain=1.0, angle=0.0):
    p.add_limiter(name, gain, angle, wet, *case)
    p.connect(src, name)


def oracle_input(kind, sr):
    return fx_rig.oracle_input(kind, sr, base_project)


def random_limiter_params(rng, sr):
    L = int(rng.choice([1, 2, 48, 480, 2048]))
    return (float(rng.choice([1.0, 1.0, 0.5, 0.0])),                 # wet
            float(rng.choice([-24.0, -6.0, -0.1, 0.0])),              # ceiling_db
            lookahead_ms(sr, L),                                      # lookahead_ms
            float(rng.choice([1.0, 50.0, 1000.0, 10000.0])),          # release_ms
            float(rng.choice([-24.0, 0.0, 12.0, 24.0])))              # drive_db


def random_limiter_project(seed, allow_sinf=True):
    return fx_rig.splice_project(seed, allow_sinf, rng_offset=990_000, prefix="lm", add_call="add_limiter",
                                 draw=lambda rng, p: random_limiter_params(rng, p.psr))


def write_projects(args):
    """(base dir, seeds) -> the project dirs written: project.lua + assets, meta.txt (the block length)."""
    return fx_rig.write_projects(random_limiter_project, args)
