"""Projects that contain delay vertices (TEST INFRASTRUCTURE, a generator of its own: the generators the existing tests and soaks
draw from keep producing the graphs they always did).

* grid_cases / E: the parameter grid and the bound's constant that tests/test_gpu_delay.py (on the device) and
  tests/test_delay_host.py (the derivation of E, on the CPU) share; the inputs are tests/eq_projects.py's (drums, noise, burst
  into a Sum `bus`).
* random_delay_project / write_projects: a project of tests/test_gpu_fuzz.py's generator with one to three delay vertices spliced
  into edges it already has and, now and then, one more as the output (the sanitizer run's input)."""
import itertools
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import eq_projects as EP  # noqa: E402
import fx_rig  # noqa: E402

RATES = EP.RATES
INPUTS = EP.INPUTS
base_project = EP.base_project
write_project = EP.write_project
# The grid: delay times x feedback x cross.  The times reach from the shortest the vertex takes (44 to 96 lanes: hundreds of
# steps, several tiles, the carry's threads-per-lane form) over a non-integer number of frames (7.3 ms) and a slapback (30 ms)
# to an echo of half the 0.5 s project (250 ms: two steps, the single-launch form).  Longer times do not sound inside the
# project (the burst input starts at 0.21 s) and are rendered by the 20 s test instead.
TIMES_MS = (1.0, 7.3, 30.0, 250.0)
FEEDBACKS = (0.0, 0.5, 0.98)
CROSSES = (0.0, 0.35, 1.0)
# The GPU test's bound, per value: |p' - p| <= 2^-23 |p| + E max|p|.  E_EMULATED is the worst max|blocked - serial| / max|serial|
# that np_delay.blocked() -- the tiled scan in numpy, long-double powers -- shows over grid_cases() on the three inputs at the
# three rates with every candidate tile length, rounded up (test_delay_host.py recomputes it and fails above this figure); the
# device's own order of the same float64 operations gets a factor 8 on top.  E must stay <= 2^-28, the EQ's cap.  (The
# emulation's worst is 6.85e-16 = 2^-50.4, at 1 ms / feedback 0.98 / 44.1 kHz on the burst input with 64 steps per tile, and no
# float32 value of the grid changes: G's entries are non-negative and below 1, nothing cancels, and the joins cost a few float64
# roundings of a sum that is at most 1 / (1 - 0.98) = 50 inputs large.)
E_EMULATED = 1.0e-15
E = 8.0 * E_EMULATED
assert E <= 2.0 ** -28


def grid_cases(sr=48000):
    """(time_ms, feedback, cross): the same 36 at every rate."""
    return [(t, f, c) for t, f, c in itertools.product(TIMES_MS, FEEDBACKS, CROSSES)]


def add_delay(p, name, src, time_ms, feedback, cross, wet=1.0, gain=1.0, angle=0.0):
    p.add_delay(name, gain, angle, wet, time_ms, feedback, cross)
    p.connect(src, name)


def random_delay_params(rng):
    return (float(rng.choice([1.0, 1.0, 0.5, 0.0])),                       # wet
            float(rng.choice([1.0, 1.5, 7.3, 21.4, 85.4, 250.0, 2000.0])), # time_ms (21.4 ms: above a 1 024-frame block at 48 kHz; 85.4: above a 4 096-frame chunk)
            float(rng.choice([0.0, 0.5, 0.98])),                           # feedback
            float(rng.choice([0.0, 0.35, 1.0])))                           # cross


def random_delay_project(seed, allow_sinf=True):
    return fx_rig.splice_project(seed, allow_sinf, rng_offset=920_000, prefix="d", add_call="add_delay",
                                 draw=lambda rng, p: random_delay_params(rng))


def write_projects(args):
    """(base dir, seeds) -> the project dirs written: project.lua + assets, meta.txt (the block length)."""
    return fx_rig.write_projects(random_delay_project, args)
