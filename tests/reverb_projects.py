"""Projects that contain reverb vertices (TEST INFRASTRUCTURE, a generator of its own: the generators the existing tests and
soaks draw from keep producing the graphs they always did).

* grid_cases / RATES / E: the parameter grid, the rates and the bound's constant that tests/test_gpu_reverb.py (on the device) and
  tests/test_reverb_host.py (the derivation of E, on the CPU) share; the inputs are tests/delay_projects.py's (drums, noise,
  burst into a Sum `bus`, 0.5 s).
* random_reverb_project / write_projects: a project of tests/test_gpu_fuzz.py's generator with one to three reverb vertices
  spliced into edges it already has and, now and then, one more as the output (the sanitizer run's input)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import delay_projects as DP  # noqa: E402
import fx_rig  # noqa: E402

RATES = (44100, 96000)
INPUTS = DP.INPUTS
base_project = DP.base_project
write_project = DP.write_project
# (room, damp, width, size).  The shortest line is llround(225 size sr / 44100) frames, so the window length B is
#   size 0.5: 64 at 44.1 kHz (112 frames), 128 at 96 kHz (245);  size 1 / 1.37: 128 (225 / 308 -> 256) and 256;  size 2: 256.
# damp 0 is the undamped comb (d1 = 0: the scan adds only zeros), damp 1 with room 1 the longest tail and the largest d1 (g = 0.98,
# d1 = 0.4); 1.37 makes every line length a rounded product.
CASES = ((0.5, 0.5, 1.0, 1.0), (0.0, 0.0, 0.0, 0.5), (1.0, 1.0, 0.5, 2.0), (0.84, 0.2, 1.0, 0.5), (0.3, 0.9, 0.25, 1.37))
# The GPU test's bound for form 1, per value: |p' - p| <= 2^-23 |p| + E max|p|.  E_EMULATED is the worst max|scan - serial| /
# max|serial| that np_reverb.process(form=1) -- k_reverb<1>'s windowed scan restated in numpy, long-double powers -- shows over
# grid_cases() on the three inputs at the two rates with every candidate window length B no longer than the shortest line, rounded
# up (test_reverb_host.py recomputes it and fails above this figure); the device's own order of the same float64 operations gets
# a factor 8 on top.  E must stay <= 2^-28, the EQ's cap.  (The emulation's worst is 5.6e-16 = 2^-50.7 of the peak, at room 0.3 /
# damp 0.9 / size 1.37 on the drums at 44.1 kHz with B = 64: d1 <= 0.4, so a carry is worth at most 0.4^(B / 64) of a lane's own
# sum one lane on, and the comb loop is stable with the gain 1 / (1 - g) <= 50 -- a few float64 roundings, nothing cancels.)
E_EMULATED = 1.0e-15
E = 8.0 * E_EMULATED
assert E <= 2.0 ** -28


def grid_cases():
    """(room, damp, width, size): the same five at every rate."""
    return list(CASES)


def add_reverb(p, name, src, room, damp, width, size, wet=1.0, gain=1.0, angle=0.0):
    p.add_reverb(name, gain, angle, wet, room, damp, width, size)
    p.connect(src, name)


def random_reverb_params(rng):
    return (float(rng.choice([1.0, 1.0, 0.5, 0.0])),              # wet
            float(rng.choice([0.0, 0.5, 0.84, 1.0])),             # room
            float(rng.choice([0.0, 0.2, 1.0])),                   # damp
            float(rng.choice([0.0, 0.5, 1.0])),                   # width
            float(rng.choice([0.5, 0.6, 1.0, 1.37, 2.0])))        # size (the sanitizer driver opens every project at 48 kHz: B = 64, 128, 128, 256, 256)


def random_reverb_project(seed, allow_sinf=True):
    return fx_rig.splice_project(seed, allow_sinf, rng_offset=950_000, prefix="r", add_call="add_reverb",
                                 draw=lambda rng, p: random_reverb_params(rng))


def write_projects(args):
    """(base dir, seeds) -> the project dirs written: project.lua + assets, meta.txt (the block length)."""
    return fx_rig.write_projects(random_reverb_project, args)
