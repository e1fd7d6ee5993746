"""Projects that contain chorus vertices (TEST INFRASTRUCTURE, a generator of its own: the generators the existing tests and
soaks draw from keep producing the graphs they always did).

* base_project / grid_cases: the inputs and the parameter grid tests/test_gpu_chorus.py runs on the device -- a drum bus, a sum of
  sines, noise at -20 and at +6 dBFS into a Sum `bus`, 0.25 s at 48 kHz (tests/sat_projects.py's).
* random_chorus_project / write_projects: a project of tests/test_gpu_fuzz.py's generator with one to three chorus vertices spliced
  into edges it already has and, now and then, one more as the output (the sanitizer run's input)."""
import itertools
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fx_rig  # noqa: E402
import np_chorus as NC  # noqa: E402
import sat_projects as SP  # noqa: E402

INPUTS = SP.INPUTS
base_project = SP.base_project
write_project = SP.write_project
VOICES = (1, 2, 4)
# (delay_ms, depth_ms, rate_hz, stereo) at 48 kHz: a line of 192 frames, below one tile; one of 2 432 frames, the longest the ranges
# allow, with the delay slope at 0.47 (sine) / 0.30 (triangle) frames per frame; the right channel a quarter cycle ahead
SHORT, LONG, WIDE = (2.0, 1.0, 5.0, 0.0), (40.0, 9.9, 7.5, 0.0), (15.0, 3.0, 1.3, 0.25)
TRIPLES = (SHORT, LONG, WIDE)


def case(voices, triple, shape):
    """The arguments of add_chorus behind (name, gain, angle, wet)."""
    return (voices,) + tuple(triple) + (shape,)


def grid_cases():
    """(voices, delay_ms, depth_ms, rate_hz, stereo, shape): 2 shapes x 3 voice counts x 3 triples."""
    return [case(V, t, s) for s, V, t in itertools.product(NC.SHAPES, VOICES, TRIPLES)]


def add_chorus(p, name, src, voices, delay_ms, depth_ms, rate_hz, stereo, shape, wet=1.0, gain=1.0, angle=0.0):
    p.add_chorus(name, gain, angle, wet, voices, delay_ms, depth_ms, rate_hz, stereo, shape)
    p.connect(src, name)


def random_chorus_params(rng):
    delay, depth, rate = [(0.5, 0.0, 20.0), (2.0, 1.0, 5.0), (20.0, 5.0, 0.5), (40.0, 9.9, 7.5), (7.0, 6.9, 0.01)][int(rng.integers(0, 5))]
    return (float(rng.choice([1.0, 1.0, 0.5, 0.0])),            # wet
            int(rng.integers(1, 5)), delay, depth, rate,
            float(rng.choice([0.0, 0.25, 0.5])),                 # stereo
            str(rng.choice(NC.SHAPES)))


def random_chorus_project(seed, allow_sinf=True):
    return fx_rig.splice_project(seed, allow_sinf, rng_offset=940_000, prefix="c", add_call="add_chorus",
                                 draw=lambda rng, p: random_chorus_params(rng))


def write_projects(args):
    """(base dir, seeds) -> the project dirs written: project.lua + assets, meta.txt (the block length)."""
    return fx_rig.write_projects(random_chorus_project, args)
