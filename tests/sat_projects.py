"""Projects that contain saturator vertices (TEST INFRASTRUCTURE, a generator of its own: the generators the existing tests and
soaks draw from keep producing the graphs they always did).

* base_project / grid_cases: the inputs and the parameter grid tests/test_gpu_saturator.py runs on the device -- a drum bus, a sum
  of sines, noise at -20 and at +6 dBFS into a Sum `bus`, 0.25 s.
* random_sat_project / write_projects: a project of tests/test_gpu_fuzz.py's generator with one to three saturator vertices
  spliced into edges it already has and, now and then, one more as the output (the sanitizer run's input)."""
import itertools
import os
import sys

import numpy as np

from termdaw_amd import workloads as W

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import eq_projects as EP  # noqa: E402
import fx_rig  # noqa: E402
import np_saturator as NS  # noqa: E402

INPUTS = ("drums", "sines", "noise-20", "noise+6")
write_project = EP.write_project
OVERSAMPLE = (1, 2, 4, 8)
DRIVE_BIAS = ((0.0, 0.0), (12.0, 0.2), (36.0, -0.5))


def sines_int16(frames):
    """997 Hz + 5 kHz + 9 kHz at 48 kHz, 0.9 of full scale together, the right channel the left one with the middle tone turned over."""
    t = np.arange(frames, dtype=np.float64) / 48000.0
    a, b, c = (np.sin(2.0 * np.pi * f * t) for f in (997.0, 5000.0, 9000.0))
    l, r = 0.4 * a + 0.3 * b + 0.2 * c, 0.4 * a - 0.3 * b + 0.2 * c
    return np.round(np.stack([l, r], axis=1) * 32767.0).astype(np.int16)


def base_project(kind, bl=1024, seconds=0.25, seed=0):
    """Sources -> Sum `bus` (the vertex in front of the saturator vertices under test), 48 kHz."""
    if kind == "drums":
        return EP.base_project("drums", bl=bl, seconds=seconds, seed=seed)
    p = W.ProjectScript(48000, bl)
    p.set_length(seconds)
    p.set_render_samplerate(48000)
    if kind == "sines":
        p.assets["t"] = W.Asset(sines_int16(4801 + seed))
        p.load_sample("t", "t", "")
        p.add_sampleloop("t", 1.0, 0.0, "t")
        srcs = ["t"]
    else:   # uniform noise with its peak at 0.1 (-20 dBFS) or 2.0 (+6 dBFS), a second, quiet one panned beside it
        level = {"noise-20": 0.1, "noise+6": 2.0}[kind]
        p.assets["n"] = W.Asset(W.noise_int16(31 + seed, 20011))
        p.assets["m"] = W.Asset(W.noise_int16(32 + seed, 7001))
        p.load_sample("n", "n", "")
        p.load_sample("m", "m", "")
        p.add_sampleloop("n", level, 0.0, "n")
        p.add_sampleloop("m", 0.02 * level, -40.0, "m")
        srcs = ["n", "m"]
    p.add_sum("bus", 1.0, 0.0)
    for s in srcs:
        p.connect(s, "bus")
    p.set_output("bus")
    return p


def grid_cases():
    """(kind, drive_db, bias, out_db, oversample): 3 kinds x 4 factors x 3 (drive, bias)."""
    return [(k, d, b, 0.0, R) for k, R, (d, b) in itertools.product(NS.KINDS, OVERSAMPLE, DRIVE_BIAS)]


def add_saturator(p, name, src, kind, drive_db, bias, out_db, oversample, wet=1.0, gain=1.0, angle=0.0):
    p.add_saturator(name, gain, angle, wet, kind, drive_db, bias, out_db, oversample)
    p.connect(src, name)


def random_sat_params(rng):
    return (float(rng.choice([1.0, 1.0, 0.5, 0.0])),            # wet
            str(rng.choice(NS.KINDS)),
            float(rng.choice([-24.0, 0.0, 12.0, 48.0])),         # drive_db
            float(rng.choice([-1.0, 0.0, 0.2, 1.0])),            # bias
            float(rng.choice([-48.0, -6.0, 0.0, 24.0])),         # out_db
            int(rng.choice([1, 2, 4, 8])))


def random_sat_project(seed, allow_sinf=True):
    return fx_rig.splice_project(seed, allow_sinf, rng_offset=930_000, prefix="w", add_call="add_saturator",
                                 draw=lambda rng, p: random_sat_params(rng))


def write_projects(args):
    """(base dir, seeds) -> the project dirs written: project.lua + assets, meta.txt (the block length)."""
    return fx_rig.write_projects(random_sat_project, args)
