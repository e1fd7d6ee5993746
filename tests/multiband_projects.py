"""Projects that contain multiband vertices (TEST INFRASTRUCTURE, a generator of its own: the generators the existing tests and
soaks draw from keep producing the graphs they always did).

* grid_cases / E: the parameter grid and the bound's constant that tests/test_gpu_multiband.py (on the device) and
  tests/test_multiband_host.py (the derivation of E, on the CPU) share.  The inputs are eq_projects': drums, noise and a burst
  between silences (eq_projects.base_project's `bus`).
* random_multiband_project / write_projects: a project of tests/test_gpu_fuzz.py's generator with one to three multiband vertices
  spliced into edges it already has (the sanitizer run's input)."""
import itertools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import eq_projects as EP  # noqa: E402
import fx_rig  # noqa: E402
import np_multiband as NM  # noqa: E402

RATES = EP.RATES
INPUTS = EP.INPUTS
# The GPU test's bound on p, per value: |p' - p| <= 2^-23 |p| + E max|p|.  E_EMULATED is the worst
# max|blocked - serial| / max|serial| of p that np_multiband.blocked() -- the crossover's tiled scans in numpy, with the kernels'
# tile geometry, the 18-state block operator and its join order, long-double powers -- shows over grid_cases() on the three inputs
# at the three rates, rounded up to two digits (test_multiband_host.py recomputes it and fails above this figure); the device's
# log10 / exp10 and its rounding of the detectors' joins get the project's factor 8 on top.  E must stay <= 2^-28.
# The grid is the issue's whole, 81 cases per rate and input; the worst figure is the (40, 80) Hz crossover's at 96 kHz -- the poles
# nearest z = 1 -- on the drums, with the low band at -60 dB and 1000:1, where a band signal's error goes through the logarithm at
# full slope: 3.39e-11 against 2^-28 / 8 = 4.7e-10.  No side grid is needed.
E_EMULATED = 3.4e-11
E = 8 * E_EMULATED
assert E <= 2 ** -28

# (T, R, M) per band -- low, mid, high: all three working alike; three different jobs (a hard limiter at the lowest threshold,
# a gentle one with make-up, a band left alone but turned down); only the high band working (a de-esser)
BAND_SETTINGS = (
    ((-30.0, 4.0, 0.0), (-30.0, 4.0, 0.0), (-30.0, 4.0, 0.0)),
    ((-60.0, 1000.0, 0.0), (-12.0, 2.0, 12.0), (0.0, 1.0, -12.0)),
    ((0.0, 1.0, 0.0), (0.0, 1.0, 0.0), (-40.0, 8.0, 0.0)),
)
KNEES = (0.0, 6.0, 40.0)
TIMES = ((0.0, 1.0), (5.0, 50.0), (1000.0, 10000.0))   # (attack_ms, release_ms)


def crossovers(sr):
    return ((40.0, 80.0), (200.0, 2000.0), (1000.0, 0.45 * sr))


def case(lo, hi, bands, knee, times):
    """(lo_hz, hi_hz, threshold_db, ratio, attack_ms, release_ms, knee_db, makeup_db): add_multiband's arguments behind `wet`."""
    return (lo, hi, tuple(b[0] for b in bands), tuple(b[1] for b in bands), times[0], times[1], knee, tuple(b[2] for b in bands))


def grid_cases(sr):
    """The issue's grid at rate sr, 81 cases."""
    return [case(lo, hi, b, k, t) for (lo, hi), b, k, t in itertools.product(crossovers(sr), BAND_SETTINGS, KNEES, TIMES)]


def spec(api, sr, c):
    """What np_multiband takes, on the engine's own constants."""
    return NM.spec(api.multiband_params(sr, *c), c[2], c[3], c[6], c[7])


def add_multiband(p, name, src, c, wet=1.0, gain=1.0, angle=0.0):
    p.add_multiband(name, gain, angle, wet, *c)
    p.connect(src, name)


def random_multiband_params(rng):
    lo, hi = [(40.0, 80.0), (200.0, 2000.0), (1000.0, 21600.0)][int(rng.integers(0, 3))]   # (the driver opens every project at 48 kHz)
    b = BAND_SETTINGS[int(rng.integers(0, 3))]
    return (float(rng.choice([1.0, 1.0, 0.5, 0.0])),) + case(lo, hi, b, float(rng.choice(KNEES)), TIMES[int(rng.integers(0, 3))])


def random_multiband_project(seed, allow_sinf=True):
    return fx_rig.splice_project(seed, allow_sinf, rng_offset=1_212_000, prefix="mb", add_call="add_multiband",
                                 draw=lambda rng, p: random_multiband_params(rng), as_output=False)


def write_projects(args):
    """(base dir, seeds) -> the project dirs written: project.lua + assets, meta.txt (the block length)."""
    return fx_rig.write_projects(random_multiband_project, args)


# ---- the two-tone case of the non-vacuity tests (host and GPU) ----
TONE_CASE = (400.0, 3000.0, (0.0, 0.0, -30.0), (1.0, 1.0, 4.0), 5.0, 50.0, 6.0, (0.0, 0.0, 0.0))


def tone_lines(y, sr=48000):
    """(100 Hz, 8 kHz): the two lines' amplitudes over the last 8 192 frames, in dB."""
    seg = y[-8192:, 0].astype(np.float64)
    t = np.arange(len(seg)) / sr
    w = np.hanning(len(seg))
    return tuple(20.0 * np.log10(2.0 * abs(np.sum(seg * w * np.exp(-2j * np.pi * f * t))) / w.sum()) for f in (100.0, 8000.0))
