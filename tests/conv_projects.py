"""Projects that contain convolution vertices (TEST INFRASTRUCTURE, a generator of its own: the generators the existing tests and
soaks draw from keep producing the graphs they always did).

* base_project / responses / grid_cases / E: the inputs (tests/delay_projects.py's drums, noise and burst, 0.5 s, at 44 100 and
  96 000 Hz), the impulse responses, the parameter grid and the bound's constant that tests/test_gpu_convolution.py (on the
  device) and tests/test_convolution_host.py (the derivation of E, on the CPU) share.  The grid is written for the kernels'
  partition B = 1 024 frames and moves with it: response lengths on both sides of one, two and three partitions, pre-delays
  that shift the response by a frame and by a whole partition.
* random_convolution_project / write_projects: a project of tests/test_gpu_fuzz.py's generator with one to three convolution
  vertices spliced into edges it already has and, now and then, one more as the output (the sanitizer run's input)."""
import itertools
import os
import sys

import numpy as np

from termdaw_amd import workloads as W

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import delay_projects as DP  # noqa: E402
import fx_rig  # noqa: E402
import np_convolution as NC  # noqa: E402

RATES = (44100, 96000)
INPUTS = DP.INPUTS
SECONDS = 0.5
B = NC.B
LENGTHS = (1, 2, B - 1, B, B + 1, 2 * B, 2 * B + 1, 3 * B + 1)
PREDELAYS = (0, 1, B)       # frames
NORMS = (0, 1)
CAP = 262144
SPARSE_TAPS = (0, B - 1, B, CAP // 2 - 1, CAP - 1)
SPARSE_SECONDS = 6.0
# The GPU test's bound, per value: |p' - p| <= 2^-23 |p| + E max|p|.  E_EMULATED is the worst max|emulation - direct| /
# max|direct| of p before its f32 rounding that np_convolution.emulate() -- the kernels' transforms, twiddle table and order over
# the partitions in numpy -- shows against the long-double direct sum over grid_cases() on the three inputs at the two rates and
# over the sparse response at the cap, rounded up (test_convolution_host.py recomputes it and fails above this figure); the
# device's own order of the same float64 operations gets the project's factor 8 on top.  E must stay <= 2^-28, the EQ's cap.
# The emulation's worst is 9.71e-16 = 2^-49.9, at Lh = 2 with a pre-delay of one frame, normalised, on the noise input at 96 kHz --
# among the shortest responses: there the direct sum is one or two products and carries next to no error of its own, while the
# transforms spread the 2 x 11 butterfly roundings of a 2 048-point window over every output frame and the output's peak is no
# larger than the input's.  The longer responses and the 256 partitions of the sparse one stay below it: their roundings are
# independent, and the output's peak grows with the response.
E_EMULATED = 1.0e-15
E = 8.0 * E_EMULATED
assert E <= 2.0 ** -28


def response_int16(Lh, seed):
    """A dense, decaying, random stereo response of Lh frames as int16 words, the two channels drawn apart; frame 0 is loud."""
    rng = np.random.default_rng(4100 + 7 * seed + Lh)
    env = np.exp(-5.0 * np.arange(Lh) / max(Lh, 1))[:, None]
    h = rng.uniform(-1.0, 1.0, (Lh, 2)) * env * np.array([[0.9, 0.7]])
    h[0] = (0.8, -0.6)
    return np.round(h * 32767.0).astype(np.int16)


def sparse_int16():
    """The response at the cap: zero but for five taps."""
    h = np.zeros((CAP, 2), np.int16)
    for i, k in enumerate(SPARSE_TAPS):
        h[k] = (20000 - 3000 * i, -9000 + 5000 * i)
    return h


def predelay_ms(sr, D):
    """A predelay_ms (as the f32 the engine gets) that is D frames at rate sr."""
    return float(np.float32(D * 1000.0 / sr))


def base_project(kind, sr=48000, bl=1024, seconds=SECONDS, seed=0):
    """Sources -> Sum `bus` (the vertex in front of the convolution vertices under test)."""
    return DP.base_project(kind, sr=sr, bl=bl, seconds=seconds, seed=seed)


def load_response(p, name, pcm):
    """The response as a sample of the project, at the project's rate (no resampling)."""
    p.assets[name] = W.Asset(pcm, sr=p.psr)
    p.load_sample(name, name, "")


def add_convolution(p, name, src, case, wet=1.0, gain=1.0, angle=0.0):
    """case: (sample, length_ms, predelay_ms, out_db, norm)."""
    p.add_convolution(name, gain, angle, wet, *case)
    p.connect(src, name)


def grid_cases(sr):
    """((sample, length_ms, predelay_ms, out_db, norm), Lh, D): 48 cases over eight responses "h<Lh>"."""
    out = []
    for Lh, D, norm in itertools.product(LENGTHS, PREDELAYS, NORMS):
        out.append((("h%d" % Lh, 0.0, predelay_ms(sr, D), -3.0 if norm else -12.0, norm), Lh, D))
    return out


def load_grid_responses(p, seed=0):
    for Lh in LENGTHS:
        load_response(p, "h%d" % Lh, response_int16(Lh, seed))


def oracle_input(kind, sr, seconds=SECONDS):
    return fx_rig.oracle_input(kind, sr, lambda k, sr: base_project(k, sr=sr, seconds=seconds))


def random_convolution_params(rng, p):
    """Draws a response for the vertex too: a sample of its own, loaded into the project."""
    Lh = int(rng.choice([1, 2, 700, 1024, 1025, 5000, 70000]))
    name = "ir%d" % len([k for k in p.assets if k.startswith("ir")])
    load_response(p, name, response_int16(Lh, 3) if Lh < 70000 else np.ones((Lh, 2), np.int16))
    # (the load goes to the script's end, behind everything the splice still indexes: the front end loads the samples in front
    # of the graph wherever the lines stand)
    return (float(rng.choice([1.0, 1.0, 0.5, 0.0])),                  # wet
            name,
            float(rng.choice([0.0, 0.0, 10.0])),                      # length_ms (10 ms: 480 frames of it)
            float(rng.choice([0.0, 1.0, 21.4, 500.0])),               # predelay_ms
            float(rng.choice([-60.0, -6.0, 0.0, 24.0])),              # out_db
            int(rng.choice([0, 1])))                                  # norm


def random_convolution_project(seed, allow_sinf=True):
    return fx_rig.splice_project(seed, allow_sinf, rng_offset=1_010_000, prefix="cv", add_call="add_convolution",
                                 draw=random_convolution_params)


def write_projects(args):
    """(base dir, seeds) -> the project dirs written: project.lua + assets, meta.txt (the block length)."""
    return fx_rig.write_projects(random_convolution_project, args)
