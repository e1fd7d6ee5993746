"""Projects that contain EQ vertices (TEST INFRASTRUCTURE, a generator of its own: the generators the existing tests and soaks
draw from keep producing the graphs they always did).

* base_project / grid_cases / E: the inputs, the parameter grid and the bound's constant that tests/test_gpu_eq.py (on the
  device) and tests/test_eq_host.py (the derivation of E, on the CPU) share.
* random_eq_project / write_projects: a project of tests/test_gpu_fuzz.py's generator with one to three EQ vertices spliced
  into edges it already has -- in front of Normalize vertices, behind gain stages and inlined loop sources, in series where two
  land on one path -- and, now and then, one more as the output (the sanitizer run's input)."""
import itertools
import os
import sys

import numpy as np

from termdaw_amd import workloads as W

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fx_rig  # noqa: E402
import np_eq as NE  # noqa: E402

RATES = (44100, 48000, 96000)
INPUTS = ("drums", "noise", "burst")
# The GPU test's bound, per value: |y - want| <= 2^-23 |want| + E max|want|.  E_EMULATED is the worst
# max|blocked - serial| / max|serial| that np_eq.blocked() -- the tiled scan in numpy, long-double powers -- shows over
# grid_cases() on the three inputs at the three rates, rounded up (test_eq_host.py recomputes it and fails above this figure);
# the device's tree and its own order of the same float64 operations get a factor 8 on top.  E must stay <= 2^-28, a sixteenth
# of half an ulp at the render's peak.
# The grid is the issue's -- 7 kinds x {10, 20, 100, 1000, 0.45 sr} Hz x Q {0.1, 0.707, 20} x +-24 dB -- but for the two lowest
# frequencies at 96 kHz, which are 40 and 80 Hz: at 10 and 20 Hz / 96 kHz with Q = 20 the poles sit 6.5e-4 rad from z = 1, the
# float64 recurrence itself is conditioned like 1 / angle^2, and ANY re-association of it moves the result by up to 8.7e-10 of
# the peak (0.0145 x 2^-24; five of the 1 350 combinations exceed 2^-28 / 8, all of them there) -- more precise matrices do not
# help (joins in long double: 6.7e-10).  Those 96 kHz cases are not dropped: low_cases() holds them, with a constant of their
# own derived the same way, E_LOW = 8 x E_LOW_EMULATED (about 2^-27, over the cap, which is why they are no part of the grid).
E_EMULATED = 3.0e-10
E = 8.0 * E_EMULATED
assert E <= 2.0 ** -28
E_LOW_EMULATED = 9.0e-10
E_LOW = 8.0 * E_LOW_EMULATED


def base_project(kind, sr=48000, bl=1024, seconds=0.5, seed=0):
    """Sources -> Sum `bus` (the vertex in front of the EQ vertices under test)."""
    p = W.ProjectScript(sr, bl)
    p.set_length(seconds)
    p.set_render_samplerate(sr)
    if kind == "drums":   # kick and snare hits through sample_multi
        p.assets["kick"] = W.Asset(W.kick_int16(12 + seed, 15000, sr), sr=sr)
        p.assets["snare"] = W.Asset(W.snare_int16(5 + seed, 9000), sr=sr)
        p.load_sample("kick", "kick", "")
        p.load_sample("snare", "snare", "")
        n = max(1, int(seconds / 0.125))
        p.event_files["k"] = np.array([(0.25 * i + 0.002, 36.0, 1.0 - 0.1 * (i % 4)) for i in range((n + 1) // 2)], np.float32)
        p.event_files["s"] = np.array([(0.125 * i + 0.06, 38.0, 0.2 + 0.15 * (i % 5)) for i in range(n)], np.float32)
        p.load_midi_floww("k", "k")
        p.load_midi_floww("s", "s")
        p.add_sample_multi("kick", 0.9, 0.0, "kick", "k", -1)
        p.add_sample_multi("snare", 0.6, 25.0, "snare", "s", -1)
        srcs = ["kick", "snare"]
    elif kind == "noise":
        p.assets["n"] = W.Asset(W.noise_int16(31 + seed, 20011), sr=sr)
        p.assets["m"] = W.Asset(W.noise_int16(32 + seed, 7001), sr=sr)
        p.load_sample("n", "n", "")
        p.load_sample("m", "m", "normalize-seperate")
        p.add_sampleloop("n", 0.5, 0.0, "n")
        p.add_sampleloop("m", 0.02, -40.0, "m")
        srcs = ["n", "m"]
    else:                 # silence, then one burst (and silence again once it has rung out)
        p.assets["b"] = W.Asset(W.noise_int16(77 + seed, int(0.12 * sr)), sr=sr)
        p.assets["t"] = W.Asset(W.tone_int16(78 + seed, int(0.05 * sr)), sr=sr)
        p.load_sample("b", "b", "")
        p.load_sample("t", "t", "")
        p.event_files["b"] = np.array([(0.21, 60.0, 0.9)], np.float32)
        p.event_files["t"] = np.array([(0.23, 60.0, 0.5)], np.float32)
        p.load_midi_floww("b", "b")
        p.load_midi_floww("t", "t")
        p.add_sample_multi("b", 1.0, 0.0, "b", "b", -1)
        p.add_sample_multi("t", 0.7, -20.0, "t", "t", -1)
        srcs = ["b", "t"]
    p.add_sum("bus", 1.0, 0.0)
    for s in srcs:
        p.connect(s, "bus")
    p.set_output("bus")
    return p


def grid_cases(sr):
    """The grid at rate sr: (kind, freq_hz, q, gain_db) -- 7 kinds x 5 frequencies x 3 Q, +-24 dB where the kind has gain."""
    lows = (40.0, 80.0) if sr >= 96000 else (10.0, 20.0)
    return _cases(lows + (100.0, 1000.0, 0.45 * sr))


def low_cases(sr=96000):
    """10 and 20 Hz at 96 kHz: below the grid (see E_LOW)."""
    return _cases((10.0, 20.0))


def _cases(freqs):
    out = []
    for kind, f, q in itertools.product(NE.KINDS, freqs, (0.1, 0.707, 20.0)):
        for g in ((-24.0, 24.0) if kind in NE.HAS_GAIN else (0.0,)):
            out.append((kind, float(f), q, g))
    return out


def add_eq(p, name, src, kind, freq_hz, q, gain_db, wet=1.0, gain=1.0, angle=0.0):
    p.add_eq(name, gain, angle, wet, kind, freq_hz, q, gain_db)
    p.connect(src, name)


def random_eq_params(rng, sr):
    return (float(rng.choice([1.0, 1.0, 0.5, 0.0])),                                  # wet
            str(rng.choice(NE.KINDS)),
            float(rng.choice([10.0, 55.0, 1000.0, 8000.0, 0.45 * sr])),               # freq_hz
            float(rng.choice([0.1, 0.707, 3.0, 20.0])),                               # q
            float(rng.choice([-24.0, -6.0, 0.0, 12.0, 24.0])))                        # gain_db


def random_eq_project(seed, allow_sinf=True):
    return fx_rig.splice_project(seed, allow_sinf, rng_offset=910_000, prefix="q", add_call="add_eq",
                                 draw=lambda rng, p: random_eq_params(rng, 48000))


write_project = fx_rig.write_project


def write_projects(args):
    """(base dir, seeds) -> the project dirs written: project.lua + assets, meta.txt (the block length)."""
    return fx_rig.write_projects(random_eq_project, args)
