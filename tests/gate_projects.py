"""Projects that contain gate vertices (TEST INFRASTRUCTURE, a generator of its own: the generators the existing tests and soaks
draw from keep producing the graphs they always did).

* base_project / grid_cases / E: the inputs, the parameter grid and the bound's constant that tests/test_gpu_gate.py (on the
  device) and tests/test_gate_host.py (the derivation of E, on the CPU) share.  The inputs are eq_projects' drums and noise and
  one made for the gate, `gated`: noise at a constant level per segment (SEGMENTS), so that every transition of the definition
  happens at a known place.
* random_gate_project / write_projects: a project of tests/test_gpu_fuzz.py's generator with one to three gate vertices spliced
  into edges it already has, and, now and then, one more as the output (the sanitizer run's input)."""
import itertools
import os
import sys

import numpy as np

from termdaw_amd import workloads as W

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import eq_projects as EP  # noqa: E402
import fx_rig  # noqa: E402

RATES = (44100, 48000, 96000)
INPUTS = ("drums", "noise", "gated")
# The GPU test's bound, per value: |p' - p| <= 2^-23 |p| + E max|p|.  E_EMULATED is the worst max|blocked - serial| of env (full
# scale 1: env lies in [0, 1]) that np_gate.blocked() -- the tiled scan in numpy -- shows over grid_cases() on the three inputs at
# the three rates with every tiling of TILINGS, rounded up (test_gate_host.py recomputes it and fails above this figure); the
# device's own order of the same float64 operations gets the project's factor 8 on top.  E must stay <= 2^-28, the EQ's cap.
E_EMULATED = 2.5e-13
E = 8.0 * E_EMULATED
assert E <= 2.0 ** -28
# (tile, run, carry lanes): the kernels' own, a shorter run, a shorter and a longer tile, and carry lanes that fold two tiles each
# on a 12-tile render (three on 24 tiles)
TILINGS = ((2048, 8, 256), (2048, 4, 256), (1024, 8, 256), (4096, 16, 256), (2048, 8, 8))

# `gated`: (level dB, frames).  For threshold_db -30, hysteresis_db 6 "band" (-33 dB) lies between the thresholds, -12 dB above, -50
# dB below.  24 000 frames, 12 tiles; the band segments and the long quiet one each cross a multiple of 2 048.
SEGMENTS = ((-12, 3000), (-33, 2500), (-50, 700), (-12, 500), (-50, 6000), (-33, 3000), (-12, 100), (-50, 300), (-33, 1500), (-50, 4000),
            (-12, 1200), (-50, 1200))
GATED_FRAMES = sum(n for _, n in SEGMENTS)
assert GATED_FRAMES == 24000
# The sample bank scales a loaded sample to its peak (the loud segments come out at 0 dB), so the loop plays it 12 dB down: that
# puts every segment at its level.
GATED_GAIN = 10.0 ** (-12.0 / 20.0)


def gated_int16(seed=0):
    """Every frame's level is its segment's to within a fifth of a dB: |noise| in [0.98, 1] of the level, random sign, quantised
    to int16; the right channel at 0.8 of the left."""
    rng = np.random.default_rng(4200 + seed)
    parts = []
    for db, n in SEGMENTS:
        a = 10.0 ** (db / 20.0) * 32767.0
        parts.append(rng.choice([-1.0, 1.0], n) * rng.uniform(0.98, 1.0, n) * a)
    l = np.concatenate(parts)
    return np.stack([np.round(l), np.round(0.8 * l)], axis=1).astype(np.int16)


def gated_frames(seed=0):
    """`gated` as the loop hands it on, restated without a device (to within an f32 rounding): float32 (24 000, 2)."""
    g = gated_int16(seed).astype(np.float32)
    return (g / np.abs(g).max()) * np.float32(GATED_GAIN)


def base_project(kind, sr=48000, bl=1024, seconds=0.5, seed=0):
    """Sources -> Sum `bus` (the vertex in front of the gate vertices under test)."""
    if kind != "gated":
        return EP.base_project(kind, sr=sr, bl=bl, seconds=seconds, seed=seed)
    p = W.ProjectScript(sr, bl)
    p.set_length(seconds)
    p.set_render_samplerate(sr)
    p.assets["g"] = W.Asset(gated_int16(seed), sr=sr)   # (played as it is at every rate: one decoded asset, looped)
    p.load_sample("g", "g", "")
    p.add_sampleloop("src", GATED_GAIN, 0.0, "g")
    p.add_sum("bus", 1.0, 0.0)
    p.connect("src", "bus")
    p.set_output("bus")
    return p


THRESHOLD = -30.0


def grid_cases():
    """(threshold_db, hysteresis_db, hold_ms, attack_ms, release_ms, range_db): the issue's grid, 108 cases."""
    return [(THRESHOLD, hy, ho, at, re, ra) for hy, at, re, ho, ra in
            itertools.product((0.0, 6.0), (0.0, 1.0, 40.0), (1.0, 100.0, 2000.0), (0.0, 10.0, 60.0), (-120.0, -20.0))]


def add_gate(p, name, src, case, wet=1.0, gain=1.0, angle=0.0):
    p.add_gate(name, gain, angle, wet, *case)
    p.connect(src, name)


def random_gate_params(rng):
    return (float(rng.choice([1.0, 1.0, 0.5, 0.0])),                       # wet
            float(rng.choice([-80.0, -40.0, -30.0, -12.0, 0.0])),           # threshold_db
            float(rng.choice([0.0, 6.0, 24.0])),                            # hysteresis_db
            float(rng.choice([0.0, 10.0, 60.0, 2000.0])),                   # hold_ms
            float(rng.choice([0.0, 1.0, 40.0, 1000.0])),                    # attack_ms
            float(rng.choice([1.0, 100.0, 2000.0, 10000.0])),               # release_ms
            float(rng.choice([-120.0, -20.0, 0.0])))                        # range_db


def random_gate_project(seed, allow_sinf=True):
    return fx_rig.splice_project(seed, allow_sinf, rng_offset=970_000, prefix="g", add_call="add_gate",
                                 draw=lambda rng, p: random_gate_params(rng))


def write_projects(args):
    """(base dir, seeds) -> the project dirs written: project.lua + assets, meta.txt (the block length)."""
    return fx_rig.write_projects(random_gate_project, args)
