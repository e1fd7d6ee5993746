"""Projects that contain vocoder vertices (TEST INFRASTRUCTURE, a generator of its own: the generators the existing tests and
soaks draw from keep producing the graphs they always did).

* base_project / PAIRS / grid_cases / E: the inputs, the parameter grid and the bound's constant that tests/test_gpu_vocoder.py
  (on the device) and tests/test_vocoder_host.py (the derivation of E, on the CPU) share.  The inputs are eq_projects': drums,
  noise and a burst between silences, each as carrier (`bus`) with another of the three as key (`kbus`).
* random_vocoder_project / write_projects: a project of tests/test_gpu_fuzz.py's generator with one to three vocoder vertices
  spliced into edges it already has, most of them keyed by another vertex of the project (the sanitizer run's input)."""
import itertools
import os
import sys

import numpy as np

from termdaw_amd import workloads as W

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import eq_projects as EP  # noqa: E402
import fx_rig  # noqa: E402
import np_vocoder as NV  # noqa: E402

RATES = EP.RATES
INPUTS = EP.INPUTS
PAIRS = (("drums", "noise"), ("noise", "burst"), ("burst", "drums"))   # (carrier, key)
# The GPU test's bound on p, per value: |p' - p| <= 2^-23 |p| + E max|p|.  E_EMULATED is the worst
# max|blocked - serial| / max|serial| that np_vocoder.blocked() -- the tiled scans in numpy, with the kernels' tile geometry and join
# order, long-double powers -- shows over grid_cases() on the three pairs at the three rates, rounded up (test_vocoder_host.py
# recomputes it and fails above this figure); the device's own order of the same float64 operations gets the project's factor 8 on
# top.  E must stay <= 2^-28, a sixteenth of half an f32 ulp at the render's peak.
# The grid is the issue's whole: bands {4, 8, 16} x sweep {(40, 0.45 sr), (200, 4000), (1000, 1001)} x q {0.5, 4, 20} x response_ms
# {0.1, 10, 1000}, 81 cases per rate.  The corner the issue was wary of -- q = 20 from 40 Hz at 96 kHz, poles 2.6e-3 rad from z = 1 --
# stays inside: 2.2e-12 is the worst figure and it is that corner's (burst keyed by drums, 8 bands), against 2^-28 / 8 = 4.7e-10.
# No side grid is needed.
E_EMULATED = 2.5e-12
E = 8 * E_EMULATED
assert E <= 2 ** -28

BANDS = (4, 8, 16)
QS = (0.5, 4.0, 20.0)
RESPONSES = (0.1, 10.0, 1000.0)


def sweeps(sr):
    return ((40.0, 0.45 * sr), (200.0, 4000.0), (1000.0, 1001.0))


def grid_cases(sr):
    """(bands, lo_hz, hi_hz, q, response_ms, out_db): the issue's grid at rate sr, 81 cases; out_db alternates between 12 and 0
    with the case's index."""
    return [(b, lo, hi, q, ms, 0.0 if i % 2 else 12.0)
            for i, (b, (lo, hi), q, ms) in enumerate(itertools.product(BANDS, sweeps(sr), QS, RESPONSES))]


def spec(api, sr, case):
    """What np_vocoder takes, on the engine's own constants."""
    return NV.spec(api.vocoder_params(sr, *case))


def _sources(p, kind, pre, sr, seconds):
    """eq_projects.base_project's sources of `kind`, names prefixed; returns the vertices to connect."""
    if kind == "drums":
        p.assets[pre + "kick"] = W.Asset(W.kick_int16(12, 15000, sr), sr=sr)
        p.assets[pre + "snare"] = W.Asset(W.snare_int16(5, 9000), sr=sr)
        p.load_sample(pre + "kick", pre + "kick", "")
        p.load_sample(pre + "snare", pre + "snare", "")
        n = max(1, int(seconds / 0.125))
        p.event_files[pre + "k"] = np.array([(0.25 * i + 0.002, 36.0, 1.0 - 0.1 * (i % 4)) for i in range((n + 1) // 2)], np.float32)
        p.event_files[pre + "s"] = np.array([(0.125 * i + 0.06, 38.0, 0.2 + 0.15 * (i % 5)) for i in range(n)], np.float32)
        p.load_midi_floww(pre + "k", pre + "k")
        p.load_midi_floww(pre + "s", pre + "s")
        p.add_sample_multi(pre + "kick", 0.9, 0.0, pre + "kick", pre + "k", -1)
        p.add_sample_multi(pre + "snare", 0.6, 25.0, pre + "snare", pre + "s", -1)
        return [pre + "kick", pre + "snare"]
    if kind == "noise":
        p.assets[pre + "n"] = W.Asset(W.noise_int16(31, 20011), sr=sr)
        p.assets[pre + "m"] = W.Asset(W.noise_int16(32, 7001), sr=sr)
        p.load_sample(pre + "n", pre + "n", "")
        p.load_sample(pre + "m", pre + "m", "normalize-seperate")
        p.add_sampleloop(pre + "n", 0.5, 0.0, pre + "n")
        p.add_sampleloop(pre + "m", 0.02, -40.0, pre + "m")
        return [pre + "n", pre + "m"]
    p.assets[pre + "b"] = W.Asset(W.noise_int16(77, int(0.12 * sr)), sr=sr)
    p.assets[pre + "t"] = W.Asset(W.tone_int16(78, int(0.05 * sr)), sr=sr)
    p.load_sample(pre + "b", pre + "b", "")
    p.load_sample(pre + "t", pre + "t", "")
    p.event_files[pre + "b"] = np.array([(0.21, 60.0, 0.9)], np.float32)
    p.event_files[pre + "t"] = np.array([(0.23, 60.0, 0.5)], np.float32)
    p.load_midi_floww(pre + "b", pre + "b")
    p.load_midi_floww(pre + "t", pre + "t")
    p.add_sample_multi(pre + "b", 1.0, 0.0, pre + "b", pre + "b", -1)
    p.add_sample_multi(pre + "t", 0.7, -20.0, pre + "t", pre + "t", -1)
    return [pre + "b", pre + "t"]


def base_project(carrier, key, sr=48000, bl=1024, seconds=0.5):
    """Sources -> Sum `bus` (the carrier) and Sum `kbus` (the key): the vertices in front of the vocoder vertices under test."""
    p = W.ProjectScript(sr, bl)
    p.set_length(seconds)
    p.set_render_samplerate(sr)
    cs, ks = _sources(p, carrier, "c_", sr, seconds), _sources(p, key, "k_", sr, seconds)
    p.add_sum("bus", 1.0, 0.0)
    p.add_sum("kbus", 1.0, 0.0)
    for s in cs:
        p.connect(s, "bus")
    for s in ks:
        p.connect(s, "kbus")
    p.set_output("bus")
    return p


def add_vocoder(p, name, src, key, case, wet=1.0, gain=1.0, angle=0.0):
    p.add_vocoder(name, gain, angle, wet, *case)
    p.connect(src, name)
    if key is not None:
        p.connect_key(key, name)


def random_vocoder_params(rng):
    lo, hi = [(40.0, 21600.0), (200.0, 4000.0), (1000.0, 1001.0)][int(rng.integers(0, 3))]   # (the driver opens every project at 48 kHz)
    return (float(rng.choice([1.0, 1.0, 0.5, 0.0])),                     # wet
            int(rng.choice(BANDS)), lo, hi,
            float(rng.choice(QS)), float(rng.choice(RESPONSES)), float(rng.choice([-24.0, 0.0, 12.0, 48.0])))


def _random_keys(rng, order, nm):
    """Up to two keys from anywhere in the project."""
    names = sorted({a[0] for fn, a in order if fn.startswith("add_")})
    return [(str(rng.choice(names)), nm) for _ in range(int(rng.integers(0, 3)))]


def random_vocoder_project(seed, allow_sinf=True):
    return fx_rig.splice_project(seed, allow_sinf, rng_offset=1_010_000, prefix="vo", add_call="add_vocoder",
                                 draw=lambda rng, p: random_vocoder_params(rng), as_output=False, draw_keys=_random_keys)


def write_projects(args):
    """(base dir, seeds) -> the project dirs written: project.lua + assets, meta.txt (the block length)."""
    return fx_rig.write_projects(random_vocoder_project, args)
