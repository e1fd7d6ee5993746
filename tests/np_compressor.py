"""The compressor vertex, serially (TEST INFRASTRUCTURE): a float64 restatement of the definition in include/termdaw_amd.h
(td_graph_add_compressor), steps 1-6, with plain loops for the two recurrences.  No reference counterpart exists for this
vertex; the header's text is the definition and this file is its twin.

    compress(x, sr, threshold_db=..., ..., state=(y1, yL)) -> (out, (y1, yL))

x: (frames, 2) float32, the vertex' summed input.  Every parameter is rounded to float32 first (the C ABI takes floats) and
widened to float64, as the engine does.  Steps 1-5 run in float64, step 6 (the reference's lerp, pan, gain) in float32."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from np_twin import pan_gain  # noqa: E402  (sample.rs:97-114 in float32, as the engine's make_pg)

F32_TINY = float(np.float32(2.0) ** -149)   # the smallest subnormal


def coefficients(sr, attack_ms, release_ms):
    attack_ms, release_ms = float(np.float32(attack_ms)), float(np.float32(release_ms))
    aR = math.exp(-1.0 / (release_ms * float(sr) / 1000.0))
    aA = math.exp(-1.0 / (attack_ms * float(sr) / 1000.0)) if attack_ms > 0.0 else 0.0
    return aR, aA


def wanted_reduction(x, threshold_db, ratio, knee_db):
    """Steps 1 and 2: d[n] in dB, float64, from (frames, 2) float32."""
    T, R, W = (float(np.float32(v)) for v in (threshold_db, ratio, knee_db))
    x = np.asarray(x, np.float32).astype(np.float64)
    s = np.maximum(np.abs(x[:, 0]), np.abs(x[:, 1]))   # (np.maximum hands a NaN on)
    ok = np.isfinite(s) & (s > 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        o = 20.0 * np.log10(np.where(ok, s, 1.0)) - T
    slope = 1.0 - 1.0 / R
    d = np.zeros(len(s))
    if W > 0.0:
        knee = ok & (2.0 * o >= -W) & (2.0 * np.abs(o) <= W)
        t = o + W / 2.0
        d = np.where(knee, slope * (t * t) / (2.0 * W), d)
    above = ok & (2.0 * o > W)
    d = np.where(above, slope * o, d)
    return d


def detector(d, aR, aA, state=(0.0, 0.0)):
    """Steps 3 and 4, serially: (yL[n], end state)."""
    y1, yL = float(state[0]), float(state[1])
    oA = 1.0 - aA
    out = np.empty(len(d))
    dl = d.tolist()
    for n in range(len(dl)):
        v = aR * y1
        dn = dl[n]
        y1 = dn if dn >= v else v
        yL = aA * yL + oA * y1
        out[n] = yL
    return out, (y1, yL)


def compress(x, sr, threshold_db, ratio, attack_ms, release_ms, knee_db, makeup_db, wet=1.0, gain=1.0, angle=0.0, state=(0.0, 0.0),
             processed=False):
    """Returns (out float32 (frames, 2), end state); processed=True: p of step 5 instead of step 6's mix, pan and gain."""
    x = np.asarray(x, np.float32)
    wet = np.float32(min(max(float(np.float32(wet)), 0.0), 1.0))
    if wet < np.float32(0.0001) and not processed:   # (the engine's test, in f32: 0.0001f itself is processed)
        l, r = pan_gain(x[:, 0].copy(), x[:, 1].copy(), gain, angle)
        return np.stack([l, r], axis=1).astype(np.float32), (float(state[0]), float(state[1]))
    aR, aA = coefficients(sr, attack_ms, release_ms)
    d = wanted_reduction(x, threshold_db, ratio, knee_db)
    yL, end = detector(d, aR, aA, state)
    M = float(np.float32(makeup_db))
    G = np.power(10.0, (M - yL) / 20.0)
    with np.errstate(invalid="ignore", over="ignore"):
        p = (x.astype(np.float64) * G[:, None]).astype(np.float32)
        if processed:
            return p, end
        out = x + wet * (p - x)   # float32 throughout: the reference's lerp (adsr.rs:42)
        l, r = pan_gain(out[:, 0], out[:, 1], gain, angle)
    return np.stack([l, r], axis=1).astype(np.float32), end
