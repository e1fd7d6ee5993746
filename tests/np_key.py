"""A compressor or gate vertex with a key input (TEST INFRASTRUCTURE): the twin of include/termdaw_amd.h's td_graph_connect_key.
It composes the twins of the two vertices and restates none of their steps: the level is read from the key frames k, everything
behind it acts on the summed input x.

    gate(x, k, consts, ...)        np_gate.classes(k) -> np_gate.serial -> np_gate.gain_stage(x, env)
    compressor(x, k, sr, ...)      np_compressor.wanted_reduction(k) -> np_compressor.detector -> steps 5 and 6 on x
    key_sum(parts)                 the key frames of several key sources: f32, in connect_key order, from 0.0 (sum_inputs)

x, k: (frames, 2) float32, rendered by the engine itself at the vertices in front.  With k = x both are the unkeyed twins bit for
bit (tests/test_key_host.py).  A dry vertex (wet < 0.0001f) ignores k."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import np_compressor as NC  # noqa: E402
import np_gate as NG  # noqa: E402
from np_twin import pan_gain  # noqa: E402


def key_sum(parts):
    acc = np.zeros_like(np.asarray(parts[0], np.float32))
    for part in parts:
        acc = (acc + np.asarray(part, np.float32)).astype(np.float32)
    return acc


def _dry(wet):
    return np.float32(min(max(float(np.float32(wet)), 0.0), 1.0)) < np.float32(0.0001)


def gate_env(k, consts, state=None):
    """(t, env, end state) from the key frames."""
    return NG.serial(NG.classes(k, consts[0], consts[1]), consts, NG.closed(consts[2]) if state is None else state)


def gate(x, k, consts, wet=1.0, gain=1.0, angle=0.0, state=None, processed=False):
    """Returns (out float32 (frames, 2), end state)."""
    x = np.asarray(x, np.float32)
    if _dry(wet) and not processed:
        return NG.process(x, consts, wet=wet, gain=gain, angle=angle, state=state)
    _, env, end = gate_env(k, consts, state)
    return NG.gain_stage(x, env, consts[5], wet, gain, angle, processed), end


def compressor_yl(k, sr, threshold_db, ratio, attack_ms, release_ms, knee_db, state=(0.0, 0.0)):
    """(yL[n], end state) from the key frames."""
    aR, aA = NC.coefficients(sr, attack_ms, release_ms)
    return NC.detector(NC.wanted_reduction(k, threshold_db, ratio, knee_db), aR, aA, state)


def compressor(x, k, sr, threshold_db, ratio, attack_ms, release_ms, knee_db, makeup_db, wet=1.0, gain=1.0, angle=0.0, state=(0.0, 0.0),
               processed=False):
    """Returns (out float32 (frames, 2), end state)."""
    x = np.asarray(x, np.float32)
    if _dry(wet) and not processed:
        return NC.compress(x, sr, threshold_db, ratio, attack_ms, release_ms, knee_db, makeup_db, wet=wet, gain=gain, angle=angle, state=state)
    yL, end = compressor_yl(k, sr, threshold_db, ratio, attack_ms, release_ms, knee_db, state)
    # steps 5 and 6, as np_compressor.compress has them behind its detector
    G = np.power(10.0, (float(np.float32(makeup_db)) - yL) / 20.0)
    w = np.float32(min(max(float(np.float32(wet)), 0.0), 1.0))
    with np.errstate(invalid="ignore", over="ignore"):
        p = (x.astype(np.float64) * G[:, None]).astype(np.float32)
        if processed:
            return p, end
        out = x + w * (p - x)
        l, r = pan_gain(out[:, 0], out[:, 1], gain, angle)
    return np.stack([l, r], axis=1).astype(np.float32), end
