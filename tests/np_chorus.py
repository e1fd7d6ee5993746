"""The chorus vertex' float64 twin (TEST INFRASTRUCTURE): the definition in include/termdaw_amd.h at td_graph_add_chorus restated
serially in numpy.

* params: D0, A, f, H, s, Hch from the formulas.
* lfo: the triangle, and the sine through its odd Taylor polynomial to u^9 in Horner form -- add and multiply only, so numpy and
  the device round alike.
* process / chorus: the vertex.  Every step is an elementwise numpy operation over the frames in the definition's order (numpy
  contracts nothing into an FMA), and the voices are added one by one from 0.0 -- nothing is re-associated, which is what lets the
  device tests ask for equal bits.
* The line is the last H raw input frames, oldest first; None is the silent line (a zero contributes nothing).  t0 is the
  absolute frame time of x[0]: the LFO depends on it, the line does not."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from np_twin import pan_gain  # noqa: E402

SHAPES = ("sine", "triangle")
HCH = 2.307
TILES = (256, 512, 1024)   # the candidate output frames per workgroup; the engine's default is TILE
TILE = 256
INLINE = 4096              # chunks up to here take one launch (kSatInlineFrames)
C1, C3, C5, C7, C9 = 1.5707963267948966, -0.6459640975062463, 0.07969262624616705, -0.004681754135318688, 0.00016044118478735983
SIXTH = 0.16666666666666666


def shape_index(shape):
    return SHAPES.index(shape) if isinstance(shape, str) else int(shape)


def params(sr, voices, delay_ms, depth_ms, rate_hz, stereo, shape):
    """(D0, A, f, H, s, Hch) in float64 from the float32 parameters, widened."""
    dl, dp, rt = (float(np.float32(v)) for v in (delay_ms, depth_ms, rate_hz))
    D0 = dl * float(sr) / 1000.0
    A = dp * float(sr) / 1000.0
    f = rt / float(sr)
    H = int(np.ceil((np.floor(D0 + A) + 3.0) / 64.0)) * 64
    s = 2.0 * np.pi * A * f if shape_index(shape) == 0 else 4.0 * A * f
    return D0, A, f, H, s, HCH


def lfo(shape, th):
    """th in [0, 1) -> [-1, 1] (float64 arrays)."""
    th = np.asarray(th, np.float64)
    if shape_index(shape) == 1:
        return 1.0 - 4.0 * np.abs(th - 0.5)
    u = np.where(th < 0.25, 4.0 * th, np.where(th < 0.75, 2.0 - 4.0 * th, 4.0 * th - 4.0))
    u2 = u * u
    p = np.full_like(u, C9)
    p = p * u2 + C7
    p = p * u2 + C5
    p = p * u2 + C3
    p = p * u2 + C1
    return u * p


def _clean(x):
    return np.where(np.isfinite(x), x, np.float32(0.0)).astype(np.float64)


def process(x, sr, voices, delay_ms, depth_ms, rate_hz, stereo, shape, line=None, t0=0, consts=None):
    """(p float32 (frames, 2), line): the processed signal and the new line.  consts: (D0, A, f, H) as the engine reports them
    (else the formulas')."""
    x = np.asarray(x, np.float32).reshape(-1, 2)
    n = len(x)
    D0, A, f, H = consts if consts is not None else params(sr, voices, delay_ms, depth_ms, rate_hz, stereo, shape)[:4]
    H = int(H)
    V = int(voices)
    iv = 1.0 / float(V)
    st = float(np.float32(stereo))
    old = np.zeros((H, 2), np.float32) if line is None else np.asarray(line, np.float32)
    assert old.shape == (H, 2)
    X = np.concatenate([old, x])        # index = frame + H
    xs = _clean(X)
    nn = (np.arange(n, dtype=np.uint64) + np.uint64(t0)).astype(np.float64)
    nf = nn * f
    at = np.arange(n, dtype=np.int64) + H
    S = np.zeros((n, 2))
    for v in range(V):
        phi = float(v) * iv
        for c in range(2):
            th = nf + (phi + st if c else phi)
            th = th - np.floor(th)
            d = D0 + A * lfo(shape, th)
            fi = np.floor(d)
            mu = d - fi
            m = at - fi.astype(np.int64)
            assert (fi >= 1).all() and (fi + 2 <= H).all()   # (the polynomial's overshoot can carry fi to floor(D0 + A) + 1)
            a, b, e = mu - 1.0, mu - 2.0, mu + 1.0
            w0 = ((mu * a) * b) * -SIXTH
            w1 = ((e * a) * b) * 0.5
            w2 = ((e * mu) * b) * -0.5
            w3 = ((e * mu) * a) * SIXTH
            y = np.zeros(n)
            y = y + w0 * xs[m + 1, c]
            y = y + w1 * xs[m, c]
            y = y + w2 * xs[m - 1, c]
            y = y + w3 * xs[m - 2, c]
            S[:, c] = S[:, c] + y
    return (iv * S).astype(np.float32), X[len(X) - H:].copy()


def chorus(x, sr, voices, delay_ms, depth_ms, rate_hz, stereo, shape, wet=1.0, gain=1.0, angle=0.0, line=None, t0=0, consts=None):
    """The vertex: (out float32 (frames, 2), line)."""
    x = np.asarray(x, np.float32).reshape(-1, 2)
    wet = np.float32(min(max(float(np.float32(wet)), 0.0), 1.0))
    if wet < np.float32(0.0001):   # (the engine's test, in f32: 0.0001f itself is processed)
        l, r = pan_gain(x[:, 0].copy(), x[:, 1].copy(), gain, angle)
        return np.stack([l, r], axis=1).astype(np.float32), line
    p, end = process(x, sr, voices, delay_ms, depth_ms, rate_hz, stereo, shape, line, t0, consts)
    with np.errstate(invalid="ignore", over="ignore"):
        out = x + wet * (p - x)   # float32 throughout: the reference's lerp (adsr.rs:42)
        l, r = pan_gain(out[:, 0], out[:, 1], gain, angle)
    return np.stack([l, r], axis=1).astype(np.float32), end
