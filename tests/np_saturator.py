"""The saturator vertex' float64 twin (TEST INFRASTRUCTURE): the definition in include/termdaw_amd.h at td_graph_add_saturator
restated serially in numpy.

* taps_formula: the 4-term Blackman-Harris windowed sinc.
* params: g_in, g_out, f(bias), latency, Lf, Hsat from the formulas (Hup / Hdown on a dense grid).
* process / saturator: the vertex.  Every output is a sum accumulated from 0.0 in ascending index; the loops below run over the
  TAPS and add one product to every output's accumulator per step, so each output sees the definition's operations in the
  definition's order -- nothing is re-associated, which is what lets the device tests ask for equal bits.
* The line is the last 128 raw input frames, oldest first; None is the silent line (a zero contributes nothing)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from np_twin import pan_gain  # noqa: E402

Z = 32
LATENCY = 2 * Z
LINE = 4 * Z
KINDS = ("hard", "cubic", "soft")
TILES = (128, 256, 384)   # the candidate output frames per workgroup; the engine's default is TILE
TILE = 256


def taps_formula(R):
    L = 2 * Z * R + 1
    k = np.arange(L, dtype=np.float64)
    t = k - Z * R
    fc = (0.5 - 2.0 / Z) / R
    with np.errstate(invalid="ignore", divide="ignore"):
        s = np.where(t == 0.0, 2.0 * fc, np.sin(2.0 * np.pi * fc * t) / (np.pi * t))
    a = 2.0 * np.pi * k / (L - 1)
    w = 0.35875 - 0.48829 * np.cos(a) + 0.14128 * np.cos(2.0 * a) - 0.01168 * np.cos(3.0 * a)
    sw = s * w
    total = 0.0
    for v in sw:   # (ascending, like the engine)
        total += float(v)
    return sw / total


def shape(kind, u):
    kind = KINDS.index(kind) if isinstance(kind, str) else int(kind)
    u = np.asarray(u, np.float64)
    if kind == 0:
        return np.minimum(np.maximum(u, -1.0), 1.0)
    if kind == 1:
        return np.where(np.abs(u) < 1.0, 1.5 * u - ((0.5 * u) * u) * u, np.copysign(1.0, u))
    return u / (1.0 + np.abs(u))


def lipschitz(kind):
    kind = KINDS.index(kind) if isinstance(kind, str) else int(kind)
    return 1.5 if kind == 1 else 1.0


def branch_gain(h, R, scale, n_grid=2048):
    """sqrt(sum_r max_w |scale h[r::R] (e^jw)|^2) on a grid of n_grid + 1 points over [0, pi]."""
    w = np.pi * np.arange(n_grid + 1, dtype=np.longdouble) / n_grid
    total = np.longdouble(0)
    for r in range(R):
        b = scale * np.asarray(h[r::R], np.longdouble)
        j = np.arange(len(b), dtype=np.longdouble)
        re = (b[None, :] * np.cos(w[:, None] * j[None, :])).sum(axis=1)
        im = (b[None, :] * np.sin(w[:, None] * j[None, :])).sum(axis=1)
        total += (re * re + im * im).max()
    return float(np.sqrt(total))


def params(kind, R, drive_db, bias, out_db, h=None):
    """(g_in, g_out, f(bias), latency, Lf, Hsat) in float64 from the float32 parameters, widened."""
    d, b, o = (float(np.float32(v)) for v in (drive_db, bias, out_db))
    g_in, g_out = 10.0 ** (d / 20.0), 10.0 ** (o / 20.0)
    fb = float(shape(kind, b))
    lf = lipschitz(kind)
    if R == 1:
        return g_in, g_out, fb, 0, lf, g_out * lf * g_in
    h = taps_formula(R) if h is None else h
    return g_in, g_out, fb, LATENCY, lf, g_out * branch_gain(h, R, 1.0) * lf * g_in * branch_gain(h, R, float(R))


def _clean(x):
    return np.where(np.isfinite(x), x, np.float32(0.0)).astype(np.float64)


def process(x, kind, R, g_in, bias, fb, g_out, h=None, line=None):
    """(p float32 (frames, 2), xd float32 (frames, 2), line): the processed signal, the dry leg it is mixed with, the new line."""
    x = np.asarray(x, np.float32).reshape(-1, 2)
    n = len(x)
    bias = float(np.float32(bias))
    if R == 1:
        with np.errstate(invalid="ignore", over="ignore"):
            p = (g_out * (shape(kind, g_in * _clean(x) + bias) - fb)).astype(np.float32)
        return np.where(np.isfinite(x), p, x), x, None
    old = np.zeros((LINE, 2), np.float32) if line is None else np.asarray(line, np.float32)
    assert old.shape == (LINE, 2)
    X = np.concatenate([old, x])        # index = frame + 128
    xs = _clean(X)
    nw = n + LATENCY                     # w for frames -64 .. n - 1: index = frame + 64
    w = np.zeros((R, nw, 2))
    for r in range(R):
        acc = np.zeros((nw, 2))
        for j in range(2 * Z + (1 if r == 0 else 0)):
            acc = acc + (R * h[r + j * R]) * xs[LATENCY - j:LATENCY - j + nw]
        w[r] = shape(kind, g_in * acc + bias) - fb
    y = np.zeros((n, 2))
    y = y + h[0] * w[0, LATENCY:LATENCY + n]
    for g in range(1, 2 * Z + 1):
        for s in range(1, R):
            y = y + h[(g - 1) * R + s] * w[R - s, LATENCY - g:LATENCY - g + n]
        y = y + h[g * R] * w[0, LATENCY - g:LATENCY - g + n]
    return (g_out * y).astype(np.float32), X[LATENCY:LATENCY + n], X[len(X) - LINE:].copy()


def saturator(x, kind, R, drive_db, bias, out_db, wet=1.0, gain=1.0, angle=0.0, h=None, line=None, consts=None):
    """The vertex: (out float32 (frames, 2), line).  consts: (g_in, g_out, fb) as the engine reports them (else the formulas')."""
    x = np.asarray(x, np.float32).reshape(-1, 2)
    wet = np.float32(min(max(float(np.float32(wet)), 0.0), 1.0))
    if wet < np.float32(0.0001):   # (the engine's test, in f32: 0.0001f itself is processed)
        l, r = pan_gain(x[:, 0].copy(), x[:, 1].copy(), gain, angle)
        return np.stack([l, r], axis=1).astype(np.float32), line
    if h is None and R > 1:
        h = taps_formula(R)
    g_in, g_out, fb = consts if consts is not None else params(kind, R, drive_db, bias, out_db, h)[:3]
    p, xd, end = process(x, kind, R, g_in, bias, fb, g_out, h, line)
    with np.errstate(invalid="ignore", over="ignore"):
        out = xd + wet * (p - xd)   # float32 throughout: the reference's lerp (adsr.rs:42)
        l, r = pan_gain(out[:, 0], out[:, 1], gain, angle)
    return np.stack([l, r], axis=1).astype(np.float32), end
