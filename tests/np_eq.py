"""The parametric EQ vertex, serially (TEST INFRASTRUCTURE): a float64 restatement of the definition in include/termdaw_amd.h
(td_graph_add_eq), with a plain loop for the recurrence.  No reference counterpart exists for this vertex; the header's text is
the definition and this file is its twin.

    cookbook(kind, sr, freq_hz, q, gain_db) -> (b0, b1, b2, a1, a2)      the cookbook formulas, float64
    biquad(x, c, state) -> (y float64, end state)                        the recurrence alone; c may hold K filters at once
    eq(x, c, wet=, gain=, angle=, state=) -> (out float32, end state)    the whole vertex
    blocked(x, c, state) -> y float64                                    the device's tiled scan, emulated (derives the GPU
                                                                         test's bound E; nothing else uses it)

x: (frames, 2) float32, the vertex' summed input.  c: the five normalised coefficients -- the tests take them from
td_eq_coefficients, so that a last-bit difference between the host's libm and numpy's cannot show up as a filter difference.
The recurrence runs in float64 (Python floats / numpy float64: no fused multiply-add), the lerp, pan and gain in float32."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from np_twin import pan_gain  # noqa: E402  (sample.rs:97-114 in float32, as the engine's make_pg)

KINDS = ("lowpass", "highpass", "bandpass", "notch", "peak", "lowshelf", "highshelf")
HAS_GAIN = ("peak", "lowshelf", "highshelf")
RUN, LANES = 8, 256
TILE = RUN * LANES


def cookbook(kind, sr, freq_hz, q, gain_db):
    """Robert Bristow-Johnson's Audio EQ Cookbook, float64 from the float32 parameters; 1 - cos w0 as 2 sin^2(w0 / 2)."""
    kind = KINDS[kind] if not isinstance(kind, str) else kind
    f, q, g = float(np.float32(freq_hz)), float(np.float32(q)), float(np.float32(gain_db))
    w0 = 2.0 * math.pi * f / float(sr)
    cw, sw, sh = math.cos(w0), math.sin(w0), math.sin(0.5 * w0)
    omc = 2.0 * sh * sh
    opc = 1.0 + cw
    alpha = sw / (2.0 * q)
    A = math.pow(10.0, g / 40.0) if kind in HAS_GAIN else 1.0
    if kind == "lowpass":
        b, a = (omc / 2.0, omc, omc / 2.0), (1.0 + alpha, -2.0 * cw, 1.0 - alpha)
    elif kind == "highpass":
        b, a = (opc / 2.0, -opc, opc / 2.0), (1.0 + alpha, -2.0 * cw, 1.0 - alpha)
    elif kind == "bandpass":
        b, a = (alpha, 0.0, -alpha), (1.0 + alpha, -2.0 * cw, 1.0 - alpha)
    elif kind == "notch":
        b, a = (1.0, -2.0 * cw, 1.0), (1.0 + alpha, -2.0 * cw, 1.0 - alpha)
    elif kind == "peak":
        b, a = (1.0 + alpha * A, -2.0 * cw, 1.0 - alpha * A), (1.0 + alpha / A, -2.0 * cw, 1.0 - alpha / A)
    else:
        s, p, m = 2.0 * math.sqrt(A) * alpha, A + 1.0, A - 1.0
        if kind == "lowshelf":
            b = (A * ((p - m * cw) + s), 2.0 * A * (m - p * cw), A * ((p - m * cw) - s))
            a = ((p + m * cw) + s, -2.0 * (m + p * cw), (p + m * cw) - s)
        else:
            b = (A * ((p + m * cw) + s), -2.0 * A * (m + p * cw), A * ((p + m * cw) - s))
            a = ((p - m * cw) + s, 2.0 * (m - p * cw), (p - m * cw) - s)
    return np.array([b[0] / a[0], b[1] / a[0], b[2] / a[0], a[1] / a[0], a[2] / a[0]])


def response(c, w):
    """H(e^jw) of normalised coefficients at the angular frequencies w (complex128)."""
    z1 = np.exp(-1j * np.asarray(w, np.float64))
    return (c[0] + c[1] * z1 + c[2] * z1 * z1) / (1.0 + c[3] * z1 + c[4] * z1 * z1)


def _clean(x):
    x = np.asarray(x, np.float32)
    return np.where(np.isfinite(x), x, np.float32(0.0)).astype(np.float64)


def biquad(x, c, state=None):
    """y[n] = b0 x[n] + s1;  s1 = (b1 x[n] - a1 y[n]) + s2;  s2 = b2 x[n] - a2 y[n], float64, per channel; non-finite samples
    enter as 0.  c of shape (5,): x (frames, C) -> y (frames, C), state (2, C).  c of shape (K, 5): y (K, frames, C), the K
    filters stepped together, state (K, 2, C)."""
    c = np.asarray(c, np.float64)
    xs = _clean(x)
    n, C = xs.shape
    if c.ndim == 1:
        b0, b1, b2, a1, a2 = (float(v) for v in c)
        y = np.empty((n, C))
        end = np.zeros((2, C))
        for ch in range(C):
            s1, s2 = (0.0, 0.0) if state is None else (float(state[0][ch]), float(state[1][ch]))
            out = [0.0] * n
            col = xs[:, ch].tolist()
            for i in range(n):
                v = col[i]
                w = b0 * v + s1
                s1 = (b1 * v - a1 * w) + s2
                s2 = b2 * v - a2 * w
                out[i] = w
            y[:, ch] = out
            end[:, ch] = (s1, s2)
        return y, end
    K = c.shape[0]
    b0, b1, b2, a1, a2 = (c[:, j][:, None] for j in range(5))
    s1 = np.zeros((K, C)) if state is None else np.array(state[:, 0, :], np.float64)
    s2 = np.zeros((K, C)) if state is None else np.array(state[:, 1, :], np.float64)
    y = np.empty((K, n, C))
    for i in range(n):
        v = xs[i][None, :]
        w = b0 * v + s1
        s1 = (b1 * v - a1 * w) + s2
        s2 = b2 * v - a2 * w
        y[:, i, :] = w
    return y, np.stack([s1, s2], axis=1)


def eq(x, c, wet=1.0, gain=1.0, angle=0.0, state=None, processed=False):
    """The vertex: (out float32 (frames, 2), end state (2, 2)); processed=True: p, the filtered signal rounded to float32,
    instead of the mix, pan and gain."""
    x = np.asarray(x, np.float32)
    wet = np.float32(min(max(float(np.float32(wet)), 0.0), 1.0))
    if wet < np.float32(0.0001) and not processed:   # (the engine's test, in f32: 0.0001f itself is processed)
        l, r = pan_gain(x[:, 0].copy(), x[:, 1].copy(), gain, angle)
        return np.stack([l, r], axis=1).astype(np.float32), (np.zeros((2, 2)) if state is None else np.array(state, np.float64))
    y, end = biquad(x, c, state)
    with np.errstate(invalid="ignore", over="ignore"):
        p = np.where(np.isfinite(x), y.astype(np.float32), x)   # a non-finite input frame's p is the input sample itself
        if processed:
            return p, end
        out = x + wet * (p - x)   # float32 throughout: the reference's lerp (adsr.rs:42)
        l, r = pan_gain(out[:, 0], out[:, 1], gain, angle)
    return np.stack([l, r], axis=1).astype(np.float32), end


# ---- the device's tiled scan, emulated ----
def _ld_matmul(x, y):
    return np.stack([x[..., 0] * y[..., 0] + x[..., 1] * y[..., 2], x[..., 0] * y[..., 1] + x[..., 1] * y[..., 3],
                     x[..., 2] * y[..., 0] + x[..., 3] * y[..., 2], x[..., 2] * y[..., 1] + x[..., 3] * y[..., 3]], axis=-1)


def _ld_power(x, e):
    r = np.zeros_like(x)
    r[..., 0] = 1
    r[..., 3] = 1
    while e:
        if e & 1:
            r = _ld_matmul(r, x)
        if e > 1:
            x = _ld_matmul(x, x)
        e >>= 1
    return r


def powers(a1, a2, chunk, dtype=np.longdouble):
    """The descriptor's matrices (row-major 2x2, A = [[-a1, 1], [-a2, 0]]): pw[k] = A^(8 2^k), a_tile = A^2048,
    pwc[k] = A^(2048 chunk 2^k); squared in `dtype` (long double, as the engine does; float64 to see why), rounded once to float64.
    a1, a2 of shape (K,): results (K, 8, 4), (K, 4), (K, 8, 4)."""
    a1, a2 = np.atleast_1d(np.asarray(a1, np.float64)), np.atleast_1d(np.asarray(a2, np.float64))
    A = np.zeros(a1.shape + (4,), dtype)
    A[..., 0], A[..., 1], A[..., 2] = -a1.astype(dtype), 1, -a2.astype(dtype)
    p = _ld_power(A, RUN)
    pw = []
    for _ in range(8):
        pw.append(p.astype(np.float64))
        p = _ld_matmul(p, p)
    a_tile = p.astype(np.float64)
    p = _ld_power(p, chunk)
    pwc = []
    for _ in range(8):
        pwc.append(p.astype(np.float64))
        p = _ld_matmul(p, p)
    return np.stack(pw, axis=1), a_tile, np.stack(pwc, axis=1)


def _mac(u, P, o):
    """u + P o on (.., 2, C) states with P (K, 4) broadcast over the middle axes."""
    P = P.reshape((P.shape[0],) + (1,) * (u.ndim - 3) + (4,))
    return np.stack([u[..., 0, :] + (P[..., 0, None] * o[..., 0, :] + P[..., 1, None] * o[..., 1, :]),
                     u[..., 1, :] + (P[..., 2, None] * o[..., 0, :] + P[..., 3, None] * o[..., 1, :])], axis=-2)


def _lane_scan(u, pw):
    """Hillis-Steele over axis -3 (256 lanes) of u (K, .., 256, 2, C) with pw (K, 8, 4): the inclusive join."""
    for k in range(8):
        off = 1 << k
        v = u.copy()
        v[..., off:, :, :] = _mac(u[..., off:, :, :], pw[:, k], u[..., :-off, :, :])
        u = v
    return u


def blocked(x, c, state=None, power_dtype=np.longdouble):
    """The scan as k_eq_local / k_eq_carry / k_eq_apply run it, float64 with numpy's operation order: every lane's
    8 frames from zero in the form z <- A z + c x, the lanes joined by Hillis-Steele, the tiles by k_eq_carry's chunked scan, then
    every lane serially from its entry state in the definition's form.  c (5,) or (K, 5); returns y float64 (K, frames, C)."""
    c = np.atleast_2d(np.asarray(c, np.float64))
    K = c.shape[0]
    xs = _clean(x)
    n, C = xs.shape
    T = (n + TILE - 1) // TILE
    chunk = (T + LANES - 1) // LANES
    xp = np.zeros((T * TILE, C))
    xp[:n] = xs
    xl = xp.reshape(1, T, LANES, RUN, C)
    b0, b1, b2, a1, a2 = (c[:, j].reshape(K, 1, 1, 1) for j in range(5))
    c0, c1 = b1 - a1 * b0, b2 - a2 * b0
    pw, a_tile, pwc = powers(c[:, 3], c[:, 4], chunk, power_dtype)
    entry0 = np.zeros((K, 2, C)) if state is None else np.broadcast_to(np.asarray(state, np.float64), (K, 2, C)).copy()

    def zrun(s1, s2):
        for j in range(RUN):
            v = xl[:, :, :, j, :]
            s1, s2 = (c0 * v - a1 * s1) + s2, c1 * v - a2 * s1
        return np.stack([s1, s2], axis=-2)   # (K, T, LANES, 2, C)
    z = np.zeros((K, T, LANES, C))
    total = _lane_scan(zrun(z, z), pw)[:, :, -1]   # (K, T, 2, C): k_eq_local's tile words
    # k_eq_carry: lane t folds tiles [t chunk, (t + 1) chunk), Hillis-Steele with pwc, a second walk writes the entries
    pad = np.zeros((K, LANES * chunk, 2, C))
    pad[:, :T] = total
    agg = pad.reshape(K, LANES, chunk, 2, C)
    u = np.zeros((K, LANES, 2, C))
    u[:, 0] = entry0
    for r in range(chunk):
        u = _mac(agg[:, :, r], a_tile, u)
    inc = _lane_scan(u, pwc)
    cur = np.concatenate([entry0[:, None], inc[:, :-1]], axis=1)
    entry = np.empty((K, LANES, chunk, 2, C))
    for r in range(chunk):
        entry[:, :, r] = cur
        cur = _mac(agg[:, :, r], a_tile, cur)
    entry = entry.reshape(K, LANES * chunk, 2, C)[:, :T]
    # k_eq_apply: lane 0 from the tile's entry, the others from zero; join; then the definition's form from each lane's entry
    s1 = np.zeros((K, T, LANES, C))
    s2 = np.zeros((K, T, LANES, C))
    s1[:, :, 0], s2[:, :, 0] = entry[:, :, 0], entry[:, :, 1]
    inc = _lane_scan(zrun(s1, s2), pw)
    zin = np.concatenate([entry[:, :, None], inc[:, :, :-1]], axis=2)
    s1, s2 = zin[..., 0, :], zin[..., 1, :]
    y = np.empty((K, T, LANES, RUN, C))
    for j in range(RUN):
        v = xl[:, :, :, j, :]
        w = b0 * v + s1
        s1 = (b1 * v - a1 * w) + s2
        s2 = b2 * v - a2 * w
        y[:, :, :, j, :] = w
    return y.reshape(K, T * TILE, C)[:, :n]
