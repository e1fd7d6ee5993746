"""The feedback delay vertex' float64 twin (TEST INFRASTRUCTURE): the definition in include/termdaw_amd.h at td_graph_add_delay
restated serially in numpy, and an emulation of the device's tiled scan that the bound of
tests/test_gpu_delay.py is derived from.

* params: D, gs, gc, Hecho from the formulas.
* delay: the vertex.  u[n] = x[n] + G u[n - D] depends on the frame D earlier only, so the serial definition is evaluated D frames
  at a time -- the same float64 operations in the same order for every frame, nothing re-associated.
* blocked: the three launches in numpy -- every (tile, lane) from the zero state, the carry over tiles with matrix powers squared
  in long double and rounded once (seg threads per lane folding `chunk` tiles, Hillis-Steele over them), then every tile from
  its entry state in the definition's order."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from np_twin import pan_gain  # noqa: E402

TILES = (8, 16, 32, 64)   # the candidate steps per tile; the engine's default is TILE
TILE = 16
CARRY_FOLD = 16           # tiles a carry thread folds serially before a lane gets more threads (csrc/delay_math.h)


def params(sr, time_ms, feedback, cross):
    """(D, gs, gc, Hecho) in float64 from the float32 parameters, widened."""
    t, f, c = (float(np.float32(v)) for v in (time_ms, feedback, cross))
    D = max(1, int(np.floor(t * float(sr) / 1000.0 + 0.5)))   # llround: halves away from zero (positive here)
    return D, f * (1.0 - c), f * c, 1.0 / (1.0 - f)


def _clean(x):
    """A non-finite input sample enters the line as 0."""
    return np.where(np.isfinite(x), x, np.float32(0.0)).astype(np.float64)


def echo(x, D, gs, gc, line=None):
    """(x + w as float64 (frames, 2), line): w = u[n - D].  `line`: the last D values of u in time order (oldest first), zeros when
    None; returned likewise."""
    x = np.asarray(x, np.float32)
    n = len(x)
    xin = _clean(x)
    hist = np.zeros((D, 2)) if line is None else np.array(line, np.float64)
    assert hist.shape == (D, 2)
    u = np.concatenate([hist, np.zeros((n, 2))])
    for a in range(0, n, D):
        b = min(a + D, n)
        w = u[a:a + (b - a)]                       # frames a - D .. b - D of u (offset D in the array)
        xs = xin[a:b]
        nl = xs[:, 0] + (gs * w[:, 0] + gc * w[:, 1])
        nr = xs[:, 1] + (gs * w[:, 1] + gc * w[:, 0])
        u[D + a:D + b, 0] = nl
        u[D + a:D + b, 1] = nr
    return xin + u[:n], u[n:].copy()


def delay(x, D, gs, gc, wet=1.0, gain=1.0, angle=0.0, line=None, processed=False):
    """The vertex: (out float32 (frames, 2), line); processed=True: p, the echoed signal rounded to float32, instead of the mix,
    pan and gain."""
    x = np.asarray(x, np.float32)
    wet = np.float32(min(max(float(np.float32(wet)), 0.0), 1.0))
    if wet < np.float32(0.0001) and not processed:   # (the engine's test, in f32: 0.0001f itself is processed)
        l, r = pan_gain(x[:, 0].copy(), x[:, 1].copy(), gain, angle)
        return np.stack([l, r], axis=1).astype(np.float32), (np.zeros((D, 2)) if line is None else np.array(line, np.float64))
    y, end = echo(x, D, gs, gc, line)
    with np.errstate(invalid="ignore", over="ignore"):
        p = np.where(np.isfinite(x), y.astype(np.float32), x)   # a non-finite input frame's p is the input sample itself
        if processed:
            return p, end
        out = x + wet * (p - x)   # float32 throughout: the reference's lerp (adsr.rs:42)
        l, r = pan_gain(out[:, 0], out[:, 1], gain, angle)
    return np.stack([l, r], axis=1).astype(np.float32), end


# ---- the tiled scan ----
def _ld_matmul(x, y):
    return np.array([x[0] * y[0] + x[1] * y[2], x[0] * y[1] + x[1] * y[3], x[2] * y[0] + x[3] * y[2], x[2] * y[1] + x[3] * y[3]], x.dtype)


def _ld_power(x, e):
    r = np.array([1, 0, 0, 1], x.dtype)
    while e:
        if e & 1:
            r = _ld_matmul(r, x)
        e >>= 1
        if e:
            x = _ld_matmul(x, x)
    return r


def tiling(frames, D, T=TILE):
    """(lanes, n_tiles, seg, chunk) as csrc/delay_math.h computes them."""
    lanes = min(D, frames)
    steps = -(-frames // D)
    n_tiles = -(-steps // T)
    seg = 1
    while seg < 256 and seg * CARRY_FOLD < n_tiles:
        seg *= 2
    return lanes, n_tiles, seg, -(-n_tiles // seg)


def powers(gs, gc, T, chunk, dtype=np.longdouble):
    """(G^T, [G^(T chunk 2^k)] k = 0 .. 7), squared in `dtype`, each rounded once to float64."""
    p = _ld_power(np.array([gs, gc, gc, gs], dtype), T)
    g_tile = p.astype(np.float64)
    p = _ld_power(p, chunk)
    pwc = []
    for _ in range(8):
        pwc.append(p.astype(np.float64))
        p = _ld_matmul(p, p)
    return g_tile, np.stack(pwc)


def _step(x, w, gs, gc):
    return np.stack([x[..., 0] + (gs * w[..., 0] + gc * w[..., 1]), x[..., 1] + (gs * w[..., 1] + gc * w[..., 0])], axis=-1)


def _mac(t, P, o):
    """t + P o, in the kernel's order: t[0] + (P0 o0 + P1 o1), t[1] + (P2 o0 + P3 o1)."""
    return np.stack([t[..., 0] + (P[0] * o[..., 0] + P[1] * o[..., 1]), t[..., 1] + (P[2] * o[..., 0] + P[3] * o[..., 1])], axis=-1)


def blocked(x, D, gs, gc, T=TILE, line=None, power_dtype=np.longdouble):
    """x + w as float64 (frames, 2) by the three launches (needs more than one tile: ceil(frames / D) > T)."""
    x = np.asarray(x, np.float32)
    n = len(x)
    lanes, n_tiles, seg, chunk = tiling(n, D, T)
    assert n_tiles > 1 and lanes == D
    g_tile, pwc = powers(gs, gc, T, chunk, power_dtype)
    xin = np.zeros((n_tiles * T * D, 2))
    xin[:n] = _clean(x)
    xin = xin.reshape(n_tiles, T, D, 2)
    # k_delay_local: every (tile, lane) from the zero state
    u = np.zeros((n_tiles, D, 2))
    for i in range(T):
        u = _step(xin[:, i], u, gs, gc)
    agg = u
    # k_delay_carry: per lane, thread s folds tiles [s chunk, (s + 1) chunk), Hillis-Steele over the threads, a second walk
    init = np.zeros((D, 2)) if line is None else np.array(line, np.float64)
    pad = np.zeros((seg * chunk, D, 2))
    pad[:n_tiles] = agg
    pad = pad.reshape(seg, chunk, D, 2)
    live = (np.arange(seg * chunk) < n_tiles).reshape(seg, chunk)
    f = np.zeros((seg, D, 2))
    f[0] = init
    for r in range(chunk):
        f = np.where(live[:, r, None, None], _mac(pad[:, r], g_tile, f), f)
    k = 0
    while (1 << k) < seg:
        off = 1 << k
        g = f.copy()
        g[off:] = _mac(f[off:], pwc[k], f[:-off])
        f = g
        k += 1
    ent = np.concatenate([init[None], f[:-1]])
    carry = np.zeros((seg, chunk, D, 2))
    for r in range(chunk):
        carry[:, r] = ent
        ent = _mac(pad[:, r], g_tile, ent)
    carry = carry.reshape(seg * chunk, D, 2)[:n_tiles]
    # k_delay_apply: every tile from its entry state, in the definition's order
    u = carry
    y = np.zeros((n_tiles, T, D, 2))
    for i in range(T):
        y[:, i] = xin[:, i] + u
        u = _step(xin[:, i], u, gs, gc)
    return y.reshape(-1, 2)[:n]
