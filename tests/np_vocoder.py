"""The vocoder vertex, serially (TEST INFRASTRUCTURE): a float64 restatement of the definition in include/termdaw_amd.h
(td_graph_add_vocoder), with a plain loop for the recurrences.  No reference counterpart exists for this vertex; the header's text
is the definition and this file is its twin.

    spec(params) -> dict                                   what the functions below take, from api.vocoder_params' (rows, a, g)
    modulator(key) -> m float64 (frames,)                  step 1, with the key frame's non-finite rule
    serial(x, key, specs, state) -> (p float64, end)       steps 1 .. 4 before the rounding to float32; specs of ONE band count
                                                           are stepped together: p (S, frames, 2), end (S, B, 7)
    process(x, key, spec, wet=, gain=, angle=, state=)     the whole vertex: (out float32 (frames, 2), end state (B, 7))
    blocked(x, key, spec, state) -> (p float64, end)       the device's tiled scans, emulated: the kernels' tile geometry (2 048
                                                           frames = 256 lanes x 8) and join order (derives the GPU test's bound E;
                                                           nothing else uses it)

x: (frames, 2) float32, the vertex' summed input (the carrier).  key: (frames, 2) float32, the sum of its key sources, or None:
the vertex listens to itself.  The constants come from td_vocoder_params, so that a last-bit difference between the host's libm
and numpy's cannot show up as a filter difference.  The recurrences run in float64 (numpy float64: no fused multiply-add), the
lerp, pan and gain in float32.  The state is the line's: per band (s1l, s2l, s1r, s2r, s1m, s2m, e)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import np_eq as NE  # noqa: E402  (the EQ's matrix powers and lane join: the vocoder's biquad scans are the EQ's, three signals wide)
from np_twin import pan_gain  # noqa: E402

RUN, LANES = NE.RUN, NE.LANES
TILE = RUN * LANES
BLOCK = 4096   # frames whose products serial() keeps before it adds the bands up


def spec(params):
    rows, a, g = params
    rows = np.asarray(rows, np.float64)
    return dict(f=rows[:, 0].copy(), c=rows[:, 1:6].copy(), a=float(a), g=float(g), B=len(rows))


def modulator(key):
    key = np.asarray(key, np.float32)
    ok = np.isfinite(key).all(axis=1)
    with np.errstate(invalid="ignore", over="ignore"):
        m = 0.5 * (key[:, 0].astype(np.float64) + key[:, 1].astype(np.float64))
    return np.where(ok, m, 0.0)


def signals(x, key):
    """(frames, 3) float64: (l, r, m) as they enter the biquads."""
    x = np.asarray(x, np.float32)
    xs = np.where(np.isfinite(x), x, np.float32(0.0)).astype(np.float64)
    return np.concatenate([xs, modulator(x if key is None else key)[:, None]], axis=1)


def _stack(specs):
    specs = [specs] if isinstance(specs, dict) else list(specs)
    B = specs[0]["B"]
    assert all(s["B"] == B for s in specs)
    c = np.concatenate([s["c"] for s in specs])                      # (S B, 5)
    a = np.repeat(np.array([s["a"] for s in specs]), B)              # (S B,)
    g = np.array([s["g"] for s in specs])
    return specs, B, c, a, g


def _band_sum(e, y, S, B, g):
    """g (e_0 c_0 + e_1 c_1 + ..), from 0.0 in band order: e (.., S B), y (.., S B, 2) -> (.., S, 2)."""
    prod = (e[..., None] * y).reshape(e.shape[:-1] + (S, B, 2))
    acc = np.zeros(prod.shape[:-2] + (2,))
    for b in range(B):
        acc = acc + prod[..., b, :]
    return g[:, None] * acc


def serial(x, key, specs, state=None):
    single = isinstance(specs, dict)
    specs, B, c, a, g = _stack(specs)
    S, K = len(specs), len(specs) * B
    v3 = signals(x, key)
    n = len(v3)
    b0, b1, b2, a1, a2 = (c[:, j][:, None] for j in range(5))
    oa = 1.0 - a
    st = np.zeros((S, B, 7)) if state is None else np.broadcast_to(np.asarray(state, np.float64), (S, B, 7)).copy()
    st = st.reshape(K, 7)
    s1, s2, e = st[:, 0:6:2].copy(), st[:, 1:6:2].copy(), st[:, 6].copy()
    p = np.empty((S, n, 2))
    for lo in range(0, n, BLOCK):
        hi = min(n, lo + BLOCK)
        Y, E = np.empty((hi - lo, K, 2)), np.empty((hi - lo, K))
        for i in range(lo, hi):
            v = v3[i][None, :]
            w = b0 * v + s1
            s1 = (b1 * v - a1 * w) + s2
            s2 = b2 * v - a2 * w
            e = a * e + oa * np.abs(w[:, 2])
            Y[i - lo], E[i - lo] = w[:, :2], e
        p[:, lo:hi] = np.moveaxis(_band_sum(E, Y, S, B, g), 0, 1)
    end = np.empty((K, 7))
    end[:, 0:6:2], end[:, 1:6:2], end[:, 6] = s1, s2, e
    end = end.reshape(S, B, 7)
    return (p[0], end[0]) if single else (p, end)


def mix(x, p, wet=1.0, gain=1.0, angle=0.0):
    """Step 5 on p (float64, rounded here once): the float32 lerp, pan and gain."""
    x = np.asarray(x, np.float32)
    wet = np.float32(min(max(float(np.float32(wet)), 0.0), 1.0))
    with np.errstate(invalid="ignore", over="ignore"):
        out = x + wet * (p.astype(np.float32) - x)
        l, r = pan_gain(out[:, 0], out[:, 1], gain, angle)
    return np.stack([l, r], axis=1).astype(np.float32)


def process(x, key, sp, wet=1.0, gain=1.0, angle=0.0, state=None):
    x = np.asarray(x, np.float32)
    if np.float32(min(max(float(np.float32(wet)), 0.0), 1.0)) < np.float32(0.0001):   # dry: a Sum; key and state untouched
        l, r = pan_gain(x[:, 0].copy(), x[:, 1].copy(), gain, angle)
        return np.stack([l, r], axis=1).astype(np.float32), (np.zeros((sp["B"], 7)) if state is None else np.array(state, np.float64))
    p, end = serial(x, key, sp, state)
    return mix(x, p, wet, gain, angle), end


# ---- the device's tiled scans, emulated ----
def _scalar_scan(u, pw):
    """Hillis-Steele over the last axis (256 lanes) of u (K, .., 256) with the factors pw (K, 8): the inclusive join."""
    for k in range(8):
        off = 1 << k
        f = pw[:, k].reshape((-1,) + (1,) * (u.ndim - 1))
        v = u.copy()
        v[..., off:] = u[..., off:] + f * u[..., :-off]
        u = v
    return u


def _scalar_powers(a, chunk):
    """pwa[k] = a^(8 2^k), a_tile = a^2048, pwac[k] = a^(2048 chunk 2^k): long double, each rounded once."""
    p = np.asarray(a, np.longdouble) ** np.longdouble(RUN)
    pwa = []
    for _ in range(8):
        pwa.append(p.astype(np.float64))
        p = p * p
    a_tile = p.astype(np.float64)
    p = p ** np.longdouble(chunk)
    pwac = []
    for _ in range(8):
        pwac.append(p.astype(np.float64))
        p = p * p
    return np.stack(pwa, axis=1), a_tile, np.stack(pwac, axis=1)


def blocked(x, key, sp, state=None):
    """One spec.  The biquads as k_voc_local / k_voc_carry (mode 0) / k_voc_apply run them -- np_eq.blocked's steps on the three
    signals -- then the follower as k_voc_env / k_voc_carry (mode 1) / k_voc_apply: every lane's 8 frames from zero, the lanes
    joined by Hillis-Steele with a^(8 2^k), the tiles by the chunked carry, then every lane serially from its entry value."""
    B, c, a, g = sp["B"], sp["c"], np.full(sp["B"], sp["a"]), np.array([sp["g"]])
    K, C = B, 3
    v3 = signals(x, key)
    n = len(v3)
    T = (n + TILE - 1) // TILE
    chunk = (T + LANES - 1) // LANES
    xp = np.zeros((T * TILE, C))
    xp[:n] = v3
    xl = xp.reshape(1, T, LANES, RUN, C)
    b0, b1, b2, a1, a2 = (c[:, j].reshape(K, 1, 1, 1) for j in range(5))
    c0, c1 = b1 - a1 * b0, b2 - a2 * b0
    pw, a_tile, pwc = NE.powers(c[:, 3], c[:, 4], chunk)
    st = np.zeros((B, 7)) if state is None else np.asarray(state, np.float64)
    entry0 = np.stack([st[:, 0:6:2], st[:, 1:6:2]], axis=1)   # (K, 2, C)
    e0 = st[:, 6].copy()

    def zrun(s1, s2):
        for j in range(RUN):
            v = xl[:, :, :, j, :]
            s1, s2 = (c0 * v - a1 * s1) + s2, c1 * v - a2 * s1
        return np.stack([s1, s2], axis=-2)
    z = np.zeros((K, T, LANES, C))
    total = NE._lane_scan(zrun(z, z), pw)[:, :, -1]
    pad = np.zeros((K, LANES * chunk, 2, C))
    pad[:, :T] = total
    agg = pad.reshape(K, LANES, chunk, 2, C)
    u = np.zeros((K, LANES, 2, C))
    u[:, 0] = entry0
    for r in range(chunk):
        u = NE._mac(agg[:, :, r], a_tile, u)
    inc = NE._lane_scan(u, pwc)
    cur = np.concatenate([entry0[:, None], inc[:, :-1]], axis=1)
    entry = np.empty((K, LANES, chunk, 2, C))
    for r in range(chunk):
        entry[:, :, r] = cur
        cur = NE._mac(agg[:, :, r], a_tile, cur)
    entry = entry.reshape(K, LANES * chunk, 2, C)[:, :T]
    s1 = np.zeros((K, T, LANES, C))
    s2 = np.zeros((K, T, LANES, C))
    s1[:, :, 0], s2[:, :, 0] = entry[:, :, 0], entry[:, :, 1]
    inc = NE._lane_scan(zrun(s1, s2), pw)
    zin = np.concatenate([entry[:, :, None], inc[:, :, :-1]], axis=2)
    s1, s2 = zin[..., 0, :], zin[..., 1, :]
    y = np.empty((K, T, LANES, RUN, C))
    S1, S2 = np.empty_like(y), np.empty_like(y)
    for j in range(RUN):
        v = xl[:, :, :, j, :]
        w = b0 * v + s1
        s1 = (b1 * v - a1 * w) + s2
        s2 = b2 * v - a2 * w
        y[:, :, :, j, :], S1[:, :, :, j, :], S2[:, :, :, j, :] = w, s1, s2
    # the follower
    R = np.abs(y[..., 2])                                   # (K, T, LANES, RUN)
    ak, oak = a.reshape(K, 1, 1), (1.0 - a).reshape(K, 1, 1)
    pwa, at, pwac = _scalar_powers(a, chunk)

    def erun(e):
        for j in range(RUN):
            e = ak * e + oak * R[..., j]
        return e
    etot = _scalar_scan(erun(np.zeros((K, T, LANES))), pwa)[..., -1]   # (K, T): k_voc_env's tile words
    epad = np.zeros((K, LANES * chunk))
    epad[:, :T] = etot
    eagg = epad.reshape(K, LANES, chunk)
    u = np.zeros((K, LANES))
    u[:, 0] = e0
    for r in range(chunk):
        u = eagg[:, :, r] + at[:, None] * u
    inc = _scalar_scan(u, pwac)
    cur = np.concatenate([e0[:, None], inc[:, :-1]], axis=1)
    eentry = np.empty((K, LANES, chunk))
    for r in range(chunk):
        eentry[:, :, r] = cur
        cur = eagg[:, :, r] + at[:, None] * cur
    eentry = eentry.reshape(K, LANES * chunk)[:, :T]
    e = np.zeros((K, T, LANES))
    e[:, :, 0] = eentry
    inc = _scalar_scan(erun(e), pwa)
    e = np.concatenate([eentry[:, :, None], inc[:, :, :-1]], axis=2)
    E = np.empty((K, T, LANES, RUN))
    for j in range(RUN):
        e = ak * e + oak * R[..., j]
        E[..., j] = e
    E, Y = E.reshape(K, T * TILE), y.reshape(K, T * TILE, C)
    p = _band_sum(np.moveaxis(E, 0, 1)[:n], np.moveaxis(Y[..., :2], 0, 1)[:n], 1, B, g)[:, 0]
    end = np.empty((B, 7))
    if n:
        S1, S2 = S1.reshape(K, T * TILE, C), S2.reshape(K, T * TILE, C)
        end[:, 0:6:2], end[:, 1:6:2], end[:, 6] = S1[:, n - 1], S2[:, n - 1], E[:, n - 1]
    else:
        end[:] = st
    return p, end
