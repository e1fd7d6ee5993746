"""The multiband vertex, serially (TEST INFRASTRUCTURE): a float64 restatement of the definition in include/termdaw_amd.h
(td_graph_add_multiband), with a plain loop for the recurrences.  No reference counterpart exists for this vertex; the header's
text is the definition and this file is its twin.

    spec(params, threshold_db, ratio, knee_db, makeup_db)  what the functions below take, from api.multiband_params' (sets, aA, aR)
    bands_serial(x, cos, states) -> (bands, ends)          step 2: the nine biquads per channel, frame by frame
    bands_blocked(x, cos, states) -> (bands, ends)         step 2 as the device's tiled scans run it: the kernels' tile geometry
                                                           (2 048 frames = 256 lanes x 8), the 18-state block operator, its 23
                                                           blocks' join order, powers in long double
    serial(x, specs, state) -> (p float64, end)            steps 2 .. 4 before the rounding to float32; specs (one, or a list) are
                                                           stepped together: p (S, frames, 2), end (S, 42)
    blocked(x, specs, state) -> (p float64, end)           the same over bands_blocked (derives the GPU test's bound E)
    process(x, spec, wet=, gain=, angle=, state=)          the whole vertex: (out float32 (frames, 2), end state (42,))

x: (frames, 2) float32, the vertex' summed input.  The constants come from td_multiband_params, so that a last-bit difference
between the host's libm and numpy's cannot show up as a filter difference.  The recurrences run in float64 (numpy float64: no fused
multiply-add), the lerp, pan and gain in float32.  The state is the line's: (s1, s2) of the nine biquads of the left channel, of
the right, then (y1, yL) of the low, mid and high band."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from np_twin import pan_gain  # noqa: E402

RUN, LANES = 8, 256
TILE = RUN * LANES
BIQUADS, WORDS, STATE = 9, 18, 42
SET_OF = (0, 0, 4, 1, 1, 2, 2, 3, 3)       # L1 L1 A2 | H1 H1 | L2 L2 | H2 H2: the coefficient set of biquad i
FEEDS = (-1, 0, 1, -1, 3, 4, 5, 4, 7)      # ... and the biquad whose output it filters (-1: x)
LOW, MID, HIGH = 2, 6, 8                   # the biquads whose outputs are the bands


def _reach(i):
    r = {i}
    while FEEDS[i] >= 0:
        i = FEEDS[i]
        r.add(i)
    return r


# the 2x2 blocks of the operator that are not zero, in row order: biquad c reaches biquad r
BLOCKS = [(r, c) for r in range(BIQUADS) for c in sorted(_reach(r))]
assert len(BLOCKS) == 23


def spec(params, threshold_db, ratio, knee_db, makeup_db):
    sets, aA, aR = params
    f = lambda v: np.asarray(np.asarray(v, np.float32), np.float64)   # noqa: E731  (the f32 parameters, widened)
    return dict(co=np.asarray(sets, np.float64).reshape(5, 5), aA=float(aA), aR=float(aR), T=f(threshold_db), slope=1.0 - 1.0 / f(ratio),
                W=float(np.float32(knee_db)), M=f(makeup_db))


def clean(x):
    """(frames, 2) float64: the input as it enters the filters (a non-finite sample enters as 0)."""
    x = np.asarray(x, np.float32)
    return np.where(np.isfinite(x), x, np.float32(0.0)).astype(np.float64)


def _frame(co, z, x):
    """One frame of the cascade in the definition's order.  co[s][i]: coefficient i of set s, broadcastable against x; z: the 18
    state words, a list; returns the nine outputs."""
    y = [None] * BIQUADS
    for i in range(BIQUADS):
        b0, b1, b2, a1, a2 = co[SET_OF[i]]
        u = x if FEEDS[i] < 0 else y[FEEDS[i]]
        w = b0 * u + z[2 * i]
        z[2 * i] = (b1 * u - a1 * w) + z[2 * i + 1]
        z[2 * i + 1] = b2 * u - a2 * w
        y[i] = w
    return y


def _co(cos, dims):
    """cos (S, 5, 5) -> co[s][i] of shape (S,) + (1,) * dims."""
    cos = np.asarray(cos, np.float64)
    return [[cos[:, s, i].reshape((-1,) + (1,) * dims) for i in range(5)] for s in range(5)]


def _entry(states, S):
    st = np.zeros((S, 2, WORDS)) if states is None else np.broadcast_to(np.asarray(states, np.float64)[..., :2 * WORDS].reshape(-1, 2, WORDS), (S, 2, WORDS)).copy()
    return st


def bands_serial(x, cos, states=None):
    """bands (S, frames, 3, 2) -- low, mid, high per channel -- and the filters' end states (S, 2, 18)."""
    cos = np.asarray(cos, np.float64).reshape(-1, 5, 5)
    S = len(cos)
    xs = clean(x)
    n = len(xs)
    co = _co(cos, 1)
    st = _entry(states, S)
    z = [st[:, :, w].copy() for w in range(WORDS)]   # (S, 2) each
    out = np.empty((n, 3, S, 2))
    for i in range(n):
        y = _frame(co, z, xs[i][None, :])
        out[i, 0], out[i, 1], out[i, 2] = y[LOW], y[MID], y[HIGH]
    return np.moveaxis(out, 2, 0), np.stack(z, axis=-1)


# ---- the operator and its powers, in long double (csrc/multiband_math.h, step by step) ----
def operator(co):
    """A (18, 18) long double: column j is one frame from the unit state e_j with x = 0."""
    col = [[np.longdouble(co[s][i]) for i in range(5)] for s in range(5)]
    eye = np.eye(WORDS, dtype=np.longdouble)
    z = [eye[:, w].copy() for w in range(WORDS)]     # entry j of every word: the start e_j
    _frame(col, z, np.zeros(WORDS, np.longdouble))
    return np.stack(z, axis=0)                       # [i][j] = word i after the frame from e_j


def _mul(a, b):
    r = np.zeros((WORDS, WORDS), np.longdouble)
    for k in range(WORDS):   # s += a[i][k] b[k][j], k ascending
        r = r + a[:, k:k + 1] * b[k:k + 1, :]
    return r


def _power(a, n):
    """a^n, n >= 1: square and multiply from the lowest bit."""
    r, have = a, False
    while n:
        if n & 1:
            r = _mul(r, a) if have else a
            have = True
        if n > 1:
            a = _mul(a, a)
        n >>= 1
    return r


def _store(p):
    """The 23 blocks, each rounded once: (23, 4) = (p00, p01, p10, p11)."""
    return np.array([[p[2 * r, 2 * c], p[2 * r, 2 * c + 1], p[2 * r + 1, 2 * c], p[2 * r + 1, 2 * c + 1]] for r, c in BLOCKS], np.longdouble).astype(np.float64)


def powers(co, chunk):
    """pw (8, 23, 4) = A^(8 2^k), a_tile (23, 4) = A^2048, pwc (8, 23, 4) = A^(2048 chunk 2^k)."""
    p = _power(operator(co), RUN)
    pw = []
    for _ in range(8):
        pw.append(_store(p))
        p = _mul(p, p)
    a_tile = _store(p)
    p = _power(p, chunk)
    pwc = []
    for _ in range(8):
        pwc.append(_store(p))
        p = _mul(p, p)
    return np.stack(pw), a_tile, np.stack(pwc)


def _matvec_add(P, o, u):
    """u + P o over the 23 blocks in their order (mb_matvec_add): P (S, 23, 4); o, u (S, .., 18).  Returns the new u."""
    u = u.copy()
    sh = (-1,) + (1,) * (u.ndim - 2)
    for b, (r, c) in enumerate(BLOCKS):
        p0, p1, p2, p3 = (P[:, b, e].reshape(sh) for e in range(4))
        o0, o1 = o[..., 2 * c], o[..., 2 * c + 1]
        u[..., 2 * r] = u[..., 2 * r] + (p0 * o0 + p1 * o1)
        u[..., 2 * r + 1] = u[..., 2 * r + 1] + (p2 * o0 + p3 * o1)
    return u


def _lane_scan(u, pw):
    """Hillis-Steele over the lane axis (-3) of u (S, .., 256, 2, 18) with pw (S, 8, 23, 4): the inclusive join."""
    for k in range(8):
        off = 1 << k
        v = u.copy()
        v[..., off:, :, :] = _matvec_add(pw[:, k], u[..., :-off, :, :], u[..., off:, :, :])
        u = v
    return u


def bands_blocked(x, cos, states=None):
    """bands_serial's result as k_mb_local / k_mb_carry / k_mb_detect / k_mb_apply reach it: every lane's 8 frames from zero, the
    lanes joined by Hillis-Steele with the blocks of A^(8 2^k), the tiles by the chunked carry, then every lane serially from
    its entry state."""
    cos = np.asarray(cos, np.float64).reshape(-1, 5, 5)
    S = len(cos)
    xs = clean(x)
    n = len(xs)
    T = max(1, (n + TILE - 1) // TILE)
    chunk = (T + LANES - 1) // LANES
    xp = np.zeros((T * TILE, 2))
    xp[:n] = xs
    xl = xp.reshape(1, T, LANES, RUN, 2)
    co = _co(cos, 3)
    pws = [powers(c, chunk) for c in cos]
    pw, a_tile, pwc = (np.stack([p[i] for p in pws]) for i in range(3))
    entry0 = _entry(states, S)                      # (S, 2, 18)

    def run(z0):                                    # z0 (S, T, LANES, 2, 18) -> the run-end states
        z = [z0[..., w].copy() for w in range(WORDS)]
        for j in range(RUN):
            _frame(co, z, xl[:, :, :, j, :])
        return np.stack(z, axis=-1)
    zero = np.zeros((S, T, LANES, 2, WORDS))
    total = _lane_scan(run(zero), pw)[:, :, -1]     # (S, T, 2, 18): k_mb_local's tile words
    pad = np.zeros((S, LANES * chunk, 2, WORDS))
    pad[:, :T] = total
    agg = pad.reshape(S, LANES, chunk, 2, WORDS)
    u = np.zeros((S, LANES, 2, WORDS))
    u[:, 0] = entry0
    for r in range(chunk):
        u = _matvec_add(a_tile, u, agg[:, :, r])
    inc = _lane_scan(u, pwc)
    cur = np.concatenate([entry0[:, None], inc[:, :-1]], axis=1)
    entry = np.empty((S, LANES, chunk, 2, WORDS))
    for r in range(chunk):
        entry[:, :, r] = cur
        cur = _matvec_add(a_tile, cur, agg[:, :, r])
    entry = entry.reshape(S, LANES * chunk, 2, WORDS)[:, :T]     # k_mb_carry's
    z0 = zero.copy()
    z0[:, :, 0] = entry
    inc = _lane_scan(run(z0), pw)
    zin = np.concatenate([entry[:, :, None], inc[:, :, :-1]], axis=2)
    z = [zin[..., w].copy() for w in range(WORDS)]
    bands = np.empty((S, T, LANES, RUN, 3, 2))
    Z = np.empty((S, T, LANES, RUN, 2, WORDS))
    for j in range(RUN):
        y = _frame(co, z, xl[:, :, :, j, :])
        bands[:, :, :, j, 0], bands[:, :, :, j, 1], bands[:, :, :, j, 2] = y[LOW], y[MID], y[HIGH]
        Z[:, :, :, j] = np.stack(z, axis=-1)
    bands = bands.reshape(S, T * TILE, 3, 2)[:, :n]
    end = Z.reshape(S, T * TILE, 2, WORDS)[:, n - 1] if n else entry0
    return bands, end


# ---- steps 3 and 4 ----
def wanted(bands, T, slope, W):
    """d_b[n] of the compressor's steps 1 and 2 on the f64 band signals: bands (.., frames, 3, 2); T, slope (.., 1, 3); W (.., 1, 1)."""
    al, ar = np.abs(bands[..., 0]), np.abs(bands[..., 1])
    s = np.maximum(al, ar)
    ok = np.isfinite(al) & np.isfinite(ar) & (s > 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        o = 20.0 * np.log10(np.where(ok, s, 1.0)) - T
        d = np.zeros(o.shape)
        Ws = np.where(W > 0.0, W, 1.0)
        t = o + W / 2.0
        knee = ok & (W > 0.0) & (2.0 * o >= -W) & (2.0 * np.abs(o) <= W)
        d = np.where(knee, slope * (t * t) / (2.0 * Ws), d)
        d = np.where(ok & (2.0 * o > W), slope * o, d)
    return d


def gains(d, aR, aA, M, y1, yL):
    """Steps 3 and 4 serially over d (K, frames, 3) with aR, aA (K, 1), M (K, 3) from (y1, yL) (K, 3): G (K, frames, 3), the ends."""
    oA = 1.0 - aA
    y1, yL = y1.copy(), yL.copy()
    n = d.shape[1]
    Y = np.empty((n,) + y1.shape)
    dn = np.moveaxis(d, 1, 0)
    for i in range(n):
        y1 = np.maximum(dn[i], aR * y1)
        yL = aA * yL + oA * y1
        Y[i] = yL
    return np.power(10.0, (M[None] - Y) / 20.0).transpose(1, 0, 2), y1, yL


def _run(x, specs, state, crossover):
    single = isinstance(specs, dict)
    specs = [specs] if single else list(specs)
    S = len(specs)
    st = np.zeros((S, STATE)) if state is None else np.broadcast_to(np.asarray(state, np.float64), (S, STATE)).copy()
    # the specs that share a crossover (and its entry state) share its run
    keys, groups = {}, []
    for i, sp in enumerate(specs):
        k = (sp["co"].tobytes(), st[i, :2 * WORDS].tobytes())
        if k not in keys:
            keys[k] = len(groups)
            groups.append(i)
        keys[i] = keys[k]
    bands, zend = crossover(x, np.stack([specs[i]["co"] for i in groups]), np.stack([st[i] for i in groups]))
    which = np.array([keys[i] for i in range(S)])
    bands, zend = bands[which], zend[which]                       # (S, frames, 3, 2), (S, 2, 18)
    col = lambda k: np.array([sp[k] for sp in specs])             # noqa: E731
    T, slope, M = col("T"), col("slope"), col("M")
    W, aR, aA = col("W").reshape(S, 1, 1), col("aR").reshape(S, 1), col("aA").reshape(S, 1)
    d = wanted(bands, T[:, None, :], slope[:, None, :], W)
    G, y1, yL = gains(d, aR, aA, M, st[:, 2 * WORDS::2], st[:, 2 * WORDS + 1::2])
    p = ((0.0 + bands[:, :, 0] * G[:, :, 0, None]) + bands[:, :, 1] * G[:, :, 1, None]) + bands[:, :, 2] * G[:, :, 2, None]
    end = np.empty((S, STATE))
    end[:, :2 * WORDS] = zend.reshape(S, 2 * WORDS)
    end[:, 2 * WORDS::2], end[:, 2 * WORDS + 1::2] = y1, yL
    return (p[0], end[0]) if single else (p, end)


def serial(x, specs, state=None):
    return _run(x, specs, state, bands_serial)


def blocked(x, specs, state=None):
    return _run(x, specs, state, bands_blocked)


def mix(x, p, wet=1.0, gain=1.0, angle=0.0):
    """Step 4's second half on p (float64, rounded here once): the float32 lerp, pan and gain."""
    x = np.asarray(x, np.float32)
    wet = np.float32(min(max(float(np.float32(wet)), 0.0), 1.0))
    with np.errstate(invalid="ignore", over="ignore"):
        out = x + wet * (p.astype(np.float32) - x)
        l, r = pan_gain(out[:, 0], out[:, 1], gain, angle)
    return np.stack([l, r], axis=1).astype(np.float32)


def process(x, sp, wet=1.0, gain=1.0, angle=0.0, state=None, scans=serial):
    x = np.asarray(x, np.float32)
    if np.float32(min(max(float(np.float32(wet)), 0.0), 1.0)) < np.float32(0.0001):   # dry: a Sum; the state untouched
        l, r = pan_gain(x[:, 0].copy(), x[:, 1].copy(), gain, angle)
        return np.stack([l, r], axis=1).astype(np.float32), (np.zeros(STATE) if state is None else np.array(state, np.float64))
    p, end = scans(x, sp, state)
    return mix(x, p, wet, gain, angle), end
