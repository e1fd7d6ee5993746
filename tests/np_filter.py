"""The filter vertex (TEST INFRASTRUCTURE): a float64 restatement of the definition in include/termdaw_amd.h
(td_graph_add_filter), operation for operation.  No reference counterpart exists for this vertex; the header's text is the
definition and this file is its twin.

    spec(consts, kind, stereo, shape)                                    what a case is to this file
    sweep_exp(t)                                                         E(t) of the header: the fixed multiplies and adds
    serial(x, specs, state=None, t0=0, key=None)  -> (p, end state)      the definition with plain loops, the cases side by side
    process(x, spec, wet=..., gain=..., angle=..., state=..., t0=..., key=...)   the vertex: (out float32, end state)
    blocked(x, specs, state=None, t0=0, key=None) -> (p, end state)      the tiled scans of the kernels restated: the follower's two
                                                                         scalar scans with their carries, then lane maps, Hillis-
                                                                         Steele joins of maps, the tiles in series, and every
                                                                         lane's run from its entry state

x: (frames, 2) float32, the vertex' summed input; key: the same shape, the summed key sources (None: the vertex listens to
itself).  consts = (g0, k, gmin, gmax, cl, ce, f, S, aA, 1 - aA, aR), the engine's own doubles (api.filter_params); kind is the
name or TD_FILTER_*, stereo the f32 parameter widened, shape the chorus' name or index.  A state is six float64 -- (y1, e, i1l,
i2l, i1r, i2r) -- zero where a render starts; t0 is the graph's absolute frame at x[0] (the LFO's n).  p is the filter's output
in float64, (frames, 2) -- or (K, frames, 2) for a list of K specs."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from np_chorus import lfo, shape_index  # noqa: E402  (the chorus' LFO: the filter has no second one)
from np_twin import pan_gain  # noqa: E402  (sample.rs:97-114 in float32, as the engine's make_pg)

KINDS = ("lowpass", "highpass", "bandpass", "notch")   # TD_FILTER_* in order
RUN, LANES = 8, 256     # kFiltRun, kThreads
TILE = RUN * LANES      # kFiltTile
C = tuple(1.0 / j for j in range(1, 11))   # c_j, the double nearest 1 / j


def kind_index(kind):
    return KINDS.index(kind) if isinstance(kind, str) else int(kind)


def spec(consts, kind, stereo, shape):
    return (tuple(float(c) for c in consts), kind_index(kind), float(np.float32(stereo)), shape_index(shape))


def sweep_exp(t):
    """E(t): x = t / 16, the degree-10 Horner form with c_j, squared four times."""
    x = np.asarray(t, np.float64) * 0.0625
    p = np.ones_like(x)
    for j in range(10, 0, -1):
        p = 1.0 + p * (x * C[j - 1])
    for _ in range(4):
        p = p * p
    return p


def _clean(x):
    return np.where(np.isfinite(x), x, np.float32(0.0)).astype(np.float64)


def level(key):
    """s[n] of step 1: max(|kl|, |kr|) in f32, widened; 0 for a frame with a NaN or an infinity."""
    k = np.abs(np.asarray(key, np.float32).reshape(-1, 2))
    ok = np.isfinite(k).all(axis=1)
    return np.where(ok, np.maximum(k[:, 0], k[:, 1]), np.float32(0.0)).astype(np.float64)


def follows(sp):
    return sp[0][5] != 0.0   # ce = ln2 env_oct: zero exactly when env_oct is


def coefs(sp, t0, e):
    """(a1, a2, a3) of both channels, each (n, 2), from e[n] (steps 2 and 3, and the division of step 4)."""
    (g0, k, gmin, gmax, cl, ce, f, S, aA, oA, aR), kind, stereo, shape = sp
    n = len(e)
    nn = (np.arange(n, dtype=np.uint64) + np.uint64(t0)).astype(np.float64)
    env = ce * np.minimum(S * e, 1.0)
    a1 = np.empty((n, 2))
    for c, phi in enumerate((0.0, stereo)):
        th = nn * f + phi
        th = th - np.floor(th)
        t = cl * lfo(shape, th) + env
        g = np.minimum(np.maximum(g0 * sweep_exp(t), gmin), gmax)
        a1[:, c] = 1.0 / (1.0 + g * (g + k))
        if c == 0:
            gl = g
    g2 = np.stack([gl, g], axis=1)
    a2 = g2 * a1
    a3 = g2 * a2
    return a1, a2, a3


def follower(s, sp, y1, e):
    """Steps 1's two recurrences, serially: (e[n], y1 end, e end)."""
    aA, oA, aR = sp[0][8], sp[0][9], sp[0][10]
    out = np.empty(len(s))
    for n, sn in enumerate(s.tolist()):
        v = aR * y1
        y1 = sn if sn >= v else v
        e = aA * e + oA * y1
        out[n] = e
    return out, y1, e


def _many(specs):
    single = isinstance(specs[0], tuple) and not isinstance(specs[0][0], tuple)
    return single, ([specs] if single else list(specs))


def _state(state, K):
    if state is None:
        return np.zeros((K, 6))
    return np.array(np.broadcast_to(np.asarray(state, np.float64), (K, 6)))


def _output(kind, kq, xs, v1, v2):
    """p of step 4 by kind (arrays over the cases: kind (K, 1), kq (K, 1))."""
    return np.where(kind == 0, v2, np.where(kind == 1, (xs - kq * v1) - v2, np.where(kind == 2, kq * v1, xs - kq * v1)))


def _levels(x, key, specs, st, t0, scan):
    """e[n] per case (K, n) and the follower's end values, through `scan` (the serial loop or the tiled one); a case whose
    follower does not run keeps (y1, e) and holds e[n] at that value (its ce is 0)."""
    n = len(x)
    s = level(x if key is None else key)
    ev = np.empty((len(specs), n))
    end = st[:, :2].copy()
    seen = {}   # (cases that share the follower's constants and entering values share its result)
    for i, sp in enumerate(specs):
        if follows(sp):
            k = (sp[0][8], sp[0][9], sp[0][10], st[i, 0], st[i, 1])
            if k not in seen:
                seen[k] = scan(s, sp, st[i, 0], st[i, 1])
            ev[i], end[i, 0], end[i, 1] = seen[k]
        else:
            ev[i] = st[i, 1]
    return ev, end


def serial(x, specs, state=None, t0=0, key=None):
    single, specs = _many(specs)
    K = len(specs)
    x = np.asarray(x, np.float32).reshape(-1, 2)
    xs = _clean(x)
    n = len(xs)
    st = _state(state, K)
    ev, fend = _levels(x, key, specs, st, t0, follower)
    co = [coefs(sp, t0, ev[i]) for i, sp in enumerate(specs)]
    a1, a2, a3 = (np.stack([c[j] for c in co]) for j in range(3))   # each (K, n, 2)
    kind = np.array([sp[1] for sp in specs]).reshape(K, 1)
    kq = np.array([sp[0][1] for sp in specs]).reshape(K, 1)
    i1, i2 = st[:, 2::2].copy(), st[:, 3::2].copy()   # each (K, 2): left, right
    out = np.empty((K, n, 2))
    for m in range(n):
        b1, b2, b3 = a1[:, m], a2[:, m], a3[:, m]
        v3 = xs[m] - i2
        v1 = b1 * i1 + b2 * v3
        v2 = (i2 + b2 * i1) + b3 * v3
        i1 = 2.0 * v1 - i1
        i2 = 2.0 * v2 - i2
        out[:, m] = _output(kind, kq, xs[m], v1, v2)
    end = np.stack([fend[:, 0], fend[:, 1], i1[:, 0], i2[:, 0], i1[:, 1], i2[:, 1]], axis=1)
    return (out[0], end[0]) if single else (out, end)


def process(x, sp, wet=1.0, gain=1.0, angle=0.0, state=None, t0=0, key=None, processed=False):
    """The vertex: (out float32 (frames, 2), end state); processed=True: p, the filter's output rounded to float32, instead of
    the mix, pan and gain."""
    x = np.asarray(x, np.float32).reshape(-1, 2)
    wet = np.float32(min(max(float(np.float32(wet)), 0.0), 1.0))
    if wet < np.float32(0.0001) and not processed:   # (the engine's test, in f32: 0.0001f itself is processed)
        l, r = pan_gain(x[:, 0].copy(), x[:, 1].copy(), gain, angle)
        return np.stack([l, r], axis=1).astype(np.float32), _state(state, 1)[0]
    v, end = serial(x, sp, state, t0, key)
    with np.errstate(invalid="ignore", over="ignore"):
        p = v.astype(np.float32)
        if processed:
            return p, end
        out = x + wet * (p - x)   # float32 throughout: the reference's lerp (adsr.rs:42)
        l, r = pan_gain(out[:, 0], out[:, 1], gain, angle)
    return np.stack([l, r], axis=1).astype(np.float32), end


# ---- the device's tiled scans, emulated ----
def _lane_scan(u, pw, add):
    """comp_lane_scan: the lanes' run-end values (.., LANES) joined by Hillis-Steele with the host's powers."""
    lanes = u.shape[-1]
    k, off = 0, 1
    while off < lanes:
        o = pw[k] * u[..., :-off]
        u = u.copy()
        u[..., off:] = (u[..., off:] + o) if add else np.maximum(u[..., off:], o)
        k, off = k + 1, off << 1
    return u


def _master_carry(agg, a, init, add, tile):
    """k_master_carry: the value entering each tile -- a lane folds `chunk` consecutive tiles, the lanes are joined with the
    host's powers a^(tile chunk 2^k), a second walk writes the carries."""
    T = len(agg)
    chunk = (T + LANES - 1) // LANES
    a_tile = math.pow(a, float(tile))
    pwc = [math.pow(a, float(tile) * float(chunk) * float(1 << k)) for k in range(8)]
    step = (lambda g, u: g + a_tile * u) if add else (lambda g, u: max(g, a_tile * u))
    u = np.zeros(LANES)
    for t in range(LANES):
        v = init if t == 0 else 0.0
        for r in range(t * chunk, min(t * chunk + chunk, T)):
            v = step(agg[r], v)
        u[t] = v
    u = _lane_scan(u, pwc, add)
    carry = np.empty(T)
    for t in range(LANES):
        v = init if t == 0 else u[t - 1]
        for r in range(t * chunk, min(t * chunk + chunk, T)):
            carry[r] = v
            v = step(agg[r], v)
    return carry


def _run_fold(y, a, o, u, add):
    """A lane's run from u: per frame u = a u + o y (add) or max(y, a u); returns the values per frame (.., run) and the last."""
    out = np.empty_like(y)
    for k in range(y.shape[-1]):
        u = (a * u + o * y[..., k]) if add else np.maximum(y[..., k], a * u)
        out[..., k] = u
    return out, u


def follower_blocked(s, sp, y1, e, run=RUN, lanes=LANES):
    """The follower as k_filt_detect / k_master_carry / k_filt_env / k_master_carry / k_filt_local run it (a chunk of one tile:
    the same steps inside k_filt_apply, entered with the carried values)."""
    aA, oA, aR = sp[0][8], sp[0][9], sp[0][10]
    tile = run * lanes
    n = len(s)
    T = (n + tile - 1) // tile
    sp_ = np.zeros(T * tile)
    sp_[:n] = s
    y = sp_.reshape(T, lanes, run)
    pwR = [math.pow(aR, float(run) * float(1 << k)) for k in range(8)]
    pwA = [math.pow(aA, float(run) * float(1 << k)) for k in range(8)]
    zero = np.zeros((T, lanes))
    # the release: tile totals from zero, their carry, then every lane from its entering value
    agg1 = _lane_scan(_run_fold(y, aR, None, zero, False)[1], pwR, False)[:, -1]
    c1 = _master_carry(agg1, aR, y1, False, tile) if T > 1 else np.array([y1])
    u = zero.copy()
    u[:, 0] = c1
    u = _lane_scan(_run_fold(y, aR, None, u, False)[1], pwR, False)
    uin = np.concatenate([c1[:, None], u[:, :-1]], axis=1)
    y1v = _run_fold(y, aR, None, uin, False)[0]
    # the attack, likewise on y1
    agg2 = _lane_scan(_run_fold(y1v, aA, oA, zero, True)[1], pwA, True)[:, -1]
    c2 = _master_carry(agg2, aA, e, True, tile) if T > 1 else np.array([e])
    b = zero.copy()
    b[:, 0] = c2
    b = _lane_scan(_run_fold(y1v, aA, oA, b, True)[1], pwA, True)
    bin_ = np.concatenate([c2[:, None], b[:, :-1]], axis=1)
    ev = _run_fold(y1v, aA, oA, bin_, True)[0]
    y1v, ev = y1v.reshape(-1)[:n], ev.reshape(-1)[:n]
    return ev, (y1v[-1] if n else y1), (ev[-1] if n else e)


def _frame(i1, i2, a1, a2, a3, xs):
    v3 = xs - i2
    v1 = a1 * i1 + a2 * v3
    v2 = (i2 + a2 * i1) + a3 * v3
    return 2.0 * v1 - i1, 2.0 * v2 - i2, v1, v2


def _join(own, left):
    """own o left on maps (.., 2, 3) = {P | q}: {P PL | P qL + q}, in the kernels' order."""
    pa, pb = own[..., :, 0:1], own[..., :, 1:2]
    acc = pa * left[..., 0:1, :] + pb * left[..., 1:2, :]
    acc[..., 2] = acc[..., 2] + own[..., 2]
    return acc


def _apply(m, s):
    """P s + q: m (.., 2, 3), s (.., 2)."""
    return (m[..., 0] * s[..., 0:1] + m[..., 1] * s[..., 1:2]) + m[..., 2]


def blocked(x, specs, state=None, t0=0, key=None, run=RUN, lanes=LANES, maps=None):
    """The vertex as the kernels run it, float64: the follower's tiled scans, then every lane's map from the
    identity through its `run` frames, the lanes' maps joined by Hillis-Steele, the tiles' totals applied in series from the
    entering state, each lane's entry state from the prefix in front of it, then the definition over the lane's run.  maps: a
    dict that receives the largest |word| of the prefix maps."""
    single, specs = _many(specs)
    K = len(specs)
    tile = run * lanes
    x = np.asarray(x, np.float32).reshape(-1, 2)
    xs = _clean(x)
    n = len(xs)
    T = (n + tile - 1) // tile
    st = _state(state, K)
    ev, fend = _levels(x, key, specs, st, t0, lambda s, sp, y1, e: follower_blocked(s, sp, y1, e, run, lanes))
    xp = np.zeros((T * tile, 2))
    xp[:n] = xs
    xl = xp.reshape(1, T, lanes, run, 2)
    evp = np.zeros((K, T * tile))
    evp[:, :n] = ev
    co = [coefs(sp, t0, evp[i]) for i, sp in enumerate(specs)]
    a1, a2, a3 = (np.stack([c[j] for c in co]).reshape(K, T, lanes, run, 2) for j in range(3))
    # a lane's map, per channel: (K, T, lanes, 2 channels, 2 rows, 3 columns) -- rows (i1, i2), columns the basis vectors and q
    P = np.zeros((K, T, lanes, 2, 2, 3))
    P[..., 0, 0] = 1.0
    P[..., 1, 1] = 1.0
    for j in range(run):
        b1, b2, b3 = a1[:, :, :, j, :, None], a2[:, :, :, j, :, None], a3[:, :, :, j, :, None]
        xin = np.zeros((1, T, lanes, 2, 3))
        xin[..., 2] = xl[:, :, :, j, :]
        n1, n2, _, _ = _frame(P[..., 0, :], P[..., 1, :], b1, b2, b3, xin)
        P = np.stack([n1, n2], axis=-2)
    inc = P
    off = 1
    while off < lanes:
        nxt = inc.copy()
        nxt[:, :, off:] = _join(inc[:, :, off:], inc[:, :, :-off])
        inc = nxt
        off <<= 1
    if maps is not None:
        maps["peak"] = max(maps.get("peak", 0.0), float(np.abs(inc).max()))
    total = inc[:, :, -1]   # (K, T, 2, 2, 3): k_filt_local's tile words
    # k_filt_carry: the tiles in series
    entry = np.empty((K, T, 2, 2))
    cur = st[:, 2:].reshape(K, 2, 2).copy()   # (K, channel, (i1, i2))
    for t in range(T):
        entry[:, t] = cur
        cur = _apply(total[:, t], cur)
    # k_filt_apply: lane 0 enters with the tile's state, lane t with the map of lanes 0 .. t - 1 applied to it
    zin = np.empty((K, T, lanes, 2, 2))
    zin[:, :, 0] = entry
    zin[:, :, 1:] = _apply(inc[:, :, :-1], entry[:, :, None])
    i1, i2 = zin[..., 0].copy(), zin[..., 1].copy()   # each (K, T, lanes, 2)
    kind = np.array([sp[1] for sp in specs]).reshape(K, 1, 1, 1)
    kq = np.array([sp[0][1] for sp in specs]).reshape(K, 1, 1, 1)
    out = np.empty((K, T, lanes, run, 2))
    last_t, last_l, last_j = (n - 1) // tile, ((n - 1) % tile) // run, (n - 1) % run
    zend = st[:, 2:].copy()
    for j in range(run):
        xj = xl[:, :, :, j, :]
        i1, i2, v1, v2 = _frame(i1, i2, a1[:, :, :, j], a2[:, :, :, j], a3[:, :, :, j], xj)
        out[:, :, :, j, :] = _output(kind, kq, xj, v1, v2)
        if j == last_j and n:
            a, b = i1[:, last_t, last_l], i2[:, last_t, last_l]   # each (K, 2)
            zend = np.stack([a[:, 0], b[:, 0], a[:, 1], b[:, 1]], axis=1)
    out = out.reshape(K, T * tile, 2)[:, :n]
    end = np.concatenate([fend, zend], axis=1)
    return (out[0], end[0]) if single else (out, end)
