"""The phaser vertex (TEST INFRASTRUCTURE): a float64 restatement of the definition in include/termdaw_amd.h
(td_graph_add_phaser), operation for operation.  No reference counterpart exists for this vertex; the header's text is the
definition and this file is its twin.

    spec(consts, stereo, shape)                                          what a case is to this file
    serial(x, specs, state=None, t0=0)       -> (v, end state)           the definition with plain loops, the cases side by side
    process(x, spec, wet=..., gain=..., angle=..., state=..., t0=...)    the vertex: (out float32, end state)
    blocked(x, specs, state=None, t0=0)      -> (v, end state)           the tiled scan of the kernels restated: lane maps pushed
                                                                         column by column, Hillis-Steele joins of maps, the tiles
                                                                         in series, then every lane's run from its entry state

x: (frames, 2) float32, the vertex' summed input.  consts = (N, a_lo, a_hi, am, ad, f, fb), the engine's own doubles
(api.phaser_params); stereo is the f32 parameter widened, shape the chorus' name or index.  A state is (D, 2) float64 --
(s_1 .. s_N, z) per channel -- zero where a render starts; t0 is the graph's absolute frame at x[0] (the LFO's n).  v is the
chain's output in float64, (frames, 2) -- or (K, frames, 2) for a list of K specs, which must share N."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from np_chorus import lfo, shape_index  # noqa: E402  (the chorus' LFO: the phaser has no second one)
from np_twin import pan_gain  # noqa: E402  (sample.rs:97-114 in float32, as the engine's make_pg)

RUN, LANES = 32, 64     # kPhaserRun, kPhaserLanes
TILE = RUN * LANES      # kPhaserTile


def spec(consts, stereo, shape):
    return (tuple(consts), float(np.float32(stereo)), shape_index(shape))


def _clean(x):
    return np.where(np.isfinite(x), x, np.float32(0.0)).astype(np.float64)


def coef(sp, t0, n):
    """a[n] of both channels, (n, 2): th = n f + phi; th = th - floor(th); a = am + ad lfo(th)."""
    (N, a_lo, a_hi, am, ad, f, fb), stereo, shape = sp
    nn = (np.arange(n, dtype=np.uint64) + np.uint64(t0)).astype(np.float64)
    out = np.empty((n, 2))
    for c, phi in enumerate((0.0, stereo)):
        th = nn * f + phi
        th = th - np.floor(th)
        out[:, c] = am + ad * lfo(shape, th)
    return out


def _many(specs):
    single = isinstance(specs[0], tuple) and not isinstance(specs[0][0], tuple)
    specs = [specs] if single else list(specs)
    N = int(specs[0][0][0])
    assert all(int(s[0][0]) == N for s in specs)
    return single, specs, N, np.array([s[0][6] for s in specs]).reshape(-1, 1)


def _state(state, K, D):
    if state is None:
        return np.zeros((K, D, 2))
    return np.array(np.broadcast_to(np.asarray(state, np.float64), (K, D, 2)))


def serial(x, specs, state=None, t0=0):
    single, specs, N, fb = _many(specs)
    K, D = len(specs), N + 1
    xs = _clean(np.asarray(x, np.float32).reshape(-1, 2))
    n = len(xs)
    a = np.stack([coef(s, t0, n) for s in specs])   # (K, n, 2)
    st = _state(state, K, D)
    S = [st[:, k].copy() for k in range(D)]
    out = np.empty((K, n, 2))
    for i in range(n):
        ai = a[:, i]
        v = xs[i] + fb * S[N]
        for k in range(N):
            w = ai * v + S[k]
            S[k] = v - ai * w
            v = w
        S[N] = v
        out[:, i] = v
    end = np.stack(S, axis=1)
    return (out[0], end[0]) if single else (out, end)


def process(x, sp, wet=1.0, gain=1.0, angle=0.0, state=None, t0=0, processed=False):
    """The vertex: (out float32 (frames, 2), end state); processed=True: p, the chain's output rounded to float32, instead of
    the mix, pan and gain."""
    x = np.asarray(x, np.float32).reshape(-1, 2)
    wet = np.float32(min(max(float(np.float32(wet)), 0.0), 1.0))
    D = int(sp[0][0]) + 1
    if wet < np.float32(0.0001) and not processed:   # (the engine's test, in f32: 0.0001f itself is processed)
        l, r = pan_gain(x[:, 0].copy(), x[:, 1].copy(), gain, angle)
        return np.stack([l, r], axis=1).astype(np.float32), _state(state, 1, D)[0]
    v, end = serial(x, sp, state, t0)
    with np.errstate(invalid="ignore", over="ignore"):
        p = v.astype(np.float32)
        if processed:
            return p, end
        out = x + wet * (p - x)   # float32 throughout: the reference's lerp (adsr.rs:42)
        l, r = pan_gain(out[:, 0], out[:, 1], gain, angle)
    return np.stack([l, r], axis=1).astype(np.float32), end


# ---- the device's tiled scan, emulated ----
def _join(own, left, D):
    """own o left on maps (.., D, D + 1) = {P | q}: the product's columns in the kernels' order -- P_own[i, 0] c[0], then
    + P_own[i, k] c[k] ascending, then + q_own on the last column."""
    acc = own[..., :, 0:1] * left[..., 0:1, :]
    for k in range(1, D):
        acc = acc + own[..., :, k:k + 1] * left[..., k:k + 1, :]
    acc[..., D] = acc[..., D] + own[..., D]
    return acc


def _apply(m, s, D):
    """P s + q in the same order: m (.., D, D + 1), s (.., D)."""
    acc = m[..., :, 0] * s[..., 0:1]
    for k in range(1, D):
        acc = acc + m[..., :, k] * s[..., k:k + 1]
    return acc + m[..., :, D]


def blocked(x, specs, state=None, t0=0, run=RUN, lanes=LANES, maps=None):
    """The scan as k_phaser_local / k_phaser_carry / k_phaser_apply run it, float64: every lane's map from the
    identity through its `run` frames, the lanes' maps joined by Hillis-Steele, the tiles' totals applied in series from the
    entering state, each lane's entry state from the prefix in front of it, then the definition over the lane's run.  maps: a
    dict that receives the largest |word| of the prefix maps."""
    single, specs, N, fb = _many(specs)
    K, D, W = len(specs), N + 1, N + 2
    tile = run * lanes
    xs = _clean(np.asarray(x, np.float32).reshape(-1, 2))
    n = len(xs)
    T = (n + tile - 1) // tile
    xp = np.zeros((T * tile, 2))
    xp[:n] = xs
    xl = xp.reshape(1, T, lanes, run, 2)
    a = np.stack([coef(s, t0, T * tile) for s in specs]).reshape(K, T, lanes, run, 2)
    fbm = fb.reshape(K, 1, 1, 1, 1)
    # a lane's map, per channel: (K, T, lanes, 2, D, W), rows the state's words, columns the basis vectors and q
    P = np.zeros((K, T, lanes, 2, D, W))
    for i in range(D):
        P[..., i, i] = 1.0
    for j in range(run):
        aj = a[:, :, :, j, :, None]
        v = fbm * P[..., N, :]
        v[..., D] = xl[:, :, :, j, :] + v[..., D]
        for k in range(N):
            w = aj * v + P[..., k, :]
            P[..., k, :] = v - aj * w
            v = w
        P[..., N, :] = v
    inc = P
    off = 1
    while off < lanes:
        nxt = inc.copy()
        nxt[:, :, off:] = _join(inc[:, :, off:], inc[:, :, :-off], D)
        inc = nxt
        off <<= 1
    if maps is not None:
        maps["peak"] = max(maps.get("peak", 0.0), float(np.abs(inc).max()))
    total = inc[:, :, -1]   # (K, T, 2, D, W): k_phaser_local's tile words
    # k_phaser_carry: the tiles in series
    entry = np.empty((K, T, 2, D))
    cur = np.moveaxis(_state(state, K, D), 1, 2)   # (K, 2, D)
    for t in range(T):
        entry[:, t] = cur
        cur = _apply(total[:, t], cur, D)
    # k_phaser_apply: lane 0 enters with the tile's state, lane t with the map of lanes 0 .. t - 1 applied to it
    zin = np.empty((K, T, lanes, 2, D))
    zin[:, :, 0] = entry
    zin[:, :, 1:] = _apply(inc[:, :, :-1], entry[:, :, None], D)
    S = [zin[..., k].copy() for k in range(D)]   # each (K, T, lanes, 2)
    out = np.empty((K, T, lanes, run, 2))
    last_t, last_l, last_j = (n - 1) // tile, ((n - 1) % tile) // run, (n - 1) % run
    end = None
    fbl = fb.reshape(K, 1, 1, 1)
    for j in range(run):
        aj = a[:, :, :, j, :]
        v = xl[:, :, :, j, :] + fbl * S[N]
        for k in range(N):
            w = aj * v + S[k]
            S[k] = v - aj * w
            v = w
        S[N] = v
        out[:, :, :, j, :] = v
        if j == last_j and n:
            end = np.stack([s[:, last_t, last_l] for s in S], axis=1)   # (K, D, 2)
    out = out.reshape(K, T * tile, 2)[:, :n]
    if end is None:
        end = _state(state, K, D)
    return (out[0], end[0]) if single else (out, end)
