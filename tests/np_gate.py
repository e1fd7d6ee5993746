"""The gate vertex (TEST INFRASTRUCTURE): a float64 restatement of the definition in include/termdaw_amd.h (td_graph_add_gate).
No reference counterpart exists for this vertex; the header's text is the definition and this file is its twin.

    process(x, consts, wet=..., gain=..., angle=..., state=(env, h, c))  -> (out, end state)     the serial twin: plain loops
    target(cls, H, state) / fade(t, aA, aR, env0)                        the same two recurrences, array-at-a-time: target() by
                                                                         index arithmetic (integers: exact), fade() frame by
                                                                         frame with the cases side by side (elementwise float64:
                                                                         the loop's own operations, bit for bit)
    blocked(cls, consts, state, tile=2048, run=8, carry_lanes=256)       the tiled scan of the kernels restated: lane runs,
                                                                         Hillis-Steele joins, tile carries, in their order

x: (frames, 2) float32, the vertex' summed input.  consts = (To, Tc, H, aA, aR, F), the engine's own doubles
(api.gate_params).  A state is (env, h, c); closed(H) = (0.0, 0, H + 1) is where a render starts.  Steps 1-5 run in float64,
step 6 (the reference's lerp, pan, gain) in float32."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from np_twin import pan_gain  # noqa: E402  (sample.rs:97-114 in float32, as the engine's make_pg)


def closed(H):
    return (0.0, 0, int(H) + 1)


def classes(x, To, Tc):
    """Steps 1 and 2's reading of every frame: 1 opens (s >= To), 2 closes (s < Tc), 0 forces nothing (in between, or a frame
    with a NaN / infinite sample)."""
    x = np.asarray(x, np.float32)
    ok = np.isfinite(x[:, 0]) & np.isfinite(x[:, 1])
    s = np.maximum(np.abs(x[:, 0]), np.abs(x[:, 1])).astype(np.float64)
    s = np.where(ok, s, 0.0)
    return np.where(ok & (s >= To), 1, np.where(ok & (s < Tc), 2, 0)).astype(np.int8)


def serial(cls, consts, state):
    """Steps 2-4 with plain loops: (t[n] uint8, env[n] float64, end state)."""
    To, Tc, H, aA, aR, F = consts
    env, h, c = float(state[0]), int(state[1]), int(state[2])
    n = len(cls)
    t_out, e_out = np.empty(n, np.uint8), np.empty(n)
    cl = np.asarray(cls).tolist()
    for i in range(n):
        k = cl[i]
        if k == 1:
            h = 1
        elif k == 2:
            h = 0
        c = 0 if h == 1 else min(c + 1, H + 1)
        t = 1 if c <= H else 0
        a = aA if t == 1 else aR
        env = a * env + (1.0 - a) * float(t)
        t_out[i] = t
        e_out[i] = env
    return t_out, e_out, (env, h, c)


def target(cls, H, state):
    """Steps 2 and 3 by index arithmetic: (h[n], c[n], t[n]) and the end (h, c)."""
    cls = np.asarray(cls)
    n = len(cls)
    if n == 0:
        return np.zeros(0, np.uint8), np.zeros(0, np.int64), np.zeros(0, np.uint8), (int(state[1]), int(state[2]))
    idx = np.arange(n)
    last = np.maximum.accumulate(np.where(cls != 0, idx, -1))
    h = np.where(last >= 0, cls[np.maximum(last, 0)] == 1, bool(state[1]))
    lo = np.maximum.accumulate(np.where(h, idx, -1))
    c = np.minimum(np.where(lo >= 0, idx - lo, int(state[2]) + idx + 1), H + 1)
    return h.astype(np.uint8), c.astype(np.int64), (c <= H).astype(np.uint8), (int(h[-1]), int(c[-1]))


def fade(t, aA, aR, env0):
    """Step 4 along the last axis, the leading axes side by side: t (..., n) of 0 / 1, aA / aR / env0 broadcast over the leading
    axes.  Every operation is the serial loop's, elementwise in float64."""
    t = np.asarray(t)
    lead = t.shape[:-1]
    aA, aR = np.broadcast_to(np.asarray(aA, np.float64), lead), np.broadcast_to(np.asarray(aR, np.float64), lead)
    env = np.array(np.broadcast_to(np.asarray(env0, np.float64), lead))
    oA, oR = 1.0 - aA, 1.0 - aR
    out = np.empty(t.shape)
    for i in range(t.shape[-1]):
        ti = t[..., i] != 0
        env = np.where(ti, aA, aR) * env + np.where(ti, oA, oR) * ti.astype(np.float64)
        out[..., i] = env
    return out


def gain_stage(x, env, F, wet=1.0, gain=1.0, angle=0.0, processed=False):
    """Steps 5 and 6 from env[n]."""
    x = np.asarray(x, np.float32)
    wet = np.float32(min(max(float(np.float32(wet)), 0.0), 1.0))
    G = F + (1.0 - F) * env
    with np.errstate(invalid="ignore", over="ignore"):
        p = (x.astype(np.float64) * G[:, None]).astype(np.float32)
        if processed:
            return p
        out = x + wet * (p - x)   # float32 throughout: the reference's lerp (adsr.rs:42)
        l, r = pan_gain(out[:, 0], out[:, 1], gain, angle)
    return np.stack([l, r], axis=1).astype(np.float32)


def process(x, consts, wet=1.0, gain=1.0, angle=0.0, state=None, processed=False):
    """The serial twin.  Returns (out float32 (frames, 2), end state); processed=True: p of step 5 instead of step 6's mix, pan
    and gain."""
    x = np.asarray(x, np.float32)
    To, Tc, H, aA, aR, F = consts
    state = closed(H) if state is None else state
    if np.float32(min(max(float(np.float32(wet)), 0.0), 1.0)) < np.float32(0.0001) and not processed:   # (0.0001f itself is processed)
        l, r = pan_gain(x[:, 0].copy(), x[:, 1].copy(), gain, angle)
        return np.stack([l, r], axis=1).astype(np.float32), state
    _, env, end = serial(classes(x, To, Tc), consts, state)
    return gain_stage(x, env, F, wet, gain, angle, processed), end


# ---- the tiled scan, as the kernels run it (kernels.h GateDesc) ----
# A map: (h, R, k), each of shape (2, ...) -- index 0 / 1: the entering h.  h: the leaving h; R: c restarts; k: closed frames since
# the restart, or on top of the entering c; capped at cap = H + 1.  A state (h, c) is the constant map (h, restart, c).
def _identity(shape):
    h = np.zeros((2,) + shape, bool)
    h[1] = True
    return h, np.zeros((2,) + shape, bool), np.zeros((2,) + shape, np.int64)


def _step(m, cls, valid, cap):
    h, R, k = m
    hn = np.where(cls == 1, True, np.where(cls == 2, False, h))
    Rn = np.where(hn, True, R)
    kn = np.where(hn, 0, np.minimum(k + 1, cap))
    return np.where(valid, hn, h), np.where(valid, Rn, R), np.where(valid, kn, k)


def _join(l, r, cap):
    """l then r (r's leading axis, the entering h, is selected by l's leaving h)."""
    lh, lR, lk = l
    rh, rR, rk = (np.where(lh, a[1], a[0]) for a in r)
    return rh, np.where(rR, True, lR), np.where(rR, rk, np.minimum(lk + rk, cap))


def _hs_maps(m, cap):
    """Hillis-Steele along the last axis: inclusive prefixes."""
    L, off = m[0].shape[-1], 1
    while off < L:
        left = tuple(a[..., :-off] for a in m)
        mine = tuple(a[..., off:] for a in m)
        j = _join(left, mine, cap)
        m = tuple(np.concatenate([a[..., :off], b], axis=-1) for a, b in zip(m, j))
        off *= 2
    return m


def _hs_pairs(A, B):
    L, off = A.shape[-1], 1
    while off < L:
        Bn, An = B.copy(), A.copy()
        Bn[..., off:] = A[..., off:] * B[..., :-off] + B[..., off:]
        An[..., off:] = A[..., :-off] * A[..., off:]
        A, B, off = An, Bn, off * 2
    return A, B


def _excl_maps(inc):
    ident = _identity(inc[0].shape[1:-1] + (1,))
    return tuple(np.concatenate([i, a[..., :-1]], axis=-1) for i, a in zip(ident, inc))


def _state_word(h, c):
    return np.array(bool(h)), np.array(True), np.array(int(c), np.int64)


def _apply(word, m, cap):
    """A state word behind a map."""
    h, R, k = word
    rh, rR, rk = (np.where(h, a[1], a[0]) for a in m)
    return rh, np.where(rR, True, R), np.where(rR, rk, np.minimum(k + rk, cap))


def blocked(cls, consts, state=None, tile=2048, run=8, carry_lanes=256):
    """(t[n], env[n], end state) the way the five launches compute them."""
    To, Tc, H, aA, aR, F = consts
    cap = H + 1
    state = closed(H) if state is None else state
    n = len(cls)
    lanes = tile // run
    T = max(1, -(-n // tile))
    pad = np.full(T * tile, -1, np.int64)
    pad[:n] = cls
    cl = pad.reshape(T, lanes, run)
    valid = cl >= 0
    # k_gate_detect: each lane folds its frames into a map, the lanes are joined; the tile's map is the last lane's prefix
    m = _identity((T, lanes))
    for j in range(run):
        m = _step(m, cl[None, :, :, j], valid[None, :, :, j], cap)
    inc = _hs_maps(m, cap)
    tile_map = tuple(a[..., -1] for a in inc)          # (2, T)
    excl = _excl_maps(inc)
    # k_gate_carry (discrete): a lane folds `chunk` consecutive tiles, the lanes are joined, a second walk writes the carries
    chunk = -(-T // carry_lanes)
    busy = min(carry_lanes, -(-T // chunk))   # (the lanes behind hold the identity and write nothing)
    cm = _identity((carry_lanes,))
    for q in range(busy):
        for r in range(min(q * chunk, T), min(q * chunk + chunk, T)):
            j = _join(tuple(a[:, q] for a in cm), tuple(a[:, r] for a in tile_map), cap)
            for a, b in zip(cm, j):
                a[:, q] = b
    cex = _excl_maps(_hs_maps(cm, cap))
    init = _state_word(state[1], min(int(state[2]), cap))
    ent_h, ent_k = np.empty(T, bool), np.empty(T, np.int64)
    for q in range(busy):
        w = _apply(init, tuple(a[:, q] for a in cex), cap)
        for r in range(min(q * chunk, T), min(q * chunk + chunk, T)):
            ent_h[r], ent_k[r] = w[0], w[2]
            w = _apply(w, tuple(a[:, r] for a in tile_map), cap)
    # k_gate_env: the state entering each lane's run, t[n], the lanes' pairs and the tile's pair
    w = _apply((ent_h[:, None], np.ones((T, 1), bool), ent_k[:, None]), excl, cap)
    w = (w[0], w[1], w[2])
    t = np.zeros((T, lanes, run), np.uint8)
    A, B = np.ones((T, lanes)), np.zeros((T, lanes))
    end_h, end_c = int(state[1]), int(state[2])
    for j in range(run):
        v = valid[:, :, j]
        h, R, k = w
        hn = np.where(cl[:, :, j] == 1, True, np.where(cl[:, :, j] == 2, False, h))
        kn = np.where(hn, 0, np.minimum(k + 1, cap))
        w = (np.where(v, hn, h), R, np.where(v, kn, k))
        tj = (w[2] < cap) & v
        t[:, :, j] = tj
        a, o = np.where(tj, aA, aR), np.where(tj, 1.0 - aA, 1.0 - aR)
        B = np.where(v, a * B + o * tj.astype(np.float64), B)
        A = np.where(v, A * a, A)
    flat_h, flat_k = np.broadcast_to(w[0], (T, lanes)), np.broadcast_to(w[2], (T, lanes))
    if n:
        lt, ll = (n - 1) // tile, ((n - 1) % tile) // run
        end_h, end_c = int(flat_h[lt, ll]), int(flat_k[lt, ll])
    At, Bt = _hs_pairs(A, B)
    aggA, aggB = At[:, -1], Bt[:, -1]
    # k_gate_carry (affine)
    env0 = float(state[0])
    cA, cB = np.ones(carry_lanes), np.zeros(carry_lanes)
    cB[0] = env0
    for q in range(busy):
        for r in range(min(q * chunk, T), min(q * chunk + chunk, T)):
            cB[q] = aggA[r] * cB[q] + aggB[r]
            cA[q] = cA[q] * aggA[r]
    _, sB = _hs_pairs(cA, cB)
    ent_env = np.empty(T)
    for q in range(busy):
        u = sB[q - 1] if q else env0
        for r in range(min(q * chunk, T), min(q * chunk + chunk, T)):
            ent_env[r] = u
            u = aggA[r] * u + aggB[r]
    # k_gate_apply: lane 0 starts from the entry, the others from zero; the lanes are joined; every lane runs its frames
    A, B = np.ones((T, lanes)), np.zeros((T, lanes))
    B[:, 0] = ent_env
    for j in range(run):
        v, tj = valid[:, :, j], t[:, :, j] != 0
        a, o = np.where(tj, aA, aR), np.where(tj, 1.0 - aA, 1.0 - aR)
        B = np.where(v, a * B + o * tj.astype(np.float64), B)
        A = np.where(v, A * a, A)
    _, sB = _hs_pairs(A, B)
    env = np.concatenate([ent_env[:, None], sB[:, :-1]], axis=1)
    out = np.empty((T, lanes, run))
    for j in range(run):
        v, tj = valid[:, :, j], t[:, :, j] != 0
        a, o = np.where(tj, aA, aR), np.where(tj, 1.0 - aA, 1.0 - aR)
        env = np.where(v, a * env + o * tj.astype(np.float64), env)
        out[:, :, j] = env
    t, out = t.reshape(-1)[:n], out.reshape(-1)[:n]
    return t, out, ((float(out[-1]) if n else env0), end_h, end_c)
