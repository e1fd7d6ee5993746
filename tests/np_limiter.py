"""The limiter vertex (td_graph_add_limiter) in numpy (TEST INFRASTRUCTURE): the float64 serial twin of the
definition in include/termdaw_amd.h -- `serial`, `process` -- and `blocked`, the kernels' tile geometry, halo and prefix-sum
order restated (kernels.h LimDesc: tiles of 2 048 frames, 8 frames per lane, 256 lanes).

consts = (c, gin, L, a, latency) as td_limiter_params / api.limiter_params return them.  A state is (u, xh, eh): u at the last
frame, the last L - 1 raw input frames (float32 (L - 1, 2)) and the last L - 1 values of e (float64), oldest first -- what the
engine's carried line holds.  `start(L)` is the state at the restart: u = 0, and the frames before it count as x = 0, e = 1.

Steps 1 and 2 are exact in any order (a maximum of f32 values).  Every e = fl(1 - u) with u in [0, 1) is an integer multiple of
2^-53, so the serial twin sums a window of e EXACTLY, in 64-bit integers (a window holds at most 2 048 values of at most 2^53),
and rounds the mean once from an 80-bit quotient: the same G whatever the cuts, G = 1 exactly on an idle input, G = e at L = 1."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from np_filter import LANES, RUN, _lane_scan, _master_carry, _run_fold  # noqa: E402  (comp_lane_scan / k_master_carry, emulated)
from np_twin import pan_gain  # noqa: E402  (sample.rs:97-114 in float32, as the engine's make_pg)

TILE = RUN * LANES
assert TILE == 2048
assert np.finfo(np.longdouble).nmant >= 63   # (window_mean: an 80-bit quotient)
_TWO53 = 2.0 ** 53


def start(L):
    return 0.0, np.zeros((L - 1, 2), np.float32), np.ones(L - 1)


def level(x):
    """Step 1: s = max(|l|, |r|) as f32; a frame with a NaN or an infinite sample has s = 0."""
    a = np.abs(np.asarray(x, np.float32))
    s = np.maximum(a[:, 0], a[:, 1])
    return np.where(np.isfinite(a).all(axis=1), s, np.float32(0.0)).astype(np.float32)


def window_max(s_ext, L):
    """Step 2: s_ext holds s from L - 1 frames before the first frame on; Q[j] = max s_ext[j .. j + L - 1], by doubling."""
    n = len(s_ext) - (L - 1)
    r = s_ext.copy()
    k2 = 0
    while (2 << k2) <= L:
        k2 += 1
    for j in range(k2):
        s = 1 << j
        r[:-s] = np.maximum(r[:-s], r[s:])
    sh = L - (1 << k2)
    return np.maximum(r[:n], r[sh:sh + n])


def one_minus_h(Q, c, gin):
    """Steps 3 and 4's 1 - h."""
    d = gin * Q.astype(np.float64)
    over = d > c
    return np.where(over, 1.0 - c / np.where(over, d, 1.0), 0.0)


def release(omh, a, u):
    """Step 4, serially: u[n] = max(1 - h[n], a u[n-1])."""
    out = [0.0] * len(omh)
    for i, w in enumerate(omh.tolist()):
        t = a * u
        u = w if w > t else t
        out[i] = u
    return np.array(out, np.float64)


def window_mean(e_ext, L):
    """Step 5, exactly summed: e_ext holds e from L - 1 frames before the first frame on."""
    k = e_ext * _TWO53
    assert np.array_equal(k, np.floor(k)) and (k >= 0).all() and (k <= _TWO53).all()
    k = k.astype(np.uint64)

    def windows(v):   # (modulo 2^64: a window's sum of 32-bit halves is far below that)
        cs = np.concatenate([np.zeros(1, np.uint64), np.cumsum(v, dtype=np.uint64)])
        return (cs[L:] - cs[:-L]).astype(np.longdouble)

    # the window's sum in an 80-bit float, exact: at most 2 048 x 2^53 = 2^64, and that only when every e is 1
    w = windows(k >> np.uint64(32)) * np.longdouble(2.0 ** 32) + windows(k & np.uint64(0xFFFFFFFF))
    return ((w / np.longdouble(L)).astype(np.float64)) * 2.0 ** -53


def _front(x, consts, state):
    c, gin, L, a = float(consts[0]), float(consts[1]), int(consts[2]), float(consts[3])
    x = np.asarray(x, np.float32).reshape(-1, 2)
    u0, xh, eh = start(L) if state is None else state
    assert xh.shape == (L - 1, 2) and eh.shape == (L - 1,)
    x_ext = np.concatenate([np.asarray(xh, np.float32), x])
    omh = one_minus_h(window_max(level(x_ext), L), c, gin)
    return c, gin, L, a, x, float(u0), x_ext, np.asarray(eh, np.float64), omh


def _back(x, x_ext, e, eh, gin, L, G, u_end):
    n = len(x)
    xd = x_ext[:n]
    with np.errstate(invalid="ignore", over="ignore"):
        p64 = (xd.astype(np.float64) * gin) * G[:, None]
        p = p64.astype(np.float32)
    e_ext = np.concatenate([eh, e])
    H = L - 1
    end = (u_end, x_ext[len(x_ext) - H:].copy(), e_ext[len(e_ext) - H:].copy())
    return p, xd, G, end, p64


def serial(x, consts, state=None):
    """The definition, frame by frame.  Returns (p float32 (n, 2), xd, G, end state, p in float64 before its rounding)."""
    c, gin, L, a, x, u0, x_ext, eh, omh = _front(x, consts, state)
    u = release(omh, a, u0)
    e = 1.0 - u
    G = window_mean(np.concatenate([eh, e]), L)
    return _back(x, x_ext, e, eh, gin, L, G, float(u[-1]) if len(u) else u0)


def trace(x, consts, state=None):
    """(1 - h, u, G) of the serial twin, per frame: what the tests read to show that a grid is not vacuous."""
    c, gin, L, a, x, u0, x_ext, eh, omh = _front(x, consts, state)
    u = release(omh, a, u0)
    return omh, u, window_mean(np.concatenate([eh, 1.0 - u]), L)


def process(x, consts, wet=1.0, gain=1.0, angle=0.0, state=None, processed=False):
    """The serial twin.  Returns (out float32 (frames, 2), end state); processed=True: p of step 6 instead of the mix, pan and
    gain.  A dry vertex hands its input on undelayed and keeps its state."""
    x = np.asarray(x, np.float32)
    L = int(consts[2])
    state = start(L) if state is None else state
    wet = np.float32(min(max(float(np.float32(wet)), 0.0), 1.0))
    if wet < np.float32(0.0001) and not processed:   # (0.0001f itself is processed)
        l, r = pan_gain(x[:, 0].copy(), x[:, 1].copy(), gain, angle)
        return np.stack([l, r], axis=1).astype(np.float32), state
    p, xd, G, end, _ = serial(x, consts, state)
    if processed:
        return p, end
    with np.errstate(invalid="ignore", over="ignore"):
        out = xd + wet * (p - xd)   # float32 throughout: the reference's lerp (adsr.rs:42)
        l, r = pan_gain(out[:, 0], out[:, 1], gain, angle)
    return np.stack([l, r], axis=1).astype(np.float32), end


# ---- the device's order, emulated: one call is one chunk ----
def _prefix(e, running):
    """lim_prefix: e (T, LANES, RUN) -> PS (T, LANES, RUN) behind `running` (T,), and the new running."""
    ps = np.empty_like(e)
    acc = np.zeros(e.shape[:2])
    for k in range(RUN):
        acc = acc + e[..., k]
        ps[..., k] = acc
    v = acc
    off = 1
    while off < LANES:
        w = v.copy()
        w[:, off:] = v[:, :-off] + v[:, off:]
        v = w
        off <<= 1
    before = running[:, None] + np.concatenate([np.zeros((len(v), 1)), v[:, :-1]], axis=1)
    return before[..., None] + ps, running + v[:, -1]


def blocked(x, consts, state=None):
    """The chunk as k_lim_detect / k_master_carry / k_lim_apply run it (a chunk of one tile: the same steps inside k_lim_apply):
    the release by lane runs joined with the host's powers, G as differences of prefix sums taken per tile over the tile before
    (the chunk's first tile: the line's e) and the tile itself.  Returns what `serial` returns."""
    c, gin, L, a, x, u0, x_ext, eh, omh = _front(x, consts, state)
    n, H = len(x), L - 1
    T = max(1, (n + TILE - 1) // TILE)
    y = np.zeros(T * TILE)
    y[:n] = omh
    y = y.reshape(T, LANES, RUN)
    pw = [math.pow(a, float(RUN) * float(1 << k)) for k in range(8)]
    zero = np.zeros((T, LANES))
    agg = _lane_scan(_run_fold(y, a, None, zero, False)[1], pw, False)[:, -1]
    carry = _master_carry(agg, a, u0, False, TILE) if T > 1 else np.array([u0])
    u = zero.copy()
    u[:, 0] = carry
    u = _lane_scan(_run_fold(y, a, None, u, False)[1], pw, False)
    uin = np.concatenate([carry[:, None], u[:, :-1]], axis=1)
    uv = _run_fold(y, a, None, uin, False)[0].reshape(T, TILE)
    ev = 1.0 - uv
    # round A: the tile before (tile 0: the line's e), only the frames behind s0 = t0 - L; round B: the tile itself
    running = np.zeros(T)
    psa = np.zeros((T, TILE))
    if H:
        ea = np.zeros((T, TILE))
        ea[1:, TILE - H:] = ev[:-1, TILE - H:]
        ea[0, TILE - H:] = eh
        pa, running = _prefix(ea.reshape(T, LANES, RUN), running)
        psa = pa.reshape(T, TILE)
    psb = _prefix(ev.reshape(T, LANES, RUN), running)[0].reshape(T, TILE)
    i = np.arange(TILE)
    back = np.where(i[None, :] < L, psa[:, (TILE - L + i) % TILE], psb[:, np.maximum(i - L, 0)])
    back[:, 0] = 0.0
    G = np.maximum(0.0, (psb - back) / float(L)).reshape(-1)[:n]
    e = ev.reshape(-1)[:n]
    return _back(x, x_ext, e, eh, gin, L, G, float(uv.reshape(-1)[n - 1]) if n else u0)
