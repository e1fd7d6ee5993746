"""The reverb vertex' float64 twin (TEST INFRASTRUCTURE): the definition in include/termdaw_amd.h at td_graph_add_reverb restated in
numpy, and an emulation of k_reverb's windowed scan.

* params: g, d1, d2, w1, w2, Hrev, B and the 24 line lengths from the formulas (the layout of api.reverb_params).
* process / reverb, form 0: the serial twin.  The vertex is walked in windows no longer than its shortest line, inside which every
  delayed read is history; the combs' one-pole runs frame by frame in the definition's order (a Python loop over the frames,
  vectorised over the 16 combs only), everything else is elementwise over the window in the definition's order -- numpy contracts
  nothing into an FMA and nothing is re-associated, which is what lets the device tests ask form 0 for equal bits.  The window
  length does not enter the result.
* form 1: the scan of k_reverb<1> for a window length B of BLOCKS, restated operation by operation: windows of B frames from the
  chunk's start, a lane-local pass over B / 64 frames from 0 (lane 0 from the carried f), a Hillis-Steele scan over the 64 lanes
  with the powers d1^((B / 64) 2^k) (squared in long double, rounded once), and the lane-local pass again from the scanned carry.
* The state is what the engine keeps: 24 circular lines (frame m of a line in slot m mod D), the 16 one-pole values and the frames
  run since the restart; None is the silent state."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from np_twin import pan_gain  # noqa: E402

COMBS = (1116, 1188, 1277, 1356, 1422, 1491, 1557, 1617)
ALLPASS = (556, 441, 341, 225)
SPREAD = 23
BLOCKS = (64, 128, 256)   # the candidate window lengths ("debug.reverb_block" caps B)


def _llround(v):
    return int(np.floor(abs(v) + 0.5)) * (1 if v >= 0 else -1)


def hrev(g):
    """The guard's bound: input mix 0.015 x 2, comb bank 8 / (1 - g), four all-passes at 5/3 each, output mix 1."""
    ap = 5.0 / 3.0
    return (0.015 * 2.0) * (8.0 / (1.0 - g)) * ((ap * ap) * (ap * ap))


def params(sr, room, damp, width, size):
    """The dict api.reverb_params returns, in float64 from the float32 parameters widened."""
    room, damp, width, size = (float(np.float32(v)) for v in (room, damp, width, size))
    g = 0.7 + 0.28 * room
    d1 = 0.4 * damp

    def frames(tuning):
        return _llround(float(tuning) * size * float(sr) / 44100.0)
    k = {"g": g, "d1": d1, "d2": 1.0 - d1, "w1": (1.0 + width) / 2.0, "w2": (1.0 - width) / 2.0, "Hrev": hrev(g),
         "combs_l": [frames(t) for t in COMBS], "combs_r": [frames(t + SPREAD) for t in COMBS],
         "allpass_l": [frames(t) for t in ALLPASS], "allpass_r": [frames(t + SPREAD) for t in ALLPASS]}
    k["B"] = window(k)
    return k


def lengths(k):
    return list(k["combs_l"]) + list(k["combs_r"]) + list(k["allpass_l"]) + list(k["allpass_r"])


def window(k, cap=256):
    """The largest of 64, 128 and 256 that exceeds neither the shortest line nor cap."""
    s = min(lengths(k))
    return min(256 if s >= 256 else 128 if s >= 128 else 64, cap)


def powers(d1, q):
    """d1^(q 2^k), k = 0 .. 5, squared in long double and rounded once."""
    p = np.longdouble(1.0)
    for _ in range(q):
        p = p * np.longdouble(d1)
    out = []
    for _ in range(6):
        out.append(float(p))
        p = p * p
    return out


def new_state(k):
    return {"lines": [np.zeros(D) for D in lengths(k)], "f": np.zeros(16), "total": 0}


def _serial(Wm, f, d1, d2):
    Wd = Wm * d2
    F = np.empty_like(Wm)
    f = f.copy()
    for n in range(Wm.shape[1]):
        f = Wd[:, n] + f * d1
        F[:, n] = f
    return F


def _scan(Wm, f, d1, d2, B, pw):
    q = B // 64
    bw = Wm.shape[1]
    w = np.zeros((16, B))
    w[:, :bw] = Wm
    w = w.reshape(16, 64, q)
    t = np.zeros((16, 64))
    t[:, 0] = f
    for i in range(q):
        t = w[:, :, i] * d2 + t * d1
    for kk in range(6):
        s = 1 << kk
        u = t[:, :64 - s].copy()
        t[:, s:] = t[:, s:] + pw[kk] * u
    c = np.empty((16, 64))
    c[:, 1:] = t[:, :63]
    c[:, 0] = f
    F = np.empty((16, 64, q))
    for i in range(q):
        c = w[:, :, i] * d2 + c * d1
        F[:, :, i] = c
    return F.reshape(16, B)[:, :bw]


def process(x, k, state=None, form=0, B=None, raw=False, tap=None):
    """(p, state): the processed signal -- float32 (frames, 2), or float64 before that rounding with raw -- and the new state.  k:
    the constants (params(), or the engine's).  form 1 takes the window length B; x is one chunk, the windows start at its first
    frame.  tap: a dict that receives "S", the comb banks' sums (frames, 2)."""
    x = np.asarray(x, np.float32).reshape(-1, 2)
    n = len(x)
    lens = lengths(k)
    st = new_state(k) if state is None else {"lines": [a.copy() for a in state["lines"]], "f": state["f"].copy(), "total": state["total"]}
    lines, f, total = st["lines"], st["f"], st["total"]
    g, d1, d2 = k["g"], k["d1"], k["d2"]
    xs = np.where(np.isfinite(x), x, np.float32(0.0)).astype(np.float64)
    inn = (xs[:, 0] + xs[:, 1]) * 0.015
    Wn = min(lens) if form == 0 else int(B)
    assert Wn <= min(lens)
    pw = powers(d1, Wn // 64) if form else None
    A = np.empty((n, 2))
    S = np.empty((n, 2))
    for n0 in range(0, n, Wn):
        bw = min(Wn, n - n0)
        m = total + n0 + np.arange(bw, dtype=np.int64)
        idx = [m % D for D in lens]
        Wm = np.stack([lines[i][idx[i]] for i in range(16)])
        F = _serial(Wm, f, d1, d2) if form == 0 else _scan(Wm, f, d1, d2, Wn, pw)
        f = F[:, bw - 1].copy()
        for i in range(16):
            lines[i][idx[i]] = inn[n0:n0 + bw] + F[i] * g
        for ch in range(2):
            s = np.zeros(bw)
            for c in range(8):
                s = s + Wm[ch * 8 + c]
            S[n0:n0 + bw, ch] = s
            for a in range(4):
                li = 16 + ch * 4 + a
                v = lines[li][idx[li]]
                y = v - s
                lines[li][idx[li]] = s + v * 0.5
                s = y
            A[n0:n0 + bw, ch] = s
    if tap is not None:
        tap["S"] = S
    p = np.stack([A[:, 0] * k["w1"] + A[:, 1] * k["w2"], A[:, 1] * k["w1"] + A[:, 0] * k["w2"]], axis=1)
    st["f"], st["total"] = f, total + n
    return (p if raw else p.astype(np.float32)), st


def reverb(x, k, wet=1.0, gain=1.0, angle=0.0, state=None, form=0, B=None):
    """The vertex: (out float32 (frames, 2), state)."""
    x = np.asarray(x, np.float32).reshape(-1, 2)
    wet = np.float32(min(max(float(np.float32(wet)), 0.0), 1.0))
    if wet < np.float32(0.0001):   # (the engine's test, in f32: 0.0001f itself is processed)
        l, r = pan_gain(x[:, 0].copy(), x[:, 1].copy(), gain, angle)
        return np.stack([l, r], axis=1).astype(np.float32), state
    p, end = process(x, k, state, form, B)
    with np.errstate(invalid="ignore", over="ignore"):
        out = x + wet * (p - x)   # float32 throughout: the reference's lerp (adsr.rs:42)
        l, r = pan_gain(out[:, 0], out[:, 1], gain, angle)
    return np.stack([l, r], axis=1).astype(np.float32), end
