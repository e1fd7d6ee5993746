"""The convolution vertex in numpy (TEST INFRASTRUCTURE; the definition is in include/termdaw_amd.h at td_graph_add_convolution).

* direct / process: the twin -- the definition as a direct sum in float64 on the float32 input, split anywhere through a state
  (the last D + Lh - 1 input frames).
* direct_ld: the same sum in long double, unrounded: what emulate() and the twin are measured against.
* emulate: the kernels' own arithmetic (termdaw_amd/csrc/kernels.hip k_conv_ir / k_conv_fwd / k_conv_mac / k_conv_inv) restated:
  the same partition B, the same radix-2 schedule (forward decimation in frequency, inverse decimation in time), the same
  twiddle table (api.convolution_twiddles()), both channels in one transform as l + i r, the products summed over the
  partitions p = 0 .. P - 1 in ascending order, every complex product as (ac - bd, ad + bc) without contraction.  Unrounded
  float64 out.
* sparse: a response of a few taps as delayed copies (the grid's response at the cap)."""
import numpy as np

B = 1024
N = 2 * B
BINS = N // 2 + 1


def clean(x):
    """The input as the wet path sees it: a NaN or infinite sample enters as 0."""
    x = np.asarray(x, np.float32)
    return np.where(np.isfinite(x), x, np.float32(0.0)).astype(np.float64)


def scale(h, g, norm):
    """g, divided by sqrt(max_c sum_k h_c[k]^2) when norm."""
    if not norm:
        return float(g)
    e = (h.astype(np.float64) ** 2).sum(axis=0).max()
    return float(g) / float(np.sqrt(e))


def direct64(x, h, D, g, state=None):
    """p before its rounding, float64 [n, 2]: g sum_k h_c[k] x_c[n - D - k], and the state behind the piece.  state: the last
    D + Lh - 1 input frames (raw float32), None: silence."""
    x = np.asarray(x, np.float32)
    h = np.asarray(h, np.float32)
    n, Lh = len(x), len(h)
    H = D + Lh - 1
    if state is None:
        state = np.zeros((H, 2), np.float32)
    assert state.shape == (H, 2)
    full = np.concatenate([state, x])
    xc = clean(full)
    out = np.empty((n, 2), np.float64)
    for c in range(2):
        y = np.convolve(xc[:, c], h[:, c].astype(np.float64))   # y[m] = sum_k h[k] full[m - k]
        out[:, c] = g * y[H - D:H - D + n]                       # chunk frame i is full[H + i]; the tap at D + k reads full[H + i - D - k]
    return out, full[len(full) - H:].copy()


def direct(x, h, D, g, state=None):
    """(p float32, xd = x, end state): the twin."""
    p64, st = direct64(x, h, D, g, state)
    return p64.astype(np.float32), np.asarray(x, np.float32), st


def direct_ld(x, h, D, g):
    """The direct sum in long double from silence, unrounded [n, 2]."""
    xc = clean(x).astype(np.longdouble)
    h = np.asarray(h, np.float32).astype(np.longdouble)
    n = len(xc)
    out = np.zeros((n, 2), np.longdouble)
    for c in range(2):
        y = np.convolve(xc[:, c], h[:, c])[:n]
        out[D:, c] = np.longdouble(g) * y[:n - D] if D < n else 0
    return out


def sparse64(x, taps, D, g, dtype=np.float64):
    """A response that is zero but for taps = [(k, (hl, hr)), ...] (float32 values), as delayed copies summed in ascending k."""
    xc = clean(x).astype(dtype)
    n = len(xc)
    out = np.zeros((n, 2), dtype)
    for k, hv in sorted(taps):
        d = D + k
        if d < n:
            out[d:] += np.asarray(hv, np.float32).astype(dtype)[None, :] * xc[:n - d]
    return dtype(g) * out


def process(x, h, D, g, wet=1.0, gain=1.0, angle=0.0, state=None):
    """What the vertex hands on, by the twin: (out float32, end state)."""
    from np_twin import pan_gain
    p, xd, st = direct(x, h, D, g, state)
    w = np.float32(min(max(wet, 0.0), 1.0))
    o = xd + w * (p - xd)
    l, r = pan_gain(o[:, 0].copy(), o[:, 1].copy(), gain, angle)
    return np.stack([l, r], axis=1), st


# ---- the kernels' arithmetic ----
def _cmul(a, b):
    return (a.real * b.real - a.imag * b.imag) + 1j * (a.real * b.imag + a.imag * b.real)


def fft_fwd(z, tw):
    """Forward, decimation in frequency, natural order in, bit-reversed out; z: [..., N] complex128 (a copy is transformed)."""
    z = z.copy()
    b = np.arange(N // 2)
    half, sh = N // 2, 0
    while half >= 1:
        pos = b & (half - 1)
        i0 = ((b - pos) << 1) + pos
        i1 = i0 + half
        u, v = z[..., i0], z[..., i1]
        w = tw[pos << sh]
        z[..., i0] = (u.real + v.real) + 1j * (u.imag + v.imag)
        z[..., i1] = _cmul((u.real - v.real) + 1j * (u.imag - v.imag), w)
        half >>= 1
        sh += 1
    return z


def fft_inv(z, tw):
    """Inverse (unscaled), decimation in time, bit-reversed in, natural order out."""
    z = z.copy()
    b = np.arange(N // 2)
    half, sh = 1, 10
    twc = np.conj(tw)
    while half <= N // 2:
        pos = b & (half - 1)
        i0 = ((b - pos) << 1) + pos
        i1 = i0 + half
        u = z[..., i0]
        v = _cmul(z[..., i1], twc[pos << sh])
        z[..., i0] = (u.real + v.real) + 1j * (u.imag + v.imag)
        z[..., i1] = (u.real - v.real) + 1j * (u.imag - v.imag)
        half <<= 1
        sh -= 1
    return z


REV = np.array([int(format(i, "011b")[::-1], 2) for i in range(N)])


def spectra(h, D, g_eff, tw):
    """(A, C) [P, BINS] of the effective response: D zeros, then g_eff h."""
    h = np.asarray(h, np.float32).astype(np.float64)
    Lh = len(h)
    P = -(-(D + Lh) // B)
    eff = np.zeros((P * B, 2))
    eff[D:D + Lh] = g_eff * h
    z = np.zeros((P, N), np.complex128)
    z[:, :B] = (eff[:, 0] + 1j * eff[:, 1]).reshape(P, B)
    Z = fft_fwd(z, tw)[:, REV]            # natural order
    k = np.arange(BINS)
    a, bq = Z[:, k], Z[:, (N - k) % N]
    lx, ly = 0.5 * (a.real + bq.real), 0.5 * (a.imag - bq.imag)
    rx, ry = 0.5 * (a.imag + bq.imag), -0.5 * (a.real - bq.real)
    return (0.5 * (lx + rx)) + 1j * (0.5 * (ly + ry)), (0.5 * (lx - rx)) + 1j * (0.5 * (ly - ry))


def emulate(x, h, D, g, norm, tw, state=None, spec=None):
    """One chunk as the kernels compute it: (p float64 [n, 2] unrounded, end state)."""
    x = np.asarray(x, np.float32)
    n, Lh = len(x), len(h)
    H = D + Lh - 1
    if spec is None:
        spec = spectra(h, D, scale(np.asarray(h, np.float32), g, norm), tw)
    A, C = spec
    P = A.shape[0]
    T = -(-n // B)
    if state is None:
        state = np.zeros((H, 2), np.float32)
    # windows w = 0 .. T + P - 2 cover chunk frames [(w - P) B, (w - P + 2) B)
    pad = np.zeros(((P + 1) * B + T * B, 2))
    hist = clean(state)
    pad[P * B - H:P * B] = hist
    pad[P * B:P * B + n] = clean(x)
    zc = pad[:, 0] + 1j * pad[:, 1]
    W = T + P - 1
    idx = (np.arange(W) * B)[:, None] + np.arange(N)[None, :]
    X = fft_fwd(zc[idx], tw)[:, REV]      # [W, N], natural order
    k = np.arange(BINS)
    kn = (N - k) % N
    Xk, Xn = X[:, k], X[:, kn]
    Yk = np.zeros((T, BINS), np.complex128)
    Yn = np.zeros((T, BINS), np.complex128)
    t = np.arange(T)
    for p in range(P):
        a, b = Xk[t - p + P - 1], Xn[t - p + P - 1]
        u, v = _cmul(a, A[p][None, :]), _cmul(np.conj(b), C[p][None, :])
        Yk = ((Yk.real + u.real) + v.real) + 1j * ((Yk.imag + u.imag) + v.imag)
        un, vn = _cmul(b, np.conj(A[p])[None, :]), _cmul(np.conj(a), np.conj(C[p])[None, :])
        Yn = ((Yn.real + un.real) + vn.real) + 1j * ((Yn.imag + un.imag) + vn.imag)
    Y = np.zeros((T, N), np.complex128)
    Y[:, kn] = Yn
    Y[:, k] = Yk                          # (bins 0 and N / 2: the k form, as the kernel stores it)
    y = fft_inv(Y[:, REV], tw)[:, B:] * (1.0 / N)
    y = y.reshape(-1)[:n]
    full = np.concatenate([state, x])
    return np.stack([y.real, y.imag], axis=1), full[len(full) - H:].copy()
