"""The convolution vertex' launches (k_conv_fwd / k_conv_mac / k_conv_inv) timed on the GPU box: BASELINE config
2's 64 loops summed into a bus, ONE convolution vertex on that 60 s / 2 880 512-frame, 48 kHz bus in front of the Normalize
output, with responses of 0.1 s, 1 s and 5.46 s (262 144 frames, the cap).  Per case and kernel: the launch's own HIP-event time
(the graph's profiling events, mean per launch over the renders; k_conv_ir runs in the first render only and is listed from
that one).  For k_conv_mac the achieved bytes / s and f64 operations / s against §3z's roofline: per output frame and partition
16 B (an (A, C) pair and one window's bin pair per 2 x 4 products: 1 025 x 64 B per 4 096 frames) and 32 f64 operations
(1 025 x 4 complex multiply-adds of 8 per 1 024 frames); the bytes against the repo's measured stream ceiling
(tools/ubench/ceilings.hip td_ubench_stream), the operations against the 78.6 Tflop/s the MI355X's data sheet gives for vector
f64.  The yardstick beside it, in the same run: a reverb vertex (§3r) in the convolution's place on the same project.

    python tools/conv_time.py            (writes profiles/conv_time.txt)"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from termdaw_amd import api, workloads as W  # noqa: E402
from gate_time import _Tee, timed  # noqa: E402
from stems_time import stream_gbs  # noqa: E402

KERNELS = ("k_conv_ir", "k_conv_fwd", "k_conv_mac", "k_conv_inv")
REVERB = ("k_reverb_sum", "k_reverb")
F64_PEAK = 78.6e12
B = 1024


def response(n, seed=5):
    rng = np.random.default_rng(seed)
    h = rng.uniform(-1.0, 1.0, (n, 2)) * np.exp(-6.9 * np.arange(n) / n)[:, None]
    h[0] = 1.0
    return np.round(h * 32767.0).astype(np.int16)


def project(ir_frames=0, reverb=False):
    p = W.config2()
    # config 2 connects its loops to the Normalize vertex `sum`: route them through a bus and the vertex instead
    loops = [a for a, b in p.calls["connect"] if b == "sum"]
    p.calls["connect"] = [(a, "bus") for a in loops] + [("bus", "fx"), ("fx", "sum")]
    p.calls["add_sum"].append(("bus", 1.0, 0.0))
    if reverb:
        p.calls["add_reverb"].append(("fx", 1.0, 0.0, 0.35, 0.84, 0.2, 1.0, 1.0))
    else:
        p.assets["ir"] = W.Asset(response(ir_frames), sr=p.psr)
        p.calls["load_sample"].append(("ir", "ir", ""))
        p.calls["add_convolution"].append(("fx", 1.0, 0.0, 0.35, "ir", 0.0, 0.0, -6.0, 1))
    return p


def single(p, reps):
    sb, fb, g = p.build(api)

    def one():
        g.reset_normalize_vertices()
        fb.set_time(0)
        g.set_time(0)
        g.render_all(sb, fb, p.cs, 16, want_f32=False, want_pcm=False)
    g.set_profiling(True)         # (the graph's first render: the one that builds the spectra)
    one()
    first = g.kernel_times()
    g.set_profiling(False)
    return first, timed(g, one, reps)


def report(name, kt, first, frames, reps, ceil, P=0, names=KERNELS):
    total = 0.0
    print("%s: %.1f M frames" % (name, frames / 1e6))
    for k in names:
        ms, n = kt.get(k, (0.0, 0))
        if not n and first and k in first:
            print("    %-12s %9.3f ms, in the first render only" % (k, first[k][0] / max(first[k][1], 1)))
            continue
        if not n:
            continue
        per = ms / n
        total += ms / reps
        line = "    %-12s %9.3f ms x%-2d" % (k, per, n // reps)
        if k == "k_conv_mac" and P:
            by, ops = 16.0 * P * frames, 32.0 * P * frames
            gbs, tf = by / (per * 1e-3) / 1e9, ops / (per * 1e-3) / 1e12
            roof_ms = max(by / (ceil * 1e9), ops / F64_PEAK) * 1e3
            line += "  %8.1f MB %7.1f GB/s = %.3f of the stream ceiling; %6.2f Tflop/s f64 = %.3f of the peak; roofline %.3f ms, achieved %.3f of it" % (
                by / 1e6, gbs, gbs / ceil, tf, tf * 1e12 / F64_PEAK, roof_ms, roof_ms / per)
        print(line)
    print("    all of them: %.3f ms of GPU time per render" % total)
    return total


def main():
    if api.device_count() < 1:
        raise SystemExit("conv_time.py needs a GPU")
    ceil = stream_gbs()
    print("stream ceiling (td_ubench_stream, 8 B in + 8 B out per frame): %.1f GB/s" % ceil)
    totals = {}
    for seconds, n in ((0.1, 4800), (1.0, 48000), (5.46, 262144)):
        p = project(n)
        frames = p.cs * p.bl
        P = api.convolution_params(p.psr, n, 0.0, 0.0, -6.0, 1)[3]
        reps = 10 if n < 100000 else 3
        first, kt = single(p, reps)
        totals[n] = report("one convolution vertex on the config-2 bus (60 s, 48 kHz), response %.2f s = %d frames, %d partitions" % (seconds, n, P),
                           kt, first, frames, reps, ceil, P)
    p = project(reverb=True)
    first, kt = single(p, 10)
    rev = report("yardstick: one reverb vertex in its place", kt, None, p.cs * p.bl, 10, ceil, names=REVERB)
    print("convolution / reverb = " + ", ".join("%.2f at %d frames" % (t / rev if rev else 0.0, n) for n, t in totals.items()))


if __name__ == "__main__":
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "conv_time.txt"), "w") as out:
        sys.stdout = _Tee(sys.__stdout__, out)
        try:
            main()
        finally:
            sys.stdout = sys.__stdout__
