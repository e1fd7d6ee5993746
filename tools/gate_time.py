"""The gate vertex' launches (k_gate_detect / k_gate_env / k_gate_apply and the two k_gate_carry launches between them,
DESIGN.md §3s) timed on the GPU box: BASELINE config 2's 64 loops summed into a bus, ONE gate vertex on that 60 s /
2 880 512-frame bus in front of the Normalize output, and a batch of 64 such projects (seed offsets 0..63).  Per case and
kernel: the launch's own HIP-event time (the graph's / batch's profiling events, mean per launch over the renders), the bytes
a launch must move -- frames times the bytes per frame below -- and that rate against the repo's measured stream ceiling
(tools/ubench/ceilings.hip td_ubench_stream, as bench.py --full reports).  The yardsticks beside it, in the same run: a
compressor vertex (§3m) in the gate's place on the same project, and §3l's limiter pass (k_master_scan + k_master_carry +
k_master_apply) on the same project's rendered output.

    python tools/gate_time.py            (writes profiles/gate_time.txt)

--key: the keyed forms instead (td_graph_connect_key) -- on the same bus, a gate and a compressor vertex without a
key and the same two keyed by a second loop source (one more sample_loop vertex on the project's first sample, read by
k_gate_detect<true> / k_comp_detect<true> as one more inlined loop term), single projects only, the whole measurement `--rounds`
times over so that the file shows its own run-to-run spread.  Appends to `--out` (default profiles/key_time.txt) under `--label`.
--tree DIR: the termdaw_amd package of another checkout (an earlier commit built beside this one) instead of this tree's, for
the unkeyed rows of that commit in the same file; a package without Graph.connect_key is timed without the keyed rows.

    python tools/gate_time.py --key [--rounds N] [--label TEXT] [--out FILE] [--tree DIR]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_ap = argparse.ArgumentParser()
_ap.add_argument("--key", action="store_true")
_ap.add_argument("--rounds", type=int, default=3)
_ap.add_argument("--label", default="this commit")
_ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "key_time.txt"))
_ap.add_argument("--tree", default=ROOT)
ARGS = _ap.parse_args() if __name__ == "__main__" else _ap.parse_args([])
sys.path.insert(0, os.path.abspath(ARGS.tree))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from termdaw_amd import api, workloads as W  # noqa: E402
from stems_time import stream_gbs  # noqa: E402

KERNELS = ("k_gate_detect", "k_gate_carry_hc", "k_gate_env", "k_gate_carry_env", "k_gate_apply")
COMP = ("k_comp_detect", "k_comp_carry_y1", "k_comp_env", "k_comp_carry_yl", "k_comp_apply")
# bytes per frame: detect reads the bus (8) and writes the summed input (8); env reads it (8) and writes a byte of t per lane of 8
# frames (0.125); apply reads both (8.125) and writes the vertex' frames (8); the carries touch a few words per 2 048-frame tile.
# The compressor's (tools/comp_time.py): 24 / 16 / 24.
BYTES = {"k_gate_detect": 16, "k_gate_carry_hc": 0, "k_gate_env": 8.125, "k_gate_carry_env": 0, "k_gate_apply": 16.125,
         "k_comp_detect": 24, "k_comp_carry_y1": 0, "k_comp_env": 16, "k_comp_carry_yl": 0, "k_comp_apply": 24}
# keyed: detect gathers one more term -- the key loop in its packed 16-bit form, 4 B / frame (8 as f32 frames) -- and the gate's
# also writes a 16-bit class word per lane of 8 frames (0.25); the gate's env reads that word instead of the summed input
KEYED_BYTES = dict(BYTES, k_gate_detect=20.25, k_gate_env=0.375, k_comp_detect=28)
LIMITER = ("k_master_scan", "k_master_carry", "k_master_apply")


def project(seed_offset=0, comp=False, key=False):
    p = W.config2(seed_offset=seed_offset)
    # config 2 connects its loops to the Normalize vertex `sum`: route them through a bus and the gate (or the compressor) instead
    loops = [a for a, b in p.calls["connect"] if b == "sum"]
    p.calls["connect"] = [(a, "bus") for a in loops] + [("bus", "fx"), ("fx", "sum")]
    p.calls["add_sum"].append(("bus", 1.0, 0.0))
    if comp:
        p.calls["add_compressor"].append(("fx", 1.0, 0.0, 1.0, -18.0, 4.0, 5.0, 150.0, 6.0, 3.0))
    else:   # (the bus of 64 full-scale loops sits around -3 dB: a threshold it crosses all the time)
        p.calls["add_gate"].append(("fx", 1.0, 0.0, 1.0, -6.0, 6.0, 10.0, 1.0, 150.0, -40.0))
    if key:   # a second loop source on the project's first sample, 3 dB down: it crosses both thresholds all the time too
        p.calls["add_sampleloop"].append(("keysrc", 0.7, 0.0, p.calls["add_sampleloop"][0][3]))
        p.calls["connect_key"].append(("keysrc", "fx"))
    return p


def timed(target, call, reps):
    for _ in range(3):
        call()
    target.set_profiling(True)
    for _ in range(reps):
        call()
    kt = target.kernel_times()
    target.set_profiling(False)
    return kt


def report(name, kt, frames, reps, ceil, names=KERNELS, BYTES=BYTES):
    total = 0.0
    print("%s: %.1f M frames" % (name, frames / 1e6))
    for k in names:
        ms, n = kt.get(k, (0.0, 0))
        if not n:
            continue
        per = ms / n
        total += ms / reps
        b = BYTES.get(k, 0) * frames
        gbs = b / (per * 1e-3) / 1e9 if per and b else 0.0
        print("    %-16s %8.3f ms x%-2d %8.1f MB  %7.1f GB/s = %.3f of the stream ceiling" % (k, per, n // reps, b / 1e6, gbs, gbs / ceil))
    print("    all of them: %.3f ms of GPU time per render" % total)
    return total


def main():
    if api.device_count() < 1:
        raise SystemExit("gate_time.py needs a GPU")
    ceil = stream_gbs()
    print("stream ceiling (td_ubench_stream, 8 B in + 8 B out per frame): %.1f GB/s" % ceil)
    p = project()
    sb, fb, g = p.build(api)
    frames = p.cs * p.bl

    def one():
        g.reset_normalize_vertices()
        fb.set_time(0)
        g.render_all(sb, fb, p.cs, 16, want_f32=False, want_pcm=False)
    kt = timed(g, one, 20)
    gate = report("one gate vertex on the config-2 bus (60 s)", kt, frames, 20, ceil)
    whole = sum(ms for ms, _ in kt.values()) / 20
    print("    the whole render's launches: %.3f ms (%s)" % (whole, ", ".join("%s %.3f" % (k, v[0] / 20) for k, v in sorted(kt.items()))))
    one()
    kt = timed(g, lambda: g.master(-10.0, -1.0), 20)
    passes = kt.get("k_master_scan", (0.0, 1))[1] // 20
    lim = sum(kt.get(k, (0.0, 0))[0] / max(kt.get(k, (0.0, 1))[1], 1) for k in LIMITER)
    q = project(comp=True)
    qsb, qfb, qg = q.build(api)

    def one_comp():
        qg.reset_normalize_vertices()
        qfb.set_time(0)
        qg.render_all(qsb, qfb, q.cs, 16, want_f32=False, want_pcm=False)
    comp = report("yardstick: one compressor vertex in its place", timed(qg, one_comp, 20), frames, 20, ceil, COMP)
    print("yardstick, the limiter pass of 3l on this project's output (scan + carry + apply, %d pass(es) per call): %.3f ms per pass; "
          "gate / limiter pass = %.2f; gate / compressor = %.2f" % (passes, lim, gate / lim if lim else 0.0, gate / comp if comp else 0.0))
    for name, is_comp, names in (("gate", False, KERNELS), ("compressor", True, COMP)):
        projects = [project(seed_offset=k, comp=is_comp) for k in range(64)]
        built = [x.build(api) for x in projects]
        b = api.Batch()
        for bsb, bfb, bg in built:
            b.add(bsb, bfb, bg)

        def many():
            b.rewind()
            b.render_all(projects[0].cs, 16)
        report("batch of 64 such projects (%s)" % name, timed(b, many, 5), frames * 64, 5, ceil, names)
        del b, built


def main_key():
    """Per round: the four single-project cases, one after the other (so a drift of the machine shows in every case alike)."""
    if api.device_count() < 1:
        raise SystemExit("gate_time.py needs a GPU")
    ceil = stream_gbs()
    keyed_ok = hasattr(api.Graph, "connect_key")
    print("== %s: stream ceiling %.1f GB/s; %d rounds of 20 renders per case" % (ARGS.label, ceil, ARGS.rounds))
    cases = [("gate", False, False, KERNELS), ("compressor", True, False, COMP)]
    if keyed_ok:
        cases += [("keyed gate", False, True, KERNELS), ("keyed compressor", True, True, COMP)]
    built = []
    for name, comp, key, names in cases:
        p = project(comp=comp, key=key)
        built.append((name, key, names, p, p.build(api)))
    totals = {name: [] for name, *_ in cases}
    for r in range(ARGS.rounds):
        for name, key, names, p, (sb, fb, g) in built:
            def one():
                g.reset_normalize_vertices()
                fb.set_time(0)
                g.render_all(sb, fb, p.cs, 16, want_f32=False, want_pcm=False)
            kt = timed(g, one, 20)
            totals[name].append(report("[%s, round %d] one %s vertex on the config-2 bus (60 s)" % (ARGS.label, r, name), kt, p.cs * p.bl, 20, ceil,
                                       names, KEYED_BYTES if key else BYTES))
    for name, v in totals.items():
        print("[%s] %-16s all five launches, per round: %s ms (spread %.3f)" % (ARGS.label, name, " ".join("%.3f" % x for x in v), max(v) - min(v)))


class _Tee:
    def __init__(self, *fs):
        self.fs = fs

    def write(self, s):
        for f in self.fs:
            f.write(s)

    def flush(self):
        for f in self.fs:
            f.flush()


if __name__ == "__main__" and ARGS.key:
    os.makedirs(os.path.dirname(os.path.abspath(ARGS.out)), exist_ok=True)
    with open(ARGS.out, "a") as out:
        sys.stdout = _Tee(sys.__stdout__, out)
        try:
            main_key()
        finally:
            sys.stdout = sys.__stdout__
elif __name__ == "__main__":
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "gate_time.txt"), "w") as out:
        sys.stdout = _Tee(sys.__stdout__, out)
        try:
            main()
        finally:
            sys.stdout = sys.__stdout__
