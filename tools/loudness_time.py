"""The loudness launch (k_loudness) timed on the GPU box: BASELINE config 2's 60 s output, config 3's output
plus 4 stems (front-end defaults: band_mode 2, sine_mode 2), and a batch of 64 config-2 projects.  Per case: the k_loudness
launch's own HIP-event time (the graph's / batch's profiling events around the launch, mean over the calls), the PCM bytes it
measures, and that rate against the repo's measured stream ceiling (tools/ubench/ceilings.hip td_ubench_stream: 8 B in + 8 B
out per frame, the figure bench.py --full reports).  The kernel reads more than the PCM: each tile's warm-up frames again,
both passes of the recurrence and the true-peak window go through the caches -- the rate shows how far the launch is from
being bound by the bytes it must read.

    python tools/loudness_time.py            (profiles/loudness_time.txt holds a run)"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from termdaw_amd import api, workloads as W  # noqa: E402
from stems_time import stream_gbs  # noqa: E402


def timed(target, measure, reps):
    for _ in range(3):
        measure()
    target.set_profiling(True)
    for _ in range(reps):
        rows = measure()
    ms, n = target.kernel_times().get("k_loudness", (0.0, 0))
    target.set_profiling(False)
    return (ms / n if n else 0.0), n // reps, rows


def graph_case(name, p, stems=(), opts=(), reps=50):
    sb, fb, g = p.build(api)
    for k, v in opts:
        g.set_option(k, v)
    if stems:
        g.set_stems(list(stems))
    g.render_all(sb, fb, p.cs, 16, want_f32=False)
    ms, per, rows = timed(g, lambda: g.loudness(), reps)
    return {"case": name, "ms": ms, "launches": per, "signals": len(rows), "bytes": 4 * sum(r["frames"] for r in rows), "rows": rows}


def batch_case(name, n, reps=20):
    projects = [W.config2(seed_offset=k) for k in range(n)]
    built = [p.build(api) for p in projects]
    b = api.Batch()
    for sb, fb, g in built:
        b.add(sb, fb, g)
    b.render_all(projects[0].cs, 16)
    ms, per, rows = timed(b, lambda: b.loudness(), reps)
    return {"case": name, "ms": ms, "launches": per, "signals": len(rows), "bytes": 4 * sum(r["frames"] for r in rows), "rows": rows}


def main():
    if api.device_count() < 1:
        raise SystemExit("loudness_time.py needs a GPU")
    ceil = stream_gbs()
    rows = [graph_case("config2 output", W.config2()),
            graph_case("config3 + 4 stems", W.config3(), stems=("syn", "env", "band", "sum"), opts=(("band_mode", 2), ("sine_mode", 2))),
            batch_case("batch 64 x config2", 64)]
    print("stream ceiling (td_ubench_stream, 8 B in + 8 B out per frame): %.1f GB/s" % ceil)
    for r in rows:
        gbs = r["bytes"] / (r["ms"] * 1e-3) / 1e9 if r["ms"] else 0.0
        print("%-20s k_loudness %7.3f ms x%d  %3d signals  %7.1f MB PCM  %7.1f GB/s = %.3f of the stream ceiling"
              % (r["case"], r["ms"], r["launches"], r["signals"], r["bytes"] / 1e6, gbs, gbs / ceil))
        f = r["rows"][0]
        print("    first signal: I %.2f LUFS  LRA %.2f LU  M max %.2f  S max %.2f  %.2f dBTP  %.2f dBFS  (%d frames)"
              % (f["integrated"], f["lra"], f["momentary_max"], f["short_term_max"], f["true_peak"], f["sample_peak"], f["frames"]))


if __name__ == "__main__":
    main()
