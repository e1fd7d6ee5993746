"""The mastering launches (k_master_*) timed on the GPU box: BASELINE config 2's 60 s output mastered under
-1 dBTP to -14 LUFS (gain only, the limiter idle), -10 LUFS (the limiter engaged) and -8 LUFS (louder than the input: more
passes), and a batch of 64 config-2 projects (seed offsets 0..63) mastered to -14 and to -10 LUFS.  Each case prints the
passes its signals took.  Per case and kernel: the launch's own HIP-event time (the graph's / batch's profiling events, mean
per launch over the calls), launches per call, the bytes a launch must move -- the frames of the signals IN that launch (a
signal that is done drops out of later passes) times the bytes per frame (int16 words, the f32 held detector; the meter's PCM
read for k_loudness) -- and that rate against the repo's measured stream ceiling (tools/ubench/ceilings.hip td_ubench_stream,
as bench.py --full reports).  The sum of the launches' times is the GPU time of one whole call.

    python tools/master_time.py            (profiles/master_time.txt holds a run)"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from termdaw_amd import api, workloads as W  # noqa: E402
from stems_time import stream_gbs  # noqa: E402

KERNELS = ("k_master_detect", "k_master_scan", "k_master_carry", "k_master_apply", "k_loudness")


def per_frame_bytes(name):
    """Bytes one launch must move per frame of an int16 signal: words 4 B, the held detector q 4 B (f32)."""
    return {"k_master_detect": 4 + 4, "k_master_scan": 4, "k_master_carry": 0, "k_master_apply": 4 + 4 + 4, "k_loudness": 4}[name]


def timed(target, call, reps):
    for _ in range(2):
        call()
    target.set_profiling(True)
    for _ in range(reps):
        rows = call()
    kt = target.kernel_times()
    target.set_profiling(False)
    return {k: kt.get(k, (0.0, 0)) for k in KERNELS}, rows


def launch_frames(name, rows):
    """Frames over one call's launches of a kernel: detect once per signal, scan / carry / apply once per pass the signal
    ran, the meter once more for the input."""
    if name == "k_master_detect":
        return sum(r["frames"] for r in rows)
    extra = 1 if name == "k_loudness" else 0
    return sum(r["frames"] * (r["passes"] + extra) for r in rows)


def report(name, times, rows, reps, ceil):
    frames = sum(r["frames"] for r in rows)
    total = 0.0
    print("%s: %d signal(s), %.1f M frames, passes %s, met %s" % (name, len(rows), frames / 1e6,
                                                                   sorted({r["passes"] for r in rows}), sorted({r["met"] for r in rows})))
    for k in KERNELS:
        ms, n = times[k]
        if not n:
            continue
        per = ms / n
        total += ms / reps
        b = per_frame_bytes(k) * launch_frames(k, rows) / (n // reps)   # (mean bytes per launch)
        gbs = b / (per * 1e-3) / 1e9 if per and b else 0.0
        print("    %-16s %8.3f ms x%-2d %8.1f MB  %7.1f GB/s = %.3f of the stream ceiling" % (k, per, n // reps, b / 1e6, gbs, gbs / ceil))
    print("    whole call: %.3f ms of GPU time" % total)
    r = rows[0]
    print("    first signal: I %.2f -> %.2f LUFS, TP %.2f -> %.2f dBTP, gain %.4f, ceiling %.4f, min G %.4f"
          % (r["input_integrated"], r["integrated"], r["input_true_peak"], r["true_peak"], r["gain"], r["ceiling"], r["min_gain"]))


def main():
    if api.device_count() < 1:
        raise SystemExit("master_time.py needs a GPU")
    ceil = stream_gbs()
    print("stream ceiling (td_ubench_stream, 8 B in + 8 B out per frame): %.1f GB/s" % ceil)
    p = W.config2()
    sb, fb, g = p.build(api)
    g.render_all(sb, fb, p.cs, 16, want_f32=False)
    for target in (-14.0, -10.0, -8.0):
        times, row = timed(g, lambda: [g.master(target, -1.0)], 20)
        report("config2 60 s output to %g LUFS" % target, times, row, 20, ceil)
    projects = [W.config2(seed_offset=k) for k in range(64)]
    built = [q.build(api) for q in projects]
    b = api.Batch()
    for sb, fb, gg in built:
        b.add(sb, fb, gg)
    b.render_all(projects[0].cs, 16)
    for target in (-14.0, -10.0):
        times, rows = timed(b, lambda: b.master(target, -1.0), 5)
        report("batch 64 x config2 to %g LUFS" % target, times, rows, 5, ceil)


if __name__ == "__main__":
    main()
