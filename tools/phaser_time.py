"""The phaser vertex' launches (k_phaser_local / k_phaser_carry / k_phaser_apply) timed on the GPU box: BASELINE
config 2's 64 loops summed into a bus, ONE phaser vertex on that 60 s / 2 880 512-frame bus in front of the Normalize output, at 4
and at 8 stages -- rendered whole and in 4 096-frame chunks -- and one 1 024-frame block pull of the same graph.  Per case and
kernel: the launch's own HIP-event time (the graph's profiling events), mean per launch, and the launches per render.

    python tools/phaser_time.py            (writes profiles/phaser_time.txt)"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from termdaw_amd import api, workloads as W  # noqa: E402

KERNELS = ("k_phaser_local", "k_phaser_carry", "k_phaser_apply")
REPS = 10


def project(stages):
    p = W.config2()
    # config 2 connects its loops to the Normalize vertex `sum`: route them through a bus and the phaser instead
    loops = [a for a, b in p.calls["connect"] if b == "sum"]
    p.calls["connect"] = [(a, "bus") for a in loops] + [("bus", "fx"), ("fx", "sum")]
    p.calls["add_sum"].append(("bus", 1.0, 0.0))
    p.calls["add_phaser"].append(("fx", 1.0, 0.0, 0.5, stages, 200.0, 4000.0, 0.5, 0.7, 0.25, "sine"))
    return p


def timed(g, call, reps):
    for _ in range(2):
        call()
    g.set_profiling(True)
    for _ in range(reps):
        call()
    kt = g.kernel_times()
    g.set_profiling(False)
    return kt


def report(out, name, kt, reps):
    total = 0.0
    out.append(name)
    for k in KERNELS:
        ms, n = kt.get(k, (0.0, 0))
        if not n:
            continue
        total += ms / reps
        out.append("    %-16s %9.4f ms per launch, %d per render" % (k, ms / n, n // reps))
    out.append("    all of them: %.3f ms of GPU time per render; every launch of the render: %.3f ms" % (total, sum(ms for ms, _ in kt.values()) / reps))


def main():
    if api.device_count() < 1:
        raise SystemExit("phaser_time.py needs a GPU")
    out = []
    for stages in (4, 8):
        p = project(stages)
        sb, fb, g = p.build(api)
        frames = p.cs * p.bl

        def one():
            g.reset_normalize_vertices()
            fb.set_time(0)
            g.set_time(0)
            g.render_all(sb, fb, p.cs, 16, want_f32=False, want_pcm=False)
        for chunk, what in ((1 << 24, "whole"), (4096, "in 4 096-frame chunks")):
            g.set_option("max_chunk_frames", chunk)
            report(out, "%d stages, one vertex on the config-2 bus, %.2f M frames, %s" % (stages, frames / 1e6, what), timed(g, one, REPS if chunk > 4096 else 2),
                   REPS if chunk > 4096 else 2)
        g.set_option("max_chunk_frames", 1 << 24)
        fb.set_time(0)
        g.set_time(0)

        def pull():
            g.render(sb, fb)
            fb.set_time_to_next_block()
        report(out, "%d stages, one block pull of %d frames" % (stages, p.bl), timed(g, pull, REPS), REPS)
    text = "\n".join(out) + "\n"
    print(text)
    with open(os.path.join(ROOT, "profiles", "phaser_time.txt"), "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
