"""The vocoder vertex' launches (k_voc_local / k_voc_carry / k_voc_env / k_voc_carry / k_voc_apply) timed on the GPU
box: BASELINE config 2's 64 loops summed into a bus, ONE vocoder vertex on that 60 s / 2 880 512-frame bus in front of the
Normalize output, keyed by a second loop source, at 4, 8 and 16 bands -- and 64 such vertices side by side in one level on a 10 s
bus (one launch of every step over 64 descriptors).  As yardsticks, in the same process on the same 60 s bus: the 8-stage phaser
and the compressor.  One 1 024-frame block pull of the single-vertex graph (the one-launch form) closes each band count.  Per
case and kernel: the launch's own HIP-event time (the graph's profiling events), mean per launch, and the launches per render.

    python tools/vocoder_time.py [out]            (writes profiles/vocoder_time.txt, or `out`)"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from termdaw_amd import api, workloads as W  # noqa: E402

KERNELS = {
    "vocoder": ("k_voc_local", "k_voc_carry_z", "k_voc_env", "k_voc_carry_env", "k_voc_apply"),
    "phaser": ("k_phaser_local", "k_phaser_carry", "k_phaser_apply"),
    "compressor": ("k_comp_detect", "k_comp_carry_y1", "k_comp_env", "k_comp_carry_yl", "k_comp_apply"),
}
REPS = 10


def project(kind, bands=16, n=1, seconds=60.0):
    p = W.config2(seconds=seconds)
    # config 2 connects its loops to the Normalize vertex `sum`: route them through a bus and the effect vertices instead
    loops = [a for a, b in p.calls["connect"] if b == "sum"]
    p.calls["connect"] = [(a, "bus") for a in loops]
    p.calls["add_sum"].append(("bus", 1.0, 0.0))
    for i in range(n):
        fx = "fx%d" % i
        if kind == "vocoder":
            p.calls["add_vocoder"].append((fx, 1.0, 0.0, 0.5, bands, 100.0, 8000.0, 6.0, 8.0, 12.0))
            p.calls["connect_key"].append((loops[-1 - i % 8], fx))   # a second loop source: one of the bus' own loops, gathered again
        elif kind == "phaser":
            p.calls["add_phaser"].append((fx, 1.0, 0.0, 0.5, 8, 200.0, 4000.0, 0.5, 0.7, 0.25, "sine"))
        else:
            p.calls["add_compressor"].append((fx, 1.0, 0.0, 1.0, -30.0, 4.0, 1.0, 20.0, 6.0, 0.0))
        p.calls["connect"] += [("bus", fx), (fx, "sum")]
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


def report(out, name, kind, kt, reps):
    total = 0.0
    out.append(name)
    for k in KERNELS[kind]:
        ms, n = kt.get(k, (0.0, 0))
        if not n:
            continue
        total += ms / reps
        out.append("    %-16s %9.4f ms per launch, %d per render" % (k, ms / n, n // reps))
    out.append("    all of them: %.3f ms of GPU time per render; every launch of the render: %.3f ms" % (total, sum(ms for ms, _ in kt.values()) / reps))


def whole(p, built):
    sb, fb, g = built

    def one():
        g.reset_normalize_vertices()
        fb.set_time(0)
        g.set_time(0)
        g.render_all(sb, fb, p.cs, 16, want_f32=False, want_pcm=False)
    return one


def main():
    if api.device_count() < 1:
        raise SystemExit("vocoder_time.py needs a GPU")
    out = []
    for bands in (4, 8, 16):
        p = project("vocoder", bands)
        built = p.build(api)
        sb, fb, g = built
        report(out, "%d bands, one keyed vertex on the config-2 bus, %.2f M frames" % (bands, p.cs * p.bl / 1e6), "vocoder", timed(g, whole(p, built), REPS), REPS)
        fb.set_time(0)
        g.set_time(0)

        def pull():
            g.render(sb, fb)
            fb.set_time_to_next_block()
        report(out, "%d bands, one block pull of %d frames" % (bands, p.bl), "vocoder", timed(g, pull, REPS), REPS)
        del built, sb, fb, g
        p = project("vocoder", bands, n=64, seconds=10.0)
        built = p.build(api)
        report(out, "%d bands, 64 keyed vertices in one level on a 10 s bus, %.2f M frames each" % (bands, p.cs * p.bl / 1e6), "vocoder",
               timed(built[2], whole(p, built), 3), 3)
        del built
    for kind in ("phaser", "compressor"):
        p = project(kind)
        built = p.build(api)
        report(out, "yardstick: %s, one vertex on the config-2 bus, %.2f M frames" % ("the 8-stage phaser" if kind == "phaser" else "the compressor", p.cs * p.bl / 1e6),
               kind, timed(built[2], whole(p, built), REPS), REPS)
        del built
    text = "\n".join(out) + "\n"
    print(text)
    with open(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "vocoder_time.txt"), "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
