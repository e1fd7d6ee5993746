"""The filter vertex' launches (k_filt_detect / k_master_carry / k_filt_env / k_master_carry / k_filt_local / k_filt_carry /
k_filt_apply) timed on the GPU box: BASELINE config 2's 64 loops summed into a bus, ONE filter vertex on that 60 s /
2 880 512-frame bus in front of the Normalize output -- unkeyed and keyed by a second loop source, with env_oct 0 (no follower
launches) and non-zero -- rendered whole and in 4 096-frame chunks, and one 1 024-frame block pull of the same graph (the
one-launch form).  As yardsticks, in the same process on the same 60 s bus: the 8-stage phaser and the compressor.  Per case and
kernel: the launch's own HIP-event time (the graph's profiling events), mean per launch, and the launches per render.

    python tools/filter_time.py [out]            (writes profiles/filter_time.txt, or `out`)"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from termdaw_amd import api, workloads as W  # noqa: E402

KERNELS = {
    "filter": ("k_filt_detect", "k_filt_carry_y1", "k_filt_env", "k_filt_carry_e", "k_filt_local", "k_filt_carry", "k_filt_apply"),
    "phaser": ("k_phaser_local", "k_phaser_carry", "k_phaser_apply"),
    "compressor": ("k_comp_detect", "k_comp_carry_y1", "k_comp_env", "k_comp_carry_yl", "k_comp_apply"),
}
REPS = 10


def project(kind, env_oct=4.0, keyed=False, seconds=60.0):
    p = W.config2(seconds=seconds)
    # config 2 connects its loops to the Normalize vertex `sum`: route them through a bus and the effect vertex instead
    loops = [a for a, b in p.calls["connect"] if b == "sum"]
    p.calls["connect"] = [(a, "bus") for a in loops]
    p.calls["add_sum"].append(("bus", 1.0, 0.0))
    if kind == "filter":
        p.calls["add_filter"].append(("fx", 1.0, 0.0, 0.8, "lowpass", 400.0, 4.0, 2.0, 3.0, 0.25, "sine", env_oct, 18.0, 2.0, 80.0))
        if keyed:
            p.calls["connect_key"].append((loops[-1], "fx"))   # a second loop source: one of the bus' own loops, gathered again
    elif kind == "phaser":
        p.calls["add_phaser"].append(("fx", 1.0, 0.0, 0.5, 8, 200.0, 4000.0, 0.5, 0.7, 0.25, "sine"))
    else:
        p.calls["add_compressor"].append(("fx", 1.0, 0.0, 1.0, -30.0, 4.0, 1.0, 20.0, 6.0, 0.0))
    p.calls["connect"] += [("bus", "fx"), ("fx", "sum")]
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
        raise SystemExit("filter_time.py needs a GPU")
    out = []
    for env_oct, keyed in ((0.0, False), (4.0, False), (4.0, True)):
        what = "env_oct %g, %s" % (env_oct, "keyed by a second loop" if keyed else "no key")
        p = project("filter", env_oct, keyed)
        built = p.build(api)
        sb, fb, g = built
        report(out, "%s: one vertex on the config-2 bus, %.2f M frames, whole" % (what, p.cs * p.bl / 1e6), "filter", timed(g, whole(p, built), REPS), REPS)
        g.set_option("max_chunk_frames", 4096)
        report(out, "%s: the same in 4 096-frame chunks" % what, "filter", timed(g, whole(p, built), 3), 3)
        g.set_option("max_chunk_frames", 1 << 24)
        fb.set_time(0)
        g.set_time(0)

        def pull():
            g.render(sb, fb)
            fb.set_time_to_next_block()
        report(out, "%s: one block pull of %d frames" % (what, p.bl), "filter", timed(g, pull, REPS), REPS)
        del built, sb, fb, g
    for kind in ("phaser", "compressor"):
        p = project(kind)
        built = p.build(api)
        report(out, "yardstick: %s, one vertex on the config-2 bus, %.2f M frames" % ("the 8-stage phaser" if kind == "phaser" else "the compressor", p.cs * p.bl / 1e6),
               kind, timed(built[2], whole(p, built), REPS), REPS)
        del built
    text = "\n".join(out) + "\n"
    print(text)
    with open(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "filter_time.txt"), "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
