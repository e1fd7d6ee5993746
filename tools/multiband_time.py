"""The multiband vertex' launches (k_mb_local / k_mb_carry / k_mb_detect / k_mb_carry_y1 / k_mb_env / k_mb_carry_yl / k_mb_apply,
DESIGN.md §3y) timed on the GPU box: BASELINE config 2's 64 loops summed into a bus, ONE multiband vertex on that 60 s /
2 880 512-frame bus in front of the Normalize output; 64 multiband vertices in one level on a 10 s bus; and a 1 024-frame pull of the
single vertex (the one-launch form).  Per case and kernel: the launch's own HIP-event time (the graph's profiling events, mean per
launch over 10 renders after a discarded first), the bytes a launch must move -- frames times the bytes per frame below -- and that
rate against the repo's measured stream ceiling (tools/ubench/ceilings.hip td_ubench_stream, as bench.py --full reports).  The
yardsticks beside it, in the same process: a compressor vertex (§3m) and a 16-band vocoder vertex (§3v) in the multiband's place.

    python tools/multiband_time.py            (writes profiles/multiband_time.txt)"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from termdaw_amd import api, workloads as W  # noqa: E402
from gate_time import _Tee, timed  # noqa: E402
from stems_time import stream_gbs  # noqa: E402

KERNELS = ("k_mb_local", "k_mb_carry", "k_mb_detect", "k_mb_carry_y1", "k_mb_env", "k_mb_carry_yl", "k_mb_apply")
COMP = ("k_comp_detect", "k_comp_carry_y1", "k_comp_env", "k_comp_carry_yl", "k_comp_apply")
VOC = ("k_voc_local", "k_voc_carry_z", "k_voc_env", "k_voc_carry_env", "k_voc_apply")
# bytes per frame: local reads the bus (8) and writes the summed input (8); detect reads it (8) and writes three d (24); env
# reads and writes the three (48); apply reads the summed input (8) and the three y1 twice (48: once for the attack's run, once
# for the frames) and writes the vertex' frames (8); the carries touch 36 + 36 words, or two, per 2 048-frame tile.  The
# compressor's (tools/comp_time.py): 24 / 16 / 24.  The vocoder's (tools/vocoder_time.py): 16 / 8 / 16 beside its band tables.
BYTES = {"k_mb_local": 16, "k_mb_carry": 0, "k_mb_detect": 32, "k_mb_carry_y1": 0, "k_mb_env": 48, "k_mb_carry_yl": 0, "k_mb_apply": 64,
         "k_comp_detect": 24, "k_comp_carry_y1": 0, "k_comp_env": 16, "k_comp_carry_yl": 0, "k_comp_apply": 24,
         "k_voc_local": 16, "k_voc_carry_z": 0, "k_voc_env": 8, "k_voc_carry_env": 0, "k_voc_apply": 16}
MB = (200.0, 2000.0, (-30.0, -24.0, -18.0), (4.0, 3.0, 2.0), 5.0, 150.0, 6.0, (3.0, 2.0, 1.0))
REPS = 10


def project(seconds=60.0, what="mb", n=1, seed_offset=0):
    p = W.config2(seconds, seed_offset=seed_offset)
    # config 2 connects its loops to the Normalize vertex `sum`: route them through a bus and the effect vertices instead
    loops = [a for a, b in p.calls["connect"] if b == "sum"]
    p.calls["connect"] = [(a, "bus") for a in loops]
    p.calls["add_sum"].append(("bus", 1.0 / 16.0, 0.0))   # (64 full-scale loops: the bus sits around -15 dB, above every threshold)
    for i in range(n):
        fx = "fx%d" % i
        if what == "comp":
            p.calls["add_compressor"].append((fx, 1.0, 0.0, 1.0, -18.0, 4.0, 5.0, 150.0, 6.0, 3.0))
        elif what == "voc":
            p.calls["add_vocoder"].append((fx, 1.0, 0.0, 1.0, 16, 100.0, 8000.0, 6.0, 8.0, 12.0))
        else:
            p.calls["add_multiband"].append((fx, 1.0, 0.0, 1.0) + MB[:2] + ((MB[2][0] - 0.1 * i,) + MB[2][1:],) + MB[3:])
        p.calls["connect"] += [("bus", fx), (fx, "sum")]
    return p


def report(name, kt, frames, reps, ceil, names=KERNELS):
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


def single(p, reps=REPS):
    sb, fb, g = p.build(api)

    def one():
        g.reset_normalize_vertices()
        fb.set_time(0)
        g.set_time(0)
        g.render_all(sb, fb, p.cs, 16, want_f32=False, want_pcm=False)
    return timed(g, one, reps)


def pulls(p, reps=REPS):
    sb, fb, g = p.build(api)

    def one():
        g.render(sb, fb)
        fb.set_time_to_next_block()
    return timed(g, one, reps)


def main():
    if api.device_count() < 1:
        raise SystemExit("multiband_time.py needs a GPU")
    ceil = stream_gbs()
    print("stream ceiling (td_ubench_stream, 8 B in + 8 B out per frame): %.1f GB/s" % ceil)
    p = project()
    frames = p.cs * p.bl
    kt = single(p)
    mb = report("one multiband vertex on the config-2 bus (60 s)", kt, frames, REPS, ceil)
    whole = sum(ms for ms, _ in kt.values()) / REPS
    print("    the whole render's launches: %.3f ms (%s)" % (whole, ", ".join("%s %.3f" % (k, v[0] / REPS) for k, v in sorted(kt.items()))))
    comp = report("yardstick: one compressor vertex in its place", single(project(what="comp")), frames, REPS, ceil, COMP)
    voc = report("yardstick: one 16-band vocoder vertex in its place", single(project(what="voc")), frames, REPS, ceil, VOC)
    print("multiband / compressor = %.2f, multiband / 16-band vocoder = %.2f" % (mb / comp if comp else 0.0, mb / voc if voc else 0.0))
    q = project(seconds=10.0, n=64)
    qf = q.cs * q.bl
    many = report("64 multiband vertices in one level on a 10 s bus", single(q), qf * 64, REPS, ceil)
    manyc = report("yardstick: 64 compressor vertices in one level", single(project(seconds=10.0, what="comp", n=64)), qf * 64, REPS, ceil, COMP)
    print("64 in a level: multiband / compressor = %.2f" % (many / manyc if manyc else 0.0))
    report("a 1 024-frame pull of the one vertex (k_mb_apply alone)", pulls(project(seconds=1.0)), 1024, REPS, ceil)
    report("yardstick: a 1 024-frame pull of the compressor vertex", pulls(project(seconds=1.0, what="comp")), 1024, REPS, ceil, COMP)


if __name__ == "__main__":
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "multiband_time.txt"), "w") as out:
        sys.stdout = _Tee(sys.__stdout__, out)
        try:
            main()
        finally:
            sys.stdout = sys.__stdout__
