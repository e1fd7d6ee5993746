"""The limiter vertex' launches (k_lim_detect / k_lim_carry / k_lim_apply) timed on the GPU box: BASELINE
config 2's 64 loops summed into a bus, ONE limiter vertex on that 60 s / 2 880 512-frame bus in front of the Normalize output --
at a lookahead of 5 ms (240 frames) and at the longest one, 2 048 frames -- and a batch of 64 such projects (seed offsets 0..63).
Per case and kernel: the launch's own HIP-event time (the graph's / batch's profiling events, mean per launch over the renders),
the bytes a launch must move -- frames times the bytes per frame below -- and that rate against the repo's measured stream ceiling
(tools/ubench/ceilings.hip td_ubench_stream, as bench.py --full reports).  The yardstick beside it, in the same run: a compressor
vertex (§3m) in the limiter's place on the same project.

    python tools/limiter_time.py            (writes profiles/limiter_time.txt)"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from termdaw_amd import api, workloads as W  # noqa: E402
from gate_time import _Tee, timed  # noqa: E402
from stems_time import stream_gbs  # noqa: E402

KERNELS = ("k_lim_detect", "k_lim_carry", "k_lim_apply")
COMP = ("k_comp_detect", "k_comp_carry_y1", "k_comp_env", "k_comp_carry_yl", "k_comp_apply")
# bytes per frame: detect reads the bus (8; the halo's frames once more, (L - 1) / 2 048 of that, not counted), writes the summed
# input (8) and Q (4); apply reads Q of its tile and of the tile before (8), the delayed input (8) and writes the vertex' frames
# (8); the carry touches two words per 2 048-frame tile.  The compressor's (tools/comp_time.py): 24 / 16 / 24.
BYTES = {"k_lim_detect": 20, "k_lim_carry": 0, "k_lim_apply": 24,
         "k_comp_detect": 24, "k_comp_carry_y1": 0, "k_comp_env": 16, "k_comp_carry_yl": 0, "k_comp_apply": 24}


def project(seed_offset=0, comp=False, lookahead_ms=5.0):
    p = W.config2(seed_offset=seed_offset)
    # config 2 connects its loops to the Normalize vertex `sum`: route them through a bus and the limiter (or the compressor) instead
    loops = [a for a, b in p.calls["connect"] if b == "sum"]
    p.calls["connect"] = [(a, "bus") for a in loops] + [("bus", "fx"), ("fx", "sum")]
    p.calls["add_sum"].append(("bus", 1.0, 0.0))
    if comp:
        p.calls["add_compressor"].append(("fx", 1.0, 0.0, 1.0, -18.0, 4.0, 5.0, 150.0, 6.0, 3.0))
    else:   # (the bus of 64 full-scale loops sits around -3 dB: 6 dB of drive into a -1 dB ceiling works all the time)
        p.calls["add_limiter"].append(("fx", 1.0, 0.0, 1.0, -1.0, lookahead_ms, 80.0, 6.0))
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


def single(p, reps=20):
    sb, fb, g = p.build(api)

    def one():
        g.reset_normalize_vertices()
        fb.set_time(0)
        g.set_time(0)
        g.render_all(sb, fb, p.cs, 16, want_f32=False, want_pcm=False)
    return timed(g, one, reps)


def main():
    if api.device_count() < 1:
        raise SystemExit("limiter_time.py needs a GPU")
    ceil = stream_gbs()
    print("stream ceiling (td_ubench_stream, 8 B in + 8 B out per frame): %.1f GB/s" % ceil)
    p = project()
    frames = p.cs * p.bl
    kt = single(p)
    lim = report("one limiter vertex on the config-2 bus (60 s), lookahead 5 ms = 240 frames", kt, frames, 20, ceil)
    whole = sum(ms for ms, _ in kt.values()) / 20
    print("    the whole render's launches: %.3f ms (%s)" % (whole, ", ".join("%s %.3f" % (k, v[0] / 20) for k, v in sorted(kt.items()))))
    far = report("the same at the longest lookahead, 2 048 frames (the halo's terms are a whole tile's)", single(project(lookahead_ms=2048000.0 / 48000.0)),
                 frames, 20, ceil)
    comp = report("yardstick: one compressor vertex in its place", single(project(comp=True)), frames, 20, ceil, COMP)
    print("limiter / compressor = %.2f at 240 frames, %.2f at 2 048" % (lim / comp if comp else 0.0, far / comp if comp else 0.0))
    for name, is_comp, names in (("limiter", False, KERNELS), ("compressor", True, COMP)):
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


if __name__ == "__main__":
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "limiter_time.txt"), "w") as out:
        sys.stdout = _Tee(sys.__stdout__, out)
        try:
            main()
        finally:
            sys.stdout = sys.__stdout__
