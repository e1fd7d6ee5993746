"""The saturator vertex' launches (k_sat_sum / k_sat / k_sat1) timed on the GPU box: BASELINE config 2's 64 loops
summed into a bus, and on that 60 s / 2 880 512-frame bus one saturator vertex at R = 1, 2, 4, 8 and, as the yardsticks of the
same run, one compressor vertex (§3m) and one EQ vertex (§3n) -- each rendered as the output; then a batch of 64 such projects
(seed offsets 0..63).  Per case, candidate tile length ("debug.sat_tile" 128 | 256 | 384) and kernel: the launch's own HIP-event
time (the graph's / batch's profiling events, mean per launch over the renders) and, for k_sat, the launch's VALU floor and the
fraction of it the launch reaches.

The floor: every output frame takes 2 Z R + 1 taps in the up-sampler (all R phases together) and 2 Z R + 1 in the decimator, per
channel; a tap is one f64 multiply and one f64 add (no FMA: the build keeps contraction off); an f64 wave-instruction takes
1.75 ns per SIMD (profiles/r02_issue_rate.txt, k_add64 at 8 waves) and the part has 1 024 SIMDs of 64 lanes:
    floor = frames x 2 channels x 2 (2 Z R + 1) taps x 2 instructions x 1.75 ns / (64 x 1 024)       (0.158 ms at R = 4)
No time bar is fixed: the table is what the default tile length is chosen from.

    python tools/sat_time.py [out.txt]       (default: profiles/sat_time.txt)"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from termdaw_amd import api, workloads as W  # noqa: E402

SAT = ("k_sat_sum", "k_sat", "k_sat1")
COMP = ("k_comp_detect", "k_comp_carry_y1", "k_comp_env", "k_comp_carry_yl", "k_comp_apply")
EQ = ("k_eq_local", "k_eq_carry", "k_eq_apply")
FACTORS = (1, 2, 4, 8)
TILES = (128, 256, 384)
Z = 32
NS_PER_F64 = 1.75
LANES = 64 * 1024
LINES = []


def say(s=""):
    print(s, flush=True)
    LINES.append(s)


def floor_ms(frames, R):
    return frames * 2 * 2 * (2 * Z * R + 1) * 2 * NS_PER_F64 * 1e-9 / LANES * 1e3


def project(seed_offset=0):
    p = W.config2(seed_offset=seed_offset)
    # config 2 connects its loops to the Normalize vertex `sum`: route them through a bus and hang the vertices under test on it
    loops = [a for a, b in p.calls["connect"] if b == "sum"]
    p.calls["connect"] = [(a, "bus") for a in loops] + [("bus", "sum")]
    p.calls["add_sum"].append(("bus", 1.0, 0.0))
    for R in FACTORS:
        p.calls["add_saturator"].append(("w%d" % R, 1.0, 0.0, 1.0, "cubic", 12.0, 0.1, -3.0, R))
        p.calls["connect"].append(("bus", "w%d" % R))
    p.calls["add_compressor"].append(("comp", 1.0, 0.0, 1.0, -18.0, 4.0, 5.0, 80.0, 6.0, 3.0))
    p.calls["connect"].append(("bus", "comp"))
    p.calls["add_eq"].append(("eq", 1.0, 0.0, 1.0, "peak", 1000.0, 2.0, 6.0))
    p.calls["connect"].append(("bus", "eq"))
    return p


def timed(target, call, reps):
    for _ in range(2):
        call()
    target.set_profiling(True)
    for _ in range(reps):
        call()
    kt = target.kernel_times()
    target.set_profiling(False)
    return kt


def report(name, kt, frames, reps, names, R=0):
    total = 0.0
    say("%s: %.1f M frames" % (name, frames / 1e6))
    for k in names:
        ms, n = kt.get(k, (0.0, 0))
        if not n:
            continue
        per = ms / n
        total += ms / reps
        if k == "k_sat" and R > 1:
            fl = floor_ms(frames, R)
            say("    %-16s %8.3f ms x%-2d  VALU floor %7.3f ms: the launch runs at %.3f of it" % (k, per, n // reps, fl, fl / per))
        else:
            say("    %-16s %8.3f ms x%-2d" % (k, per, n // reps))
    say("    all of them: %.3f ms of GPU time per render" % total)
    return total


def main():
    if api.device_count() < 1:
        raise SystemExit("sat_time.py needs a GPU")
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "sat_time.txt")
    p = project()
    sb, fb, g = p.build(api)
    frames = p.cs * p.bl
    reps = 10

    def one():
        fb.set_time(0)
        g.set_time(0)
        g.render_all(sb, fb, p.cs, 16, want_f32=False, want_pcm=False)
    for out, names in (("comp", COMP), ("eq", EQ)):
        assert g.set_output(out)
        report("yardstick, one %s vertex on the config-2 bus (60 s)" % out, timed(g, one, reps), frames, reps, names)
    default = g.get_option("debug.sat_tile")   # (the engine's choice)
    table = {}
    for R in FACTORS:
        assert g.set_output("w%d" % R)
        for tile in (TILES if R > 1 else (default,)):
            g.set_option("debug.sat_tile", tile)
            table[(R, tile)] = report("one saturator vertex, R = %d, %d frames per tile" % (R, tile), timed(g, one, reps), frames, reps, SAT, R)
    g.set_option("debug.sat_tile", default)
    say("\nk_sat_sum + k_sat per render, ms (the engine's default is F = %d)" % default)
    say("    %4s " % "R" + " ".join("%9s" % ("F=%d" % t) for t in TILES) + "   floor")
    for R in FACTORS[1:]:
        say("    %4d " % R + " ".join("%9.3f" % table[(R, t)] for t in TILES) + "   %.3f" % floor_ms(frames, R))
    nb = 64
    projects = [project(seed_offset=k) for k in range(nb)]
    built = [q.build(api) for q in projects]
    b = api.Batch()
    for bsb, bfb, bg in built:
        b.add(bsb, bfb, bg)

    def many():
        b.rewind()
        b.render_all(projects[0].cs, 16)
    for out, names, R in [("comp", COMP, 0), ("eq", EQ, 0)] + [("w%d" % R, SAT, R) for R in FACTORS]:
        for _, _, bg in built:
            assert bg.set_output(out)
        report("batch of %d such projects, output %s" % (nb, out), timed(b, many, 3), frames * nb, 3, names, R)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
