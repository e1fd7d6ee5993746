"""The chorus vertex' launches (k_chorus_sum / k_chorus) timed on the GPU box: BASELINE config 2's 64 loops summed
into a bus, and on that 60 s / 2 880 512-frame bus one chorus vertex with V = 1, 2, 4 voices (20 ms +- 4 ms at 0.8 Hz, the right
channel a quarter cycle ahead, a line of 1 216 frames) and, as the yardsticks of the same run, one saturator vertex at R = 1
(§3p: one launch, a memoryless f64 shaper -- the cost of the term loop, the stores and little else) and one EQ vertex (§3n: three
launches) -- each rendered as the output; then a batch of 64 such projects (seed offsets 0..63).  Per case, candidate tile
length ("debug.chorus_tile" 256 | 512 | 1024) and kernel: the launch's own HIP-event time (the graph's / batch's profiling
events, mean per launch over the renders).

No time bar is fixed: the table is what the default tile length is chosen from.

    python tools/chorus_time.py [out.txt]       (default: profiles/chorus_time.txt)"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from termdaw_amd import api, workloads as W  # noqa: E402

CHORUS = ("k_chorus_sum", "k_chorus")
SAT1 = ("k_sat1",)
EQ = ("k_eq_local", "k_eq_carry", "k_eq_apply")
VOICES = (1, 2, 4)
TILES = (256, 512, 1024)
LINES = []


def say(s=""):
    print(s, flush=True)
    LINES.append(s)


def project(seed_offset=0):
    p = W.config2(seed_offset=seed_offset)
    # config 2 connects its loops to the Normalize vertex `sum`: route them through a bus and hang the vertices under test on it
    loops = [a for a, b in p.calls["connect"] if b == "sum"]
    p.calls["connect"] = [(a, "bus") for a in loops] + [("bus", "sum")]
    p.calls["add_sum"].append(("bus", 1.0, 0.0))
    for V in VOICES:
        p.calls["add_chorus"].append(("c%d" % V, 1.0, 0.0, 0.5, V, 20.0, 4.0, 0.8, 0.25, "sine"))
        p.calls["connect"].append(("bus", "c%d" % V))
    p.calls["add_saturator"].append(("sat1", 1.0, 0.0, 1.0, "cubic", 12.0, 0.1, -3.0, 1))
    p.calls["connect"].append(("bus", "sat1"))
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


def report(name, kt, frames, reps, names):
    total = 0.0
    say("%s: %.1f M frames" % (name, frames / 1e6))
    for k in names:
        ms, n = kt.get(k, (0.0, 0))
        if not n:
            continue
        total += ms / reps
        say("    %-16s %8.3f ms x%-2d" % (k, ms / n, n // reps))
    say("    all of them: %.3f ms of GPU time per render" % total)
    return total


def main():
    if api.device_count() < 1:
        raise SystemExit("chorus_time.py needs a GPU")
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "chorus_time.txt")
    nb = int(os.environ.get("TD_CHORUS_TIME_BATCH", "64"))
    p = project()
    sb, fb, g = p.build(api)
    frames = p.cs * p.bl
    reps = 10

    def one():
        fb.set_time(0)
        g.set_time(0)
        g.render_all(sb, fb, p.cs, 16, want_f32=False, want_pcm=False)
    yard = {}
    for out, names in (("sat1", SAT1), ("eq", EQ)):
        assert g.set_output(out)
        yard[out] = report("yardstick, one %s vertex on the config-2 bus (60 s)" % out, timed(g, one, reps), frames, reps, names)
    default = g.get_option("debug.chorus_tile")   # (the engine's choice)
    table = {}
    for V in VOICES:
        assert g.set_output("c%d" % V)
        for tile in TILES:
            g.set_option("debug.chorus_tile", tile)
            table[(V, tile)] = report("one chorus vertex, V = %d, %d frames per tile" % (V, tile), timed(g, one, reps), frames, reps, CHORUS)
    g.set_option("debug.chorus_tile", default)
    say("\nk_chorus_sum + k_chorus per render, ms (the engine's default is F = %d; k_sat1 %.3f, the EQ's three %.3f)" % (default, yard["sat1"], yard["eq"]))
    say("    %4s " % "V" + " ".join("%9s" % ("F=%d" % t) for t in TILES))
    for V in VOICES:
        say("    %4d " % V + " ".join("%9.3f" % table[(V, t)] for t in TILES))
    projects = [project(seed_offset=k) for k in range(nb)]
    built = [q.build(api) for q in projects]
    b = api.Batch()
    for bsb, bfb, bg in built:
        b.add(bsb, bfb, bg)

    def many():
        b.rewind()
        b.render_all(projects[0].cs, 16)
    for out, names in [("sat1", SAT1), ("eq", EQ)] + [("c%d" % V, CHORUS) for V in VOICES]:
        for _, _, bg in built:
            assert bg.set_output(out)
        report("batch of %d such projects, output %s" % (nb, out), timed(b, many, 3), frames * nb, 3, names)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
