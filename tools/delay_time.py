"""The delay vertex' launches (k_delay_local / k_delay_carry / k_delay_apply) timed on the GPU box: BASELINE
config 2's 64 loops summed into a bus, and on that 60 s / 2 880 512-frame bus one delay vertex of 1, 30 and 375 ms (48, 1 440
and 18 000 lanes) and, as the yardstick of the same run, one EQ vertex (§3n) -- each rendered as the output; then a batch of 64
such projects (seed offsets 0..63).  Per case, candidate tile length ("debug.delay_tile" 8 | 16 | 32 | 64) and kernel: the
launch's own HIP-event time (the graph's / batch's profiling events, mean per launch over the renders), the bytes a launch must
move -- frames times the bytes per frame below -- and that rate against the repo's measured stream ceiling
(tools/ubench/ceilings.hip td_ubench_stream, as bench.py --full reports).  The bar: a delay vertex' three launches take at most
1.25 x the EQ vertex' three.

    python tools/delay_time.py            (what profiles/delay_time.txt is to hold; not run yet)"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from termdaw_amd import api, workloads as W  # noqa: E402
from stems_time import stream_gbs  # noqa: E402

DELAY = ("k_delay_local", "k_delay_carry", "k_delay_apply")
EQ = ("k_eq_local", "k_eq_carry", "k_eq_apply")
# bytes per frame: local reads the bus (8) and writes the summed input (8); apply reads the summed input (8) and writes the
# vertex' frames (8); the tile words (16 B per lane and tile, written once and read twice) are 48 / T bytes per frame on top and
# not counted here.  The EQ's: tools/eq_time.py.
BYTES = {"k_delay_local": 16, "k_delay_carry": 0, "k_delay_apply": 16, "k_eq_local": 16, "k_eq_carry": 0, "k_eq_apply": 16}
TIMES_MS = (1.0, 30.0, 375.0)
TILES = (8, 16, 32, 64)
BAR = 1.25


def project(seed_offset=0):
    p = W.config2(seed_offset=seed_offset)
    # config 2 connects its loops to the Normalize vertex `sum`: route them through a bus and hang the vertices under test on it
    loops = [a for a, b in p.calls["connect"] if b == "sum"]
    p.calls["connect"] = [(a, "bus") for a in loops] + [("bus", "sum")]
    p.calls["add_sum"].append(("bus", 1.0, 0.0))
    for t in TIMES_MS:
        p.calls["add_delay"].append(("d%g" % t, 1.0, 0.0, 1.0, t, 0.5, 0.35))
        p.calls["connect"].append(("bus", "d%g" % t))
    p.calls["add_eq"].append(("eq", 1.0, 0.0, 1.0, "peak", 1000.0, 2.0, 6.0))
    p.calls["connect"].append(("bus", "eq"))
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


def report(name, kt, frames, reps, ceil, names):
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
        raise SystemExit("delay_time.py needs a GPU")
    ceil = stream_gbs()
    print("stream ceiling (td_ubench_stream, 8 B in + 8 B out per frame): %.1f GB/s" % ceil)
    p = project()
    sb, fb, g = p.build(api)
    frames = p.cs * p.bl

    def one():
        fb.set_time(0)
        g.set_time(0)
        g.render_all(sb, fb, p.cs, 16, want_f32=False, want_pcm=False)
    assert g.set_output("eq")
    eq = report("yardstick, one EQ vertex on the config-2 bus (60 s)", timed(g, one, 20), frames, 20, ceil, EQ)
    table, missed = {}, []
    default = g.get_option("debug.delay_tile")   # (the engine's choice)
    for t in TIMES_MS:
        assert g.set_output("d%g" % t)
        for tile in TILES:
            g.set_option("debug.delay_tile", tile)
            table[(t, tile)] = report("one delay vertex, %g ms, %d steps per tile" % (t, tile), timed(g, one, 20), frames, 20, ceil, DELAY)
    print("\ndelay / EQ (three launches each, the same run); the bar is %.2f" % BAR)
    print("    %8s " % "ms" + " ".join("%8s" % ("T=%d" % tile) for tile in TILES))
    for t in TIMES_MS:
        print("    %8g " % t + " ".join("%8.2f" % (table[(t, tile)] / eq) for tile in TILES))
        if table[(t, default)] > BAR * eq:
            missed.append(t)
    print("    the engine's default is T = %d: %s" % (default, "every case inside the bar" if not missed else "OVER THE BAR at %s ms" % missed))
    g.set_option("debug.delay_tile", default)
    projects = [project(seed_offset=k) for k in range(64)]
    built = [q.build(api) for q in projects]
    b = api.Batch()
    for bsb, bfb, bg in built:
        b.add(bsb, bfb, bg)

    def many():
        b.rewind()
        b.render_all(projects[0].cs, 16)
    for out, names in [("eq", EQ)] + [("d%g" % t, DELAY) for t in TIMES_MS]:
        for _, _, bg in built:
            assert bg.set_output(out)
        tot = report("batch of 64 such projects, output %s" % out, timed(b, many, 5), frames * 64, 5, ceil, names)
        if out == "eq":
            beq = tot
        else:
            print("    delay / EQ = %.2f" % (tot / beq))


if __name__ == "__main__":
    main()
