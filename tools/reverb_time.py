"""The reverb vertex' launches (k_reverb_sum / k_reverb) timed on the GPU box: BASELINE config 2's 64 loops summed
into a bus, and on that 60 s / 2 880 512-frame bus one reverb vertex (room 0.84, damp 0.2, width 1, size 2: every line at least
490 frames, so all three window lengths are open to it) in both forms ("debug.reverb_form" 0 serial, 1 scan) at each window length
("debug.reverb_block" 64 | 128 | 256) and, as the yardstick of the same run, one delay vertex (§3o: three launches) -- each
rendered as the output; then a batch of 64 such projects (seed offsets 0..63).  Per case and kernel: the launch's own HIP-event
time (the graph's / batch's profiling events, mean per launch over the renders).

No time bar is fixed: the table is what the defaults of the two options are chosen from.

    python tools/reverb_time.py [out.txt]       (default: profiles/reverb_time.txt)"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from termdaw_amd import api, workloads as W  # noqa: E402

REVERB = ("k_reverb_sum", "k_reverb")
DELAY = ("k_delay_local", "k_delay_carry", "k_delay_apply")
FORMS = ((0, "serial"), (1, "scan"))
BLOCKS = (64, 128, 256)
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
    p.calls["add_reverb"].append(("rev", 1.0, 0.0, 0.5, 0.84, 0.2, 1.0, 2.0))
    p.calls["connect"].append(("bus", "rev"))
    p.calls["add_delay"].append(("dly", 1.0, 0.0, 0.5, 30.0, 0.5, 0.35))
    p.calls["connect"].append(("bus", "dly"))
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
        raise SystemExit("reverb_time.py needs a GPU")
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "reverb_time.txt")
    nb = int(os.environ.get("TD_REVERB_TIME_BATCH", "64"))
    reps = int(os.environ.get("TD_REVERB_TIME_REPS", "5"))
    p = project()
    sb, fb, g = p.build(api)
    frames = p.cs * p.bl

    def one():
        fb.set_time(0)
        g.set_time(0)
        g.render_all(sb, fb, p.cs, 16, want_f32=False, want_pcm=False)
    assert g.set_output("dly")
    yard = report("yardstick, one delay vertex (30 ms) on the config-2 bus (60 s)", timed(g, one, reps), frames, reps, DELAY)
    defaults = g.get_option("debug.reverb_form"), g.get_option("debug.reverb_block")   # (the engine's choice)
    assert g.set_output("rev")
    table = {}
    for form, fname in FORMS:
        for B in BLOCKS:
            g.set_option("debug.reverb_form", form)
            g.set_option("debug.reverb_block", B)
            table[(form, B)] = report("one reverb vertex, %s form, %d frames per window" % (fname, B), timed(g, one, reps), frames, reps, REVERB)
    g.set_option("debug.reverb_form", defaults[0])
    g.set_option("debug.reverb_block", defaults[1])
    say("\nk_reverb_sum + k_reverb per render, ms (the engine's defaults are form %d, block %d; the delay's three launches %.3f)" % (defaults + (yard,)))
    say("    %8s " % "form" + " ".join("%9s" % ("B=%d" % b) for b in BLOCKS))
    for form, fname in FORMS:
        say("    %8s " % fname + " ".join("%9.3f" % table[(form, b)] for b in BLOCKS))
    projects = [project(seed_offset=k) for k in range(nb)]
    built = [q.build(api) for q in projects]
    b = api.Batch()
    for bsb, bfb, bg in built:
        b.add(bsb, bfb, bg)

    def many():
        b.rewind()
        b.render_all(projects[0].cs, 16)
    for out, names, form in (("dly", DELAY, None), ("rev", REVERB, 0), ("rev", REVERB, 1)):
        for _, _, bg in built:
            assert bg.set_output(out)
            if form is not None:
                bg.set_option("debug.reverb_form", form)
        what = out if form is None else "%s, %s form, block %d" % (out, dict(FORMS)[form], defaults[1])
        report("batch of %d such projects, output %s" % (nb, what), timed(b, many, 2), frames * nb, 2, names)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
