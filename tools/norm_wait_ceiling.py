"""Tuning aid: what the in-launch hand-off of the running peak costs the headline launch.  Config 2 in a pipelined
render loop, one process, two graphs built from the same project: engine option debug.norm 0 (the shipped order) against
debug.norm 2 (the earlier tiles' words are not read at all: timing only, WRONG peak), alternating; one discarded round per
setting, then ROUNDS each.  The difference of the medians is the most any re-ordering of the epilogue around the wait can
bring; the spread (max - min) of the debug.norm 0 rounds is the noise it is set against.
Further debug.norm settings can be timed beside the two (8: the other order of a tile's store and its wait than the default); for
each setting but 2 one more render with bit 4 added counts the blocks that render stored twice (td_graph_norm_respec).
usage: python tools/norm_wait_ceiling.py [renders per round, default 1000] [extra debug.norm settings to time as well ...]"""
import statistics, sys, time
sys.path.insert(0, ".")
from termdaw_amd import api, workloads as W

RENDERS = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
SETTINGS = [0, 2] + [int(a) for a in sys.argv[2:]]
ROUNDS = 5
p = W.config2(seconds=60.0)
built = {}
for dbg in SETTINGS:
    sb, fb, g = p.build(api)
    for k, v in (("fuse_sources", 1), ("packed_samples", 1), ("output_f32", 0), ("debug.norm", dbg)):
        g.set_option(k, v)
    built[dbg] = (sb, fb, g)


def round_us(dbg, n):
    sb, fb, g = built[dbg]
    for _ in range(50):   # (the other graph's tables have just been through the caches)
        g.reset_normalize_vertices(); fb.set_time(0); g.render_all_async(sb, fb, p.cs, 16)
    g.sync()
    t0 = time.perf_counter()
    for _ in range(n):
        g.reset_normalize_vertices(); fb.set_time(0); g.render_all_async(sb, fb, p.cs, 16)
    g.sync()
    return (time.perf_counter() - t0) / n * 1e6


t_pre = time.perf_counter()
while time.perf_counter() - t_pre < 0.5:   # steady device clocks first
    for dbg in SETTINGS:
        round_us(dbg, 100)
us = {dbg: [] for dbg in SETTINGS}
for r in range(ROUNDS + 1):
    for dbg in SETTINGS:
        t = round_us(dbg, RENDERS)
        if r:
            us[dbg].append(t)
for dbg in SETTINGS:
    v = us[dbg]
    print("debug.norm %d: %s us per render  median %.2f  spread %.2f  (fix runs %d)"
          % (dbg, " ".join("%.2f" % x for x in v), statistics.median(v), max(v) - min(v), built[dbg][2].norm_fix_runs()), flush=True)
for dbg in SETTINGS:
    if dbg & 2:
        continue
    sb, fb, g = built[dbg]
    g.set_option("debug.norm", dbg | 16)
    counts = []
    for _ in range(5):
        g.reset_normalize_vertices(); fb.set_time(0); g.render_all_async(sb, fb, p.cs, 16); g.sync()
        counts.append(g.norm_respec())
    print("debug.norm %d: blocks stored twice in five single renders: %s of %d (early store default: %d)"
          % (dbg, counts, p.cs, g.get_option("debug.norm_early_store")))
m0, s0 = statistics.median(us[0]), max(us[0]) - min(us[0])
for dbg in SETTINGS[1:]:
    d = m0 - statistics.median(us[dbg])
    print("debug.norm 0 - debug.norm %d: %.2f us = %.1f spreads of debug.norm 0 (%.2f us)" % (dbg, d, d / max(s0, 1e-9), s0))
