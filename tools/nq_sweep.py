"""Tuning aid: config-2-like renders of several lengths with the packed loop sum forced to 4 / 8 / 16 frames per lane
(TD_FORCE_NQ = 1 | 2 | 4; read once per process, hence one subprocess per setting), in the ragged form on 3 / 4 / 5 workgroups
per CU (engine option debug.sum_groups; lengths whose quads such a grid cannot carry are skipped), and as the engine chooses
by itself ("auto").   usage: python tools/nq_sweep.py [setting ...]   (nq1 nq2 nq4 r3 r4 r5 auto)"""
import os, subprocess, sys
code = r'''
import os, sys, time
sys.path.insert(0, ".")
from termdaw_amd import api, workloads as W
wpc = int(os.environ.get("SWEEP_WPC", "0"))
for secs in (3.0, 6.0, 12.0, 24.0, 45.0, 56.0, 60.0, 75.0, 87.0, 120.0, 300.0):
    p = W.config2(seconds=secs)
    quads = p.cs * 4
    G = wpc * 256
    if wpc and not (4 * G <= quads <= 16 * G):
        print("%6.0f s %5d tiles: (%d workgroups cannot carry %d quads)" % (secs, p.cs, G, quads))
        continue
    sb, fb, g = p.build(api)
    for k, v in (("fuse_sources", 1), ("packed_samples", 1), ("output_f32", 0)):
        g.set_option(k, v)
    if wpc:
        g.set_option("debug.sum_groups", G)
    try:
        for _ in range(5):
            g.reset_normalize_vertices(); fb.set_time(0); g.render_all_async(sb, fb, p.cs, 16)
        g.sync()
    except api.TermdawError as e:   # (a grid the device does not hold at once: no single-pass Normalize in this form)
        print("%6.0f s %5d tiles: refused (%s)" % (secs, p.cs, str(e)[:60]))
        continue
    t0 = time.perf_counter(); N = 30
    for _ in range(N):
        g.reset_normalize_vertices(); fb.set_time(0); g.render_all_async(sb, fb, p.cs, 16)
    g.sync()
    dt = (time.perf_counter() - t0) / N
    print("%6.0f s %5d tiles: %.4f ms  %8.0f Msamples/s" % (secs, p.cs, dt * 1e3, p.cs * 1024 / dt / 1e6), flush=True)
'''
SETTINGS = {"nq1": {"TD_FORCE_NQ": "1"}, "nq2": {"TD_FORCE_NQ": "2"}, "nq4": {"TD_FORCE_NQ": "4"},
            "r3": {"SWEEP_WPC": "3"}, "r4": {"SWEEP_WPC": "4"}, "r5": {"SWEEP_WPC": "5"}, "auto": {}}
for name in (sys.argv[1:] or list(SETTINGS)):
    print(name, SETTINGS[name], flush=True)
    subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **SETTINGS[name]))
