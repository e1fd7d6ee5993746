"""The stem launch (k_stems) timed on the GPU box: BASELINE config 2 with 0 / 1 / 8 / 64 of its loop sources as stems, and
config 3 with a stem on its Adsr vertex (front-end defaults: band_mode 2, sine_mode 2).  Per case: ms per render, the
k_stems launch's own HIP-event time, its bytes, and its rate against the repo's measured stream ceiling
(tools/ubench/ceilings.hip td_ubench_stream: 8 B in + 8 B out per frame, the figure bench.py --full reports).

    python tools/stems_time.py            (profiles/stems_time.txt holds a run)"""
import ctypes
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from termdaw_amd import api, workloads as W  # noqa: E402


def stream_gbs():
    L = ctypes.CDLL(os.path.join(ROOT, "tools", "ubench", "libtd_ubench.so"))
    L.td_ubench_stream.restype = ctypes.c_float
    L.td_ubench_stream.argtypes = [ctypes.c_uint32, ctypes.c_int, ctypes.c_int, ctypes.c_int]
    fr = (1 << 30) // 8
    ms = float(L.td_ubench_stream(fr, 1, 1, 10))
    return 2.0 * fr * 8 / (ms * 1e-3) / 1e9


def run(name, p, stems, opts=(), reps=50):
    sb, fb, g = p.build(api)
    for k, v in opts:
        g.set_option(k, v)
    g.set_stems(stems)

    def render():
        g.reset_normalize_vertices(); fb.set_time(0); g.set_time(0)
        g.render_all_async(sb, fb, p.cs, 16)
    for _ in range(5):
        render()
    g.sync()
    t0 = time.perf_counter()
    for _ in range(reps):
        render()
    g.sync()
    plain = (time.perf_counter() - t0) / reps
    g.set_profiling(True)
    for _ in range(reps):
        render()
    g.sync()
    kt = g.kernel_times()
    g.set_profiling(False)
    ms, n = kt.get("k_stems", (0.0, 0))
    frames = p.cs * p.bl
    # PCM out: 4 B per frame and stem; in: a materialised buffer's 8 B per frame (a loop source's packed table is
    # gathered from the cache hierarchy: counted as 0 HBM bytes)
    loops = set(c[0] for c in p.calls.get("add_sampleloop", []))
    out_b = 4 * frames * len(stems)
    in_b = sum(8 * frames for s in stems if s not in loops)
    return {"case": name, "render_ms": plain * 1e3, "stems_ms": (ms / n) if n else 0.0, "launches_per_render": n // reps,
            "bytes_out": out_b, "bytes_in": in_b}


def main():
    ceil = stream_gbs()
    c2 = W.config2()
    loops = [c[0] for c in c2.calls["add_sampleloop"]]
    rows = [run("config2 0 stems", c2, []), run("config2 1 loop stem", c2, loops[:1]), run("config2 8 loop stems", c2, loops[:8]),
            run("config2 64 loop stems", c2, loops)]
    c3 = W.config3()
    rows.append(run("config3 0 stems", c3, [], opts=(("band_mode", 2), ("sine_mode", 2))))
    rows.append(run("config3 stem on env", c3, ["env"], opts=(("band_mode", 2), ("sine_mode", 2))))
    print("stream ceiling (td_ubench_stream, 8 B in + 8 B out per frame): %.1f GB/s" % ceil)
    for r in rows:
        gbs = (r["bytes_out"] + r["bytes_in"]) / (r["stems_ms"] * 1e-3) / 1e9 if r["stems_ms"] else 0.0
        print("%-22s render %8.3f ms   k_stems %7.3f ms x%d   %6.1f MB out %6.1f MB in   %7.1f GB/s = %.3f of the stream ceiling"
              % (r["case"], r["render_ms"], r["stems_ms"], r["launches_per_render"], r["bytes_out"] / 1e6, r["bytes_in"] / 1e6,
                 gbs, gbs / ceil))


if __name__ == "__main__":
    main()
