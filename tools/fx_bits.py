"""The bits of the affine-scan effect kinds (comp, eq, voc, filt, lim, mb) and of the mastering pass under two builds of the
library: one fresh child process per library (TD_LIB, as tools/ab_lib.py does) renders the cases below and prints one sha256 per
case over the output's f32 words (the mastering case: its PCM words and the report's gain); then the two columns side by side and
whether they agree.  A tool, not a test: committed digests would tie the suite to one ROCm's device libm.

The kinds' parameters are tests/test_gpu_fx_level.py's table on its drum bus, at 48 kHz; the vocoder unkeyed and keyed from the
snare, the filter (follower on) likewise.  Per kind:
  whole, chunks   0.25 s in blocks of 256 rendered whole (six 2 048-frame tiles, the last one partial) and in chunks of 4 096
                  frames (two tiles)
  pulls           block pulls of 256 frames over that 0.25 s: the one-tile forms
  long            518 blocks of 1 024 frames = 530 432 frames = 259 tiles rendered whole: every carry runs with chunk 2 and the
                  last active lane folds one tile -- the second walk over more than one tile and the e = n clamp
and tests/test_gpu_master.py's drum project at that length through k_master_scan / k_master_carry / k_master_apply.

    python tools/fx_bits.py parent/libtermdaw_amd.so termdaw_amd/lib/libtermdaw_amd.so      (profiles/fx_bits.txt holds a run)"""
import hashlib
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LONG_BLOCKS, LONG_BL = 518, 1024
CASES = ("comp", "eq", "voc", "voc_key", "filt", "filt_key", "lim", "mb")


def child():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    from termdaw_amd import api, workloads as W
    import eq_projects as EP
    import fx_rig as TG
    from test_gpu_fx_level import KINDS, BL

    def sha(*arrays):
        h = hashlib.sha256()
        for a in arrays:
            h.update(np.ascontiguousarray(a).tobytes())
        return h.hexdigest()

    def project(case, bl, seconds):
        k = case.split("_")[0]
        call, params = KINDS[k][:2]
        p = EP.base_project("drums", bl=bl, seconds=seconds)
        getattr(p, call)(k, 1.0, 0.0, 1.0, *params)
        p.connect("bus", k)
        if case.endswith("_key"):
            p.connect_key("snare", k)
        p.set_output(k)
        return k, p

    for case in CASES:
        k, p = project(case, BL, 0.25)
        built = TG.build(api, p)
        for name, chunk in (("whole", 1 << 24), ("chunks", 4096)):
            y = TG.render_f32(api, built, k, p.cs, max_chunk_frames=chunk)
            assert np.isfinite(y).all() and np.abs(y).max() > 0.005, (case, name)
            print("bits %s/%s %s" % (case, name, sha(y.view(np.uint32))), flush=True)
        built[2].set_option("max_chunk_frames", 1 << 24)
        y = TG._pull_all(api, built, k, p.cs).astype(np.float32)
        print("bits %s/pulls %s" % (case, sha(y.view(np.uint32))), flush=True)
        k, p = project(case, LONG_BL, LONG_BLOCKS * LONG_BL / 48000.0)
        assert p.cs == LONG_BLOCKS, p.cs
        y = TG.render_f32(api, TG.build(api, p), k, p.cs, max_chunk_frames=1 << 24)
        assert y.shape[0] == LONG_BLOCKS * LONG_BL and np.isfinite(y).all()
        print("bits %s/long %s" % (case, sha(y.view(np.uint32))), flush=True)
    p = W.drum_project(seconds=LONG_BLOCKS * LONG_BL / 48000.0)
    assert p.cs * p.bl == LONG_BLOCKS * LONG_BL, (p.cs, p.bl)
    sb, fb, g = p.build(api)
    g.render_all(sb, fb, p.cs, 16)
    rep = g.master(-14.0, -1.0)
    print("bits master/long %s" % sha(g.read_pcm(), np.array([rep["gain"], rep["min_gain"]], np.float64)), flush=True)


def main():
    if len(sys.argv) == 2 and sys.argv[1] == "--child":
        return child()
    libs = [os.path.abspath(a) for a in sys.argv[1:3]]
    if len(libs) != 2:
        raise SystemExit(__doc__)
    cols = []
    for lib in libs:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=dict(os.environ, TD_LIB=lib), capture_output=True,
                           text=True, timeout=420)
        if r.returncode != 0:
            raise SystemExit("the child with %s ended with %d:\n%s" % (lib, r.returncode, r.stderr[-3000:]))
        cols.append(dict(ln.split()[1:3] for ln in r.stdout.splitlines() if ln.startswith("bits ")))
    print("A = %s\nB = %s" % tuple(os.path.relpath(lib, ROOT) for lib in libs))
    differ = 0
    for case in cols[0]:
        a, b = cols[0][case], cols[1].get(case, "-")
        differ += a != b
        print("%-16s %s %s %s" % (case, a, b, "same" if a == b else "DIFFERENT"))
    same = not differ and set(cols[0]) == set(cols[1])
    print("%d cases: %s" % (len(cols[0]), "every digest agrees" if same else "%d DIFFER" % differ))
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
