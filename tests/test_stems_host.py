"""Stems on the host, no GPU: the C ABI's bookkeeping of the stem list (td_graph_set_stems), and the host engine with stems set
under AddressSanitizer / UBSan (tests/asan_stems.cpp against tests/mock_hip.cpp + tests/mock_stems.cpp, built like
tests/test_compile_asan.py): random projects of tests/test_gpu_fuzz.py with 1-4 random stems each, every band mode, sine modes
1 and 2, un-chunked and chunked, fresh / scanned / continued / resampled renders, the State's stem files.  Over the seeds the
engine must report (engine option "debug.stem_taps") that a stem switched off every way it would otherwise have kept a vertex
out of memory or out of the plan."""
import multiprocessing
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import fx_rig  # noqa: E402


def test_set_stems_bookkeeping(api):
    g = api.Graph(64, 48000)
    for n in ("a", "b", "c"):
        g.add_sum(n, 1.0, 0.0)
    g.connect("a", "b")
    g.connect("b", "c")
    g.set_output("c")
    assert g.stem_count() == 0
    g.set_stems(["a", "c"])
    assert g.stem_count() == 2
    with pytest.raises(api.TermdawError, match="not found"):
        g.set_stems(["b", "nope"])
    assert g.stem_count() == 2
    with pytest.raises(api.TermdawError, match="twice"):
        g.set_stems(["b", "b"])
    assert g.stem_count() == 2
    g.set_stems([])
    assert g.stem_count() == 0
    g.set_stems(["b"])
    api.lib().td_graph_reset(g.h)
    assert g.stem_count() == 0


# engine option "debug.stem_taps": which fusions the stems switched off in what the engine compiled (compile.cpp)
CASES = {"loop": 1, "stage": 2, "adsr": 4, "band_link": 8, "presum": 16, "unreached": 32}


def _pick(seed):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import test_gpu_fuzz as F
    if seed < 0:   # (a short BASELINE config 4: a pre-summed chain of band-pass links, stems on the Sum and on a link)
        from termdaw_amd import workloads as W
        return W.config4(seconds=0.5, depth=12), ["mix", "c001"]
    p = F.random_project(seed, allow_sinf=True)
    rng = np.random.default_rng(50_000 + seed)
    names = sorted({c[0] for k, cs in p.calls.items() if k.startswith("add_") for c in cs})
    stems = [str(x) for x in rng.choice(names, size=min(len(names), int(rng.integers(1, 5))), replace=False)]
    return p, stems


def _write_projects(args):
    base, seeds = args
    out = []
    for seed in seeds:
        p, stems = _pick(seed)
        d = os.path.join(base, "s%d" % seed)
        lua = p.to_lua(os.path.join(d, "assets"))
        with open(os.path.join(d, "project.lua"), "w") as f:
            f.write(lua)
        with open(os.path.join(d, "meta.txt"), "w") as f:
            f.write(str(p.bl))
        with open(os.path.join(d, "stems.txt"), "w") as f:
            f.write("\n".join(stems) + "\n")
        out.append(d)
    return out


@pytest.mark.skipif(shutil.which("g++") is None or not os.path.exists("/opt/rocm/include/hip/hip_runtime_api.h"), reason="needs g++ and the HIP headers")
def test_stems_under_sanitizers(tmp_path, tmp_path_factory):
    exe = fx_rig.asan_exe(tmp_path_factory, "asan_stems", ["mock_stems.cpp", "asan_stems.cpp"])
    n = int(os.environ.get("TD_ASAN_STEM_SEEDS", "160"))
    workers = max(1, min(8, os.cpu_count() or 1))
    env = dict(os.environ, **fx_rig.ENV)
    seeds = [-1] + list(range(n))
    base = str(tmp_path / "p")
    with multiprocessing.Pool(workers) as pool:
        lists = pool.map(_write_projects, [(base, seeds[i::workers]) for i in range(workers) if seeds[i::workers]])
    procs = [subprocess.Popen([exe] + lst, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for lst in lists]
    renders = loops = buffers = taps = 0
    for p in procs:
        out, err = p.communicate(timeout=1800)
        assert p.returncode == 0, (out[-800:], err[-4000:])
        assert "asan_stems done" in out
        renders += int(out.split(" renders")[0].split()[-1])
        loops += int(out.split(" loop descriptors")[0].split()[-1])
        buffers += int(out.split(" buffer descriptors")[0].split("(")[-1])
        taps |= int(out.split("stem taps ")[1].split()[0])
    missed = sorted(k for k, bit in CASES.items() if not taps & bit)
    assert not missed, "the engine never switched off these fusions for a stem over %d seeds: %s" % (n, missed)
    assert renders >= n * 20 and loops > 0 and buffers > 0, (renders, loops, buffers)
    print("asan_stems: %d projects, %d renders, %d buffer / %d loop stem descriptors clean" % (n, renders, buffers, loops))
