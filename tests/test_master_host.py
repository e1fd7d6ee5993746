"""Loudness mastering on the host, no GPU (include/termdaw_amd.h td_graph_master): parameter ranges rejected with
messages that name the parameter, the entry points failing loudly without a render or a GPU, and the host engine mastering
random projects under AddressSanitizer / UBSan (tests/asan_master.cpp against tests/mock_hip.cpp + tests/mock_stems.cpp +
tests/mock_master.cpp, built like tests/test_loudness_host.py; the mock meter reports a non-zero loudness, so the pass loop
runs its passes, and the mock launches check every descriptor's bounds and tiling)."""
import multiprocessing
import os
import shutil
import subprocess

import numpy as np
import pytest

import fx_rig
import test_loudness_host as L


BAD = [(dict(target_lufs=-61.0), "target_lufs"), (dict(target_lufs=0.5), "target_lufs"), (dict(target_lufs=float("nan")), "target_lufs"),
       (dict(ceiling_dbtp=-31.0), "ceiling_dbtp"), (dict(ceiling_dbtp=0.1), "ceiling_dbtp"),
       (dict(lookahead_ms=0.05), "lookahead_ms"), (dict(lookahead_ms=101.0), "lookahead_ms"),
       (dict(release_ms=0.5), "release_ms"), (dict(release_ms=10001.0), "release_ms")]


def _args(kw):
    a = dict(target_lufs=-14.0, ceiling_dbtp=-1.0, lookahead_ms=5.0, release_ms=100.0)
    a.update(kw)
    return a


@pytest.mark.parametrize("kw,name", BAD)
def test_parameter_ranges_are_rejected(api, kw, name):
    a = _args(kw)
    with pytest.raises(api.TermdawError, match=name):
        api.master_f32(np.zeros((4800, 2), np.float32), 48000, **a)
    g = api.Graph(64, 48000)
    g.add_sum("a", 1.0, 0.0)
    g.set_output("a")
    with pytest.raises(api.TermdawError, match=name):
        g.master(**a)
    with pytest.raises(api.TermdawError, match=name):
        api.Batch().master(**a)


def test_state_rejects_bad_targets(api):
    s = api.State("", 48000, 64)
    with pytest.raises(api.TermdawError, match="target_lufs"):
        s.set_master(-70.0)
    with pytest.raises(api.TermdawError, match="ceiling_dbtp"):
        s.set_master(-14.0, 1.0)
    s.set_master(-14.0, -2.0)
    s.set_master(None)
    assert s.master_report() is None


def test_graph_fails_without_a_render(api):
    g = api.Graph(64, 48000)
    g.add_sum("a", 1.0, 0.0)
    g.set_output("a")
    with pytest.raises(api.TermdawError, match="no whole render"):
        g.master(-14.0)


def test_parameter_edges_are_accepted(api):
    """The ends of every range pass the checks: what follows is the missing render (or GPU), not the parameters."""
    g = api.Graph(64, 48000)
    g.add_sum("a", 1.0, 0.0)
    g.set_output("a")
    for a in (dict(target_lufs=-60.0, ceiling_dbtp=-30.0, lookahead_ms=0.1, release_ms=1.0),
              dict(target_lufs=0.0, ceiling_dbtp=0.0, lookahead_ms=100.0, release_ms=10000.0)):
        with pytest.raises(api.TermdawError, match="no whole render"):
            g.master(**a)


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="only meaningful on a box without a GPU")
def test_device_mastering_fails_without_a_gpu(api):
    assert api.device_count() == 0
    with pytest.raises(api.TermdawError, match="no HIP device"):
        api.master_f32(np.zeros((48000, 2), np.float32), 48000, -14.0)


@pytest.mark.skipif(shutil.which("g++") is None or not os.path.exists("/opt/rocm/include/hip/hip_runtime_api.h"), reason="needs g++ and the HIP headers")
def test_master_under_sanitizers(tmp_path, tmp_path_factory):
    exe = fx_rig.asan_exe(tmp_path_factory, "asan_master", ["mock_stems.cpp", "mock_master.cpp", "asan_master.cpp"])
    n = int(os.environ.get("TD_ASAN_MASTER_SEEDS", "32"))
    workers = max(1, min(8, os.cpu_count() or 1))
    env = dict(os.environ, **fx_rig.ENV)
    seeds = list(range(n))
    base = str(tmp_path / "p")
    with multiprocessing.Pool(workers) as pool:
        lists = pool.map(L._write_projects, [(base, seeds[i::workers]) for i in range(workers) if seeds[i::workers]])
    procs = [subprocess.Popen([exe] + lst, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for lst in lists]
    mastered = applied = 0
    for p in procs:
        out, err = p.communicate(timeout=1800)
        assert p.returncode == 0, (out[-800:], err[-4000:])
        assert "asan_master done" in out
        mastered += int(out.split(" masterings")[0].split()[-1])
        applied += int(out.split(" signals)")[0].split("(")[-1])
    # (the mock meter never meets the target: every mastering runs its four passes)
    assert mastered >= n and applied >= 4 * mastered, (mastered, applied)
    print("asan_master: %d projects, %d masterings, %d apply signals clean" % (n, mastered, applied))
