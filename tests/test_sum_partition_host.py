"""The partition arithmetic of the ragged packed sum (termdaw_amd/csrc/sum_partition.h, shared by k_sum16r and its host side)
without a GPU: tests/asan_sum_partition.cpp -- a stand-alone program with its own main -- built with AddressSanitizer / UBSan and run
over every timeline of 16 .. 20 000 quads and the admissible grids."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "termdaw_amd", "csrc")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    out = str(tmp_path_factory.mktemp("asan_sum_partition") / "asan_sum_partition")
    subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-I", CSRC, os.path.join(ROOT, "tests", "asan_sum_partition.cpp"), "-o", out])
    return out


def test_partition_tiles_evenly_for_every_timeline_and_grid(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-400:], r.stderr[-2000:])
    tail = r.stdout.split("asan_sum_partition done:")[1]
    grids, groups, straddles = (int(tail.split(w)[0].split()[-1]) for w in (" grids", " workgroups", " straddled"))
    assert grids > 100000 and groups > grids and straddles > 0, tail


def test_the_sizes_the_gpu_tests_use(exe):
    """One second is 188 quads: 47, 40, 13 and 12 workgroups are admissible, 11 and 48 are not (tests/test_gpu_sum_ragged.py)."""
    r = subprocess.run([exe, "188", "188"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.stdout[-400:], r.stderr[-2000:])
    # 188 / 16 = 11.75 -> at least 12 workgroups; 188 / 4 = 47 -> at most 47: 36 grids
    assert " 36 grids" in r.stdout, r.stdout
