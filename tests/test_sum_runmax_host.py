"""The running-peak fold of a single-pass Normalize tile (termdaw_amd/csrc/sum_runmax.h, shared by k_sum16w's early store and its
final pass) without a GPU: tests/asan_sum_runmax.cpp -- a stand-alone program with its own main -- built with AddressSanitizer /
UBSan and run over seeded timelines (ties, zero peaks, a carried max below, among and above the block peaks, random "seen" subsets
of the lower tiles): the final fold is the plain prefix maximum, and "store again" is raised exactly for the blocks whose running
peak differs."""
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
    out = str(tmp_path_factory.mktemp("asan_sum_runmax") / "asan_sum_runmax")
    subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-I", CSRC, os.path.join(ROOT, "tests", "asan_sum_runmax.cpp"), "-o", out])
    return out


def test_the_final_fold_is_the_prefix_maximum_and_redo_marks_exactly_the_blocks_that_differ(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-400:], r.stderr[-2000:])
    tail = r.stdout.split("asan_sum_runmax done:")[1]
    tiles, redo = (int(tail.split(w)[0].split()[-1]) for w in (" tiles", " blocks to redo"))
    assert tiles > 3 * 20000 * 10 and redo > tiles // 20, tail   # (both outcomes are exercised, neither is rare)
