"""The index arithmetic of the wide packed sum's quad shape (termdaw_amd/csrc/sum_index.h, shared by sum_terms16w, the sample
loader and the ceiling micro-benchmark) without a GPU: tests/asan_sum_index.cpp -- a stand-alone program with its own main -- built
with AddressSanitizer / UBSan and run over every loop length 1 .. 1 100, a few thousand seeded ones up to 2^26 and starts from the
whole 32-bit range."""
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
    out = str(tmp_path_factory.mktemp("asan_sum_index") / "asan_sum_index")
    subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-I", CSRC, os.path.join(ROOT, "tests", "asan_sum_index.cpp"), "-o", out])
    return out


def test_start_step_and_wrap_agree_with_plain_modulo_and_stay_inside_the_table(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-400:], r.stderr[-2000:])
    tail = r.stdout.split("asan_sum_index done:")[1]
    lens, starts = (int(tail.split(w)[0].split()[-1]) for w in (" lengths", " starts"))
    assert lens >= 1100 + 3000 and starts > 1000 * lens, tail


def test_the_loop_lengths_the_gpu_tests_use(exe):
    """1 .. 3 and the lengths around 255 / 256 (tests/test_gpu_sum_scalar_index.py): a loop shorter than the pad repeats in it."""
    r = subprocess.run([exe, "1", "258"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-400:], r.stderr[-2000:])
    assert " 258 lengths" in r.stdout, r.stdout
