"""The tile deal of the late-issue main kernel (beatrice_amd/csrc/bt_tail_split.h) on the host:
tests/cpp/tail_split_check.cpp as a stand-alone program under AddressSanitizer and
UndefinedBehaviorSanitizer. It checks that the waves' static shares and the tail's tickets deal
every tile of [0, ntiles) exactly once and that every ticket maps inside the tail, for ntiles = 0,
1, fewer tiles than waves, at most the tail, no multiple of the claim, 8 and 2,048 waves, every
(rounds, claim) pair of the sweep, and the largest batch the ABI can name. (Every launch claims
from heads that start at 0 — its predecessor on the stream zeroed them — so there is no ticket
base to wrap.)"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("tail_split") / "tail_split_check")
    # the sanitizer runtimes linked into the program: it runs the same whatever else a process preloads
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan", "-I" + os.path.join(ROOT, "beatrice_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "tail_split_check.cpp"), "-o", exe], check=True)
    return exe


def test_tail_split_partitions_every_shape(check_exe):
    r = subprocess.run([check_exe], capture_output=True, text=True)
    assert r.returncode == 0 and "shapes ok" in r.stdout, r.stdout + r.stderr


@pytest.mark.parametrize("ntiles,waves", [(0, 8), (1, 8), (7, 8), (25, 8), (100, 8), (101, 8), (262144, 2048),
                                          (262143, 2048), (2047, 2048)])
def test_tail_split_adopted_pair(check_exe, ntiles, waves):
    """The adopted (rounds, claim) pair on the GPU test's batches and the benchmark's."""
    r = subprocess.run([check_exe, str(ntiles), str(waves)], capture_output=True, text=True)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout + r.stderr
