"""The item walk of the lean m = 1 pair kernel (any4_amd/csrc/pair_walk.h: operand bases moved by increments) against the division-based
decode of the general kernel, on the host: tests/native/pair_walk_check.cpp is a stand-alone program, built here with AddressSanitizer and
UndefinedBehaviorSanitizer and run once.  No GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pair_walk_matches_decode(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler found (g++ / clang++ / c++)")
    exe = str(tmp_path / "pair_walk_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "native", "pair_walk_check.cpp"), "-o", exe], check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "items equal to the division-based decode" in r.stdout
