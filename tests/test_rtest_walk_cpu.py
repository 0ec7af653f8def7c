"""CPU test of the r-test's 16-byte row walk (csrc/rtest_walk.h, the
arithmetic k_rtest_wide runs): tests/rtest_walk_host.cpp walks heap buffers
of exactly n*2 bytes rounded up to 16 under AddressSanitizer and UBSan and
compares the five sums with a naive triple loop, over view widths 37 and
40, ox in {0, 1, 3}, every sx residue mod 8 in both signs, nx 1..20 and
boxes touching the first and last voxel of either buffer. A stand-alone
program: no Python-loaded library, no GPU."""

import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_rtest_walk_host_sanitized(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler for the sanitizer program")
    exe = str(tmp_path / "rtest_walk_host")
    subprocess.run(
        [cxx, "-O1", "-g", "-std=c++17", "-Wall",
         "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
         # runtimes linked in: the program stands alone at load time
         "-static-libasan", "-static-libubsan",
         os.path.join(ROOT, "tests", "rtest_walk_host.cpp"), "-o", exe],
        check=True, cwd=ROOT)
    p = subprocess.run([exe], capture_output=True, text=True)
    out = p.stdout + p.stderr
    assert p.returncode == 0, out
    assert "Sanitizer" not in out and "runtime error" not in out, out
    assert " 0 failures" in p.stdout, out
