"""CPU test of the r-test's 8-bit dot-product sums (csrc/rtest_dot.h, the
arithmetic k_rtest_dot runs): tests/rtest_dot_host.cpp walks heap buffers of
exactly n*2 bytes rounded up to 16 under AddressSanitizer and UBSan, on the
hoisted path (row strides multiples of 8) and the per-row path, and compares
the five sums with a naive u64 triple loop over view widths 37 and 40, ox in
{0, 1, 3}, every sx residue mod 8 in both signs, nx 1..20, boxes touching
the first and last voxel of either buffer, and all-65535 data. It also
checks the byte-permute selectors on a known pattern and the overflow
bound: 4128 all-65535 chunks accumulate exactly, the next one does not fit,
and the kernel's widening guard covers it. A stand-alone program: no
Python-loaded library, no GPU."""

import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_rtest_dot_host_sanitized(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler for the sanitizer program")
    exe = str(tmp_path / "rtest_dot_host")
    subprocess.run(
        [cxx, "-O1", "-g", "-std=c++17", "-Wall",
         "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
         # runtimes linked in: the program stands alone at load time
         "-static-libasan", "-static-libubsan",
         os.path.join(ROOT, "tests", "rtest_dot_host.cpp"), "-o", exe],
        check=True, cwd=ROOT)
    p = subprocess.run([exe], capture_output=True, text=True)
    out = p.stdout + p.stderr
    assert p.returncode == 0, out
    assert "Sanitizer" not in out and "runtime error" not in out, out
    assert " 0 failures" in p.stdout, out
    assert "(0 hoisted)" not in p.stdout, out
