"""CPU test of the radix-4 / radix-8 x-pass FFT schedule (csrc/xfft_r4.h,
the functions k_fft_x_fwd_r4 and k_fft_x_inv_r4 call):
tests/xfft_r4_host.cpp emulates one wave (64 lanes, an array as its LDS
buffer) under AddressSanitizer and UBSan at h = 256 and h = 512, both
directions, and compares with a double-precision naive DFT; the error must
stay within 2x of a plain radix-2 f32 FFT run on the same inputs. It also
asserts the exchange properties a race would break silently on the GPU
(every slot written exactly once before it is read, all indices inside the
wave's buffer, last stage in register order) and prints the bank-conflict
table DESIGN.md quotes. A stand-alone program: no Python-loaded library,
no GPU."""

import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_xfft_r4_host_sanitized(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler for the sanitizer program")
    exe = str(tmp_path / "xfft_r4_host")
    subprocess.run(
        [cxx, "-O1", "-g", "-std=c++17", "-Wall",
         "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
         # runtimes linked in: the program stands alone at load time
         "-static-libasan", "-static-libubsan",
         os.path.join(ROOT, "tests", "xfft_r4_host.cpp"), "-o", exe],
        check=True, cwd=ROOT)
    p = subprocess.run([exe], capture_output=True, text=True)
    out = p.stdout + p.stderr
    print(out)
    assert p.returncode == 0, out
    assert "Sanitizer" not in out and "runtime error" not in out, out
    assert " 0 failures" in p.stdout, out
