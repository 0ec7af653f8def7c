"""CPU test of the strided-pass radix-8 FFT schedule at n = 512
(csrc/sfft_r8.h, the functions k_fft_pass_r8 and k_fft_z_fused_r8x call):
tests/sfft_r8_host.cpp emulates one workgroup (256 threads as loops, the
exchange tile as a heap array of the kernel's size) under AddressSanitizer
and UBSan. It checks the y pass in both directions and the fused z chain
against double precision, with the error of a plain radix-2 f32 FFT on the
same input as the bar (2x), at valid = 512, 300, 1 and tiles of 8, 3 and 1
live columns, unequal valid_a / valid_b and a column below the cross-power
guard (exactly 0). It asserts the exchange properties a race would break
silently on the GPU (every slot written exactly once before it is read, all
indices inside the tile, inside the owner wave's slice for the wave-private
exchanges, first and last stage in the I/O order) and prints the
bank-conflict table DESIGN.md quotes. A stand-alone program: no
Python-loaded library, no GPU."""

import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sfft_r8_host_sanitized(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler for the sanitizer program")
    exe = str(tmp_path / "sfft_r8_host")
    subprocess.run(
        [cxx, "-O1", "-g", "-std=c++17", "-Wall",
         "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
         # runtimes linked in: the program stands alone at load time
         "-static-libasan", "-static-libubsan",
         os.path.join(ROOT, "tests", "sfft_r8_host.cpp"), "-o", exe],
        check=True, cwd=ROOT)
    p = subprocess.run([exe], capture_output=True, text=True)
    out = p.stdout + p.stderr
    print(out)
    assert p.returncode == 0, out
    assert "Sanitizer" not in out and "runtime error" not in out, out
    assert " 0 failures" in p.stdout, out
