"""Program and Pauli frame of the 12-bit K-D-K passes (csrc/dtc_pass_frame.h:
pass_program, which pass_body reads at compile time, and frame12_walk, the walk
the prep kernel runs per state) on the CPU: tools/pass_frame_check.cpp applies
a pass to a 4096-amplitude tile directly (each kick's 2x2 matrix, a random
diagonal) and in frame form as pass_body runs it (form-B butterflies with the
walk's coefficients, the tile index-permuted by each named re-layout's masks,
the Z sign at the diagonal point, i^ph) and wants the two tiles within 1e-12:
RX and RY, nibble sets 1..7, pre-only / post-only / both, with and without the
diagonal, the dual pass's echo branch, every variant on every kicked bit (the
program asserts that coverage itself), and the masks off their side's register
nibble.  Built plain and with the host sanitizers; a stand-alone binary either
way."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "noise-resilience-in-discrete-time-crystal-realizations-on-quantum-computers_amd"


@pytest.mark.parametrize("flags", [["-O1"], ["-O1", "-g", "-fsanitize=address,undefined",
                                             "-fno-sanitize-recover=undefined"]],
                         ids=["plain", "sanitized"])
def test_frame_form_equals_direct(tmp_path, flags):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "pass_frame_check")
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", *flags,
                    "-I", os.path.join(ROOT, PKG, "csrc"),
                    os.path.join(ROOT, "tools", "pass_frame_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "pass frames: ok" in r.stdout
