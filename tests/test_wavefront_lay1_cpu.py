"""The column tile's layout-1 partial diagonal (csrc/dtc_wf_frame.h: register
table over tile bits 3..8, thread table over bits 3, 8..11) on the CPU:
tools/wavefront_lay1_check.cpp builds both table forms from random fields and
bonds and wants, on a 12-bit tile, the same diagonal from either (1e-14), the
staged-and-looked-up pair equal to the X-permuted, Z-signed diagonal (exactly),
and the two-layout program equal to the three-layout snake -- bit for bit where
no odd step carries a diagonal, to 1e-14 otherwise.  Both values of the outside
bit, plain and conjugated factors, RX and RY, 1..4 steps.  Built plain and with
the host sanitizers; a stand-alone binary either way."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "noise-resilience-in-discrete-time-crystal-realizations-on-quantum-computers_amd"


@pytest.mark.parametrize("flags", [["-O1"], ["-O1", "-g", "-fsanitize=address,undefined",
                                             "-fno-sanitize-recover=undefined"]],
                         ids=["plain", "sanitized"])
def test_layout1_tables_equal_three_layout_form(tmp_path, flags):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "wavefront_lay1_check")
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", *flags,
                    "-I", os.path.join(ROOT, PKG, "csrc"),
                    os.path.join(ROOT, "tools", "wavefront_lay1_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "wavefront lay1: ok" in r.stdout
