"""The block density-matrix kernels in the built library's gfx950 code objects
(no GPU): all three are there, none uses scratch -- the Gram kernel's sixteen
loaded amplitudes, its MFMA operands and accumulators must stay in registers -- and the
Gram kernel's LDS and registers leave room for two workgroups of eight waves
per CU."""
import glob
import os
import re
import subprocess

import pytest

from tests.test_kernel_resources import LLVM, ROOT, _kernels

KERNELS = ("dtc::rdm_block_gram_kernel", "dtc::rdm_block_finish_kernel",
           "dtc::rdm_block_purity_kernel")


@pytest.mark.parametrize("name", KERNELS)
def test_block_kernels_present_without_scratch(name):
    k = _kernels()
    assert name in k, sorted(n for n in k if "rdm" in n)
    assert k[name].get("private_segment_fixed_size", 0) == 0, k[name]
    # 512 registers per SIMD lane; at most 256 per wave
    assert k[name]["vgpr_count"] <= 256


def test_gram_kernel_fits_two_workgroups_per_cu():
    k = _kernels()["dtc::rdm_block_gram_kernel"]
    # two workgroups of eight waves: four waves per SIMD, 128 registers each
    assert k["vgpr_count"] <= 128


def _lds_bytes():
    """{mangled kernel name: LDS bytes} of the code objects _kernels() unbundled
    (the metadata lists a kernel's .group_segment_fixed_size before its .name)."""
    _kernels()
    out = {}
    for co in glob.glob(os.path.join(ROOT, "build", "kres", "bundle*.co")):
        notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co],
                               capture_output=True, text=True).stdout
        lds = None
        for line in notes.splitlines():
            m = re.match(r"\s+-?\s*\.(name|group_segment_fixed_size):\s+(\S+)", line)
            if not m:
                continue
            if m.group(1) == "group_segment_fixed_size":
                lds = int(m.group(2))
            elif lds is not None and m.group(2).startswith("_Z"):
                out[m.group(2)] = lds
                lds = None
    return out


def test_block_kernels_lds():
    lds = {n: v for n, v in _lds_bytes().items() if "rdm_block" in n}
    assert len(lds) == 3, lds
    for name, v in lds.items():
        assert v <= 80 * 1024, (name, v)
    gram = [v for n, v in lds.items() if "rdm_block_gram_kernel" in n]
    # the two 64 x 64 panels
    assert gram == [2 * 64 * 64 * 8]
