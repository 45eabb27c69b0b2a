"""The density-matrix kernels in the built library's gfx950 code objects (no
GPU): both are there, neither uses scratch -- the Gram kernel's sixteen
amplitudes, its MFMA operands and accumulators must stay in registers -- and
the Gram kernel's LDS leaves room for at least two workgroups per CU."""
import pytest

from tests.test_kernel_resources import _kernels

KERNELS = ("dtc::rdm_gram_kernel", "dtc::rdm_reduce_kernel")


@pytest.mark.parametrize("name", KERNELS)
def test_rdm_kernels_present_without_scratch(name):
    k = _kernels()
    assert name in k, sorted(n for n in k if "rdm" in n)
    assert k[name].get("private_segment_fixed_size", 0) == 0, k[name]


def test_gram_kernel_fits_two_workgroups_per_cu():
    k = _kernels()["dtc::rdm_gram_kernel"]
    # 160 KiB of LDS per CU; 512 VGPRs per SIMD lane, one wave of a workgroup per SIMD
    assert k["group_segment_fixed_size"] <= 160 * 1024 // 2
    assert k["vgpr_count"] <= 256
