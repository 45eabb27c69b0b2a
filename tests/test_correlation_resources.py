"""The correlator kernels in the built library's gfx950 code objects (no GPU):
both are there and neither uses scratch -- the chunk kernel is a streaming read
whose sixteen amplitudes and their transform must stay in registers."""
import pytest

from tests.test_kernel_resources import _kernels

KERNELS = ("dtc::corr_chunk_kernel", "dtc::corr_reduce_kernel")


@pytest.mark.parametrize("name", KERNELS)
def test_correlator_kernels_present_without_scratch(name):
    k = _kernels()
    assert name in k, sorted(n for n in k if "corr" in n)
    assert k[name].get("private_segment_fixed_size", 0) == 0, k[name]
