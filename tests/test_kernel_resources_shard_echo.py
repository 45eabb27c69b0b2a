"""The measure-only end of a sharded echo chain (dtc_kick_sites_final) within
the budget tests/test_kernel_resources.py holds its siblings to, read from the
same built code objects (no GPU): every instantiation the launcher can pick is
present and none spills to scratch -- at its two workgroups of 256 threads per
CU (two waves per SIMD) that is 256 VGPRs per lane."""
import pytest

from tests.test_kernel_resources import _kernels

NIBS = (4, 6, 7)       # the register-nibble sets of the plan's site groups
KINDS = (0, 1, 2)      # RX, RY, general: the unitary kick kinds a shard runs


@pytest.fixture(scope="module")
def kernels():
    return _kernels()


@pytest.mark.parametrize("nibs", NIBS)
@pytest.mark.parametrize("kind", KINDS)
def test_sites_final_does_not_spill(kernels, nibs, kind):
    name = f"dtc::dtc_kick_sites_final<{nibs}, {kind}>"
    assert name in kernels, name
    k = kernels[name]
    assert not k.get("private_segment_fixed_size"), k
    assert k["vgpr_count"] <= 256
