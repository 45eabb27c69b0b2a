"""Four workgroups per CU for the wavefront pass (DTC_WF_WG4;
csrc/dtc_wavefront.hip), read from the built library's code objects like
tests/test_wavefront_resources.py (no GPU).  Adopted for tile 1, the
`<..., 15, true>` kernels: no scratch, a quarter of a CU's 160 KiB of LDS at
most -- the half-tile re-layout buffer plus the steps' per-register tables; the
thread-constant entries come straight from the global table -- and at most 128
VGPRs, the budget of four waves per SIMD.  The column tile, `<..., 8, true>`,
measured slower at four per CU and stays at three
(profiles/r10_wavefront_wg4_ab20.txt): the same code, so no scratch and the
same VGPR budget, with the LDS bound of three workgroups."""
import pytest

from tests.test_wavefront_resources import FIELDS, KERNELS, wf_kernels  # noqa: F401 (fixture)


@pytest.mark.parametrize("name", KERNELS)
def test_wavefront_kernels_fit_four_workgroups(wf_kernels, name):  # noqa: F811
    assert name in wf_kernels, sorted(wf_kernels)
    k = wf_kernels[name]
    assert set(k) == set(FIELDS), k
    print(name, k)
    tile1 = ", 15, " in name
    assert k["private_segment_fixed_size"] == 0
    assert k["group_segment_fixed_size"] <= 160 * 1024 // (4 if tile1 else 3)
    assert k["vgpr_count"] <= 128
