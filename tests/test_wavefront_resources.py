"""Register and LDS budgets of the wavefront pass kernels, read from the built
library's code objects (no GPU), as tests/test_kernel_resources.py does for the
measured kernels: no scratch, and three workgroups per CU (a half-tile
re-layout buffer plus the steps' partial-diagonal tables in LDS, 168 VGPRs at
most; dtc_wavefront.hip)."""
import os
import re
import shutil
import subprocess

import pytest

from tests.test_kernel_resources import LIB, LLVM, MAGIC

# dtc_wf_pass<KIND, QM0, SPLIT>: RX / RY kicks, tile 1 (15) and tile 2 (8: bits 0..2 are
# columns), the half-tile re-layouts
KERNELS = ["dtc::dtc_wf_pass<0, 15, true>", "dtc::dtc_wf_pass<0, 8, true>",
           "dtc::dtc_wf_pass<1, 15, true>", "dtc::dtc_wf_pass<1, 8, true>"]
FIELDS = ("private_segment_fixed_size", "group_segment_fixed_size", "vgpr_count")


@pytest.fixture(scope="module")
def wf_kernels(tmp_path_factory):
    """name -> descriptor fields of the dtc_wf_pass kernels.  (In the notes a
    kernel's fields come in alphabetical order, .name in the middle: a kernel's
    record runs from one .args / .agpr_count line to the next.)"""
    tools = [os.path.join(LLVM, t) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf")]
    if not os.path.exists(LIB) or not all(os.path.exists(t) for t in tools) or not shutil.which("c++filt"):
        pytest.skip("built library or ROCm LLVM tools missing")
    objcopy, bundler, readelf = tools
    tmp = str(tmp_path_factory.mktemp("wfres"))
    fat = os.path.join(tmp, "fatbin")
    subprocess.run([objcopy, "--dump-section", ".hip_fatbin=" + fat, LIB, os.path.join(tmp, "lib.so")],
                   check=True, capture_output=True)
    data = open(fat, "rb").read()
    starts = [m.start() for m in re.finditer(re.escape(MAGIC), data)]
    out = {}
    for i, s in enumerate(starts):
        part = os.path.join(tmp, f"bundle{i}")
        with open(part, "wb") as f:
            f.write(data[s:starts[i + 1] if i + 1 < len(starts) else len(data)])
        co = part + ".co"
        r = subprocess.run([bundler, "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                            "--input=" + part, "--output=" + co], capture_output=True)
        if r.returncode != 0 or not os.path.exists(co) or os.path.getsize(co) == 0:
            continue
        notes = subprocess.run([readelf, "--notes", co], capture_output=True, text=True).stdout
        for rec in re.split(r"\n\s+- \.a(?:rgs|gpr_count):", notes):
            m = re.search(r"\n\s+\.name:\s+(_Z\w*dtc_wf_pass\w+)", rec)
            if not m:
                continue
            fields = {k: int(v) for k, v in re.findall(r"\n\s+\.(\w+):\s+(\d+)\s*(?=\n)", rec)
                      if k in FIELDS}
            out[m.group(1)] = fields
    names = list(out)
    dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True,
                         text=True).stdout.splitlines()
    return {d.replace("void ", "").split("(")[0]: out[n] for n, d in zip(names, dem)}


@pytest.mark.parametrize("name", KERNELS)
def test_wavefront_kernel_budgets(wf_kernels, name):
    assert name in wf_kernels, sorted(wf_kernels)
    k = wf_kernels[name]
    assert set(k) == set(FIELDS), k
    assert k["private_segment_fixed_size"] == 0
    assert k["group_segment_fixed_size"] <= 160 * 1024 // 3
    assert k["vgpr_count"] <= 168
