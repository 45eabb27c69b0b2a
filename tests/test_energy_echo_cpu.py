"""The energy echo without a GPU: the two C entry points' argument checks, the
``echo`` flag's way through energy.py / energy_cli, and the register and LDS
budgets of the kernels its schedule launches at L = 20 (read from the built
library's code objects, as tests/test_kernel_resources.py does)."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests.helpers import random_disorder
from tests.test_kernel_resources import LIB, LLVM, MAGIC


@pytest.mark.parametrize("name", ["dtc_energy_echo", "dtc_energy_echo_sums"])
def test_symbols_and_null_arguments(pkg, name):
    """Exported, and a null-argument call fails with -1 and a message before
    any device call (no context exists here)."""
    assert name in pkg._capi.EXPORTED_SYMBOLS
    lib = pkg._capi.load_library()
    fn = getattr(lib, name)
    rc = fn(None, None, None, ctypes.c_uint64(1), ctypes.c_int64(0), ctypes.c_int32(1), None,
            None, None)
    assert rc == -1
    assert b"null" in lib.dtc_last_error()


class _StubEngine:
    """Records which sums method a driver called; returns zeros of the right shapes."""

    def __init__(self):
        self.calls = []

    def _sums(self, name, spec, n_traj, **kw):
        self.calls.append((name, n_traj, kw))
        T, L, n = spec.T, spec.L, spec.n_inst
        return {"z": np.zeros((n, T, L)), "zz": np.zeros((n, T, L - 1)), "x": np.zeros((n, T, L))}

    def energy_sums(self, spec, n_traj, **kw):
        return self._sums("energy_sums", spec, n_traj, **kw)

    def energy_sums_bond(self, spec, n_traj, **kw):
        return self._sums("energy_sums_bond", spec, n_traj, **kw)

    def energy_echo_sums(self, spec, n_traj, **kw):
        return self._sums("energy_echo_sums", spec, n_traj, **kw)


def _spec(pkg, **kw):
    hs, phis = random_disorder(np.random.default_rng(1), 5, 2)
    return pkg.energy.energy_spec(5, 4, hs, phis, 0.95, "neel", **kw)


def test_get_instances_energy_echo_flag(pkg):
    en = pkg.energy
    stub = _StubEngine()
    out = en.get_instances_energy(_spec(pkg), 16, ("full", "z_zz"), engine=stub, echo=True)
    assert [c[0] for c in stub.calls] == ["energy_echo_sums"]
    assert out["full"].shape == (2, 4) and set(out) == {"full", "z_zz"}
    stub = _StubEngine()
    en.get_instances_energy(_spec(pkg), 16, engine=stub)
    en.get_instances_energy(_spec(pkg), 16, engine=stub, echo=False)
    en.get_instances_energy(_spec(pkg, bond_noise=0.01), 16, engine=stub)
    assert [c[0] for c in stub.calls] == ["energy_sums", "energy_sums", "energy_sums_bond"]


def test_run_energy_echo_flag(pkg):
    en = pkg.energy
    hs, phis = random_disorder(np.random.default_rng(2), 5, 1)
    stub = _StubEngine()
    res = en.run_energy(5, 0.95, hs, phis, 4, nprobs=(0, 0.01), n_traj=8, engine=stub, echo=True)
    assert [c[0] for c in stub.calls] == ["energy_echo_sums"] * 2
    assert set(res) == {("full", 0), ("full", 0.01)}
    stub = _StubEngine()
    en.run_energy(5, 0.95, hs, phis, 4, nprobs=(0, 0.01), n_traj=8, engine=stub)
    assert [c[0] for c in stub.calls] == ["energy_sums"] * 2
    stub = _StubEngine()
    e = en.run_energy_device(5, 0.95, hs, phis, 4, None, engine=stub, echo=True)
    assert [c[0] for c in stub.calls] == ["energy_echo_sums"] and e.shape == (4,)


def test_echo_refusals_without_a_device(pkg):
    """The refusals are raised before any engine is touched."""
    en = pkg.energy
    hs, phis = random_disorder(np.random.default_rng(3), 5, 1)
    stub = _StubEngine()
    with pytest.raises(NotImplementedError, match="bond noise"):
        en.get_instances_energy(_spec(pkg, bond_noise=0.02), 4, engine=stub, echo=True)
    with pytest.raises(NotImplementedError, match="bond noise"):
        en.run_energy(5, 0.95, hs, phis, 4, nprobs=(0.01,), n_traj=4, engine=stub, echo=True,
                      bond_noise=0.02)
    cal = pkg.device_noise.DeviceCalibration.from_json(pkg.cli.DEFAULT_CALIBRATION)
    with pytest.raises(NotImplementedError, match="device-like noise"):
        en.run_energy(5, 0.95, hs, phis, 4, nprobs=(0.01,), n_traj=4, engine=stub, echo=True,
                      calibration=cal)
    with pytest.raises(NotImplementedError, match="device-like noise"):
        en.run_energy_device(5, 0.95, hs, phis, 4, cal, engine=stub, echo=True)
    assert stub.calls == []


def test_energy_csv_name_echo(pkg):
    args = ("energy_data", "neel", 0.97, 5, 1, 1, 0.0, 1.0, 0.05, 1)
    plain = pkg.energy.energy_csv_name(*args)
    assert pkg.energy.energy_csv_name(*args, echo=False) == plain
    assert pkg.energy.energy_csv_name(*args, echo=True) == plain[:-4] + "_echo.csv"
    p = pkg.energy_cli.build_parser()
    assert p.parse_args([]).echo == 0 and p.parse_args(["--echo", "1"]).echo == 1


# L = 20 in the 12 / 8 plan: nibble sets 7 and 6; kick families RX (0), RY (1) and
# general (2).  dtc_xend_pass<SHAPE, NIBS, KIND>: a group's end is a K-D-K (3) or the
# trailing kick-only pass (0).  The forward is unmeasured (MC 0): its dual passes,
# and the plain and wavefront passes of the interior.
XEND = [f"dtc::dtc_xend_pass<{s}, {n}, {k}>" for s in (0, 3) for n in (6, 7) for k in (0, 1, 2)]
# (plain K-D-K: the 12-site group runs at three workgroups per CU, the 8-site at two)
TWO_PER_CU = XEND + [f"dtc::dtc_kdk_dual<{n}, {k}, 0, 0>" for n in (6, 7) for k in (0, 1, 2)] + [
    f"dtc::dtc_kdk_pass<6, {k}, 0, 0>" for k in (0, 1, 2)] + [
    f"dtc::dtc_kick_pass<{n}, {k}, 0, 0>" for n in (6, 7) for k in (0, 1, 2)]
THREE_PER_CU = [f"dtc::dtc_kdk_pass3<7, {k}, 0, 0>" for k in (0, 1, 2)] + [
    "dtc::dtc_wf_pass<0, 15, true>", "dtc::dtc_wf_pass<0, 8, true>",
    "dtc::dtc_wf_pass<1, 15, true>", "dtc::dtc_wf_pass<1, 8, true>"]


FIELDS = ("private_segment_fixed_size", "group_segment_fixed_size", "vgpr_count")


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    """Demangled name -> descriptor fields of the library's dtc kernels, read the
    way tests/test_wavefront_resources.py does (a kernel's record in the notes
    runs from one .args / .agpr_count line to the next, .name in the middle)."""
    tools = [os.path.join(LLVM, t) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf")]
    if not os.path.exists(LIB) or not all(os.path.exists(t) for t in tools) or not shutil.which("c++filt"):
        pytest.skip("built library or ROCm LLVM tools missing")
    objcopy, bundler, readelf = tools
    tmp = str(tmp_path_factory.mktemp("echores"))
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
            m = re.search(r"\n\s+\.name:\s+(_Z\w*dtc\w+)", rec)
            if not m:
                continue
            out[m.group(1)] = {k: int(v) for k, v in re.findall(r"\n\s+\.(\w+):\s+(\d+)\s*(?=\n)", rec)
                               if k in FIELDS}
    if not out:
        pytest.skip("no gfx950 code objects found in the library")
    names = list(out)
    dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True,
                         text=True).stdout.splitlines()
    return {d.replace("void ", "").split("(")[0]: out[n] for n, d in zip(names, dem)}


@pytest.mark.parametrize("name,per_cu", [(n, 2) for n in TWO_PER_CU] + [(n, 3) for n in THREE_PER_CU])
def test_echo_energy_kernel_budgets(kernels, name, per_cu):
    """No scratch, and the workgroups per CU of the kernel's launch bounds: 512
    VGPRs per SIMD lane and 160 KiB of LDS per CU, shared by that many
    256-thread workgroups (one wave of each per SIMD)."""
    assert name in kernels, [n for n in sorted(kernels) if "xend" in n]
    k = kernels[name]
    assert set(k) == set(FIELDS), k
    assert k["private_segment_fixed_size"] == 0, k
    assert k["vgpr_count"] <= 512 // per_cu - (512 // per_cu) % 8, k
    assert k["group_segment_fixed_size"] <= 160 * 1024 // per_cu, k
