"""Block density matrices, the host side (no GPU): the contract's reference
dtc_rdm_block_state against numpy reshape-and-matmul, every DTC_EINVAL case, the
Gram kernel's index algebra (a numpy restatement on the contract's shapes and the
header itself walked exhaustively by tools/rdm_block_geometry_check.cpp), the
choice of blocks of entanglement_profile, refusals and the command line."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import rdm_block_model as bm
from tests import rdm_model as rm
from tests.helpers import harsh_device, random_disorder

SHAPES = [(10, 0, 5), (10, 5, 5), (10, 2, 5), (13, 3, 6), (16, 8, 8), (20, 0, 10), (20, 10, 10)]


def _random_state(L, seed):
    rng = np.random.default_rng(seed)
    psi = rng.normal(size=1 << L) + 1j * rng.normal(size=1 << L)
    return psi / np.linalg.norm(psi)


@pytest.mark.parametrize("L,start,k", SHAPES)
def test_block_state_matches_numpy(pkg, L, start, k):
    psi = _random_state(L, 700 + L + start)
    rho, pur = pkg.engine.rdm_block_state(psi, L, start, k)
    want = rm.state_rdm(psi, L, list(range(start, start + k)))
    assert rho.shape == (1 << k, 1 << k) and rho.dtype == np.complex128
    err = float(np.max(np.abs(rho - want)))
    perr = abs(pur - float((want.real ** 2 + want.imag ** 2).sum()))
    print(f"L={L} start={start} k={k}: rho deviates by {err:.3e}, purity by {perr:.3e}")
    assert err <= 1e-12 and perr <= 1e-12
    assert np.array_equal(rho, rho.conj().T)
    assert np.all(np.diag(rho).imag == 0.0)
    assert abs(np.trace(rho).real - 1.0) <= 1e-12
    assert 2.0 ** -k < pur <= 1.0 + 1e-12


@pytest.mark.parametrize("L", [10, 12, 16, 20])
def test_block_state_halves_have_one_purity(pkg, L):
    """A pure state's two halves have the same spectrum."""
    psi = _random_state(L, 740 + L)
    k = L // 2
    lo = pkg.engine.rdm_block_state(psi, L, 0, k)[1]
    hi = pkg.engine.rdm_block_state(psi, L, k, k)[1]
    print(f"L={L}: purities {lo:.15f} {hi:.15f}")
    assert abs(lo - hi) <= 1e-12


def test_block_state_basis_and_product_states(pkg):
    L, k = 12, 6
    psi = np.zeros(1 << L, dtype=np.complex128)
    psi[0xA5C] = 1.0
    for start in (0, 3, 6):
        rho, pur = pkg.engine.rdm_block_state(psi, L, start, k)
        want = np.zeros((64, 64), dtype=np.complex128)
        al = (0xA5C >> start) & 63
        want[al, al] = 1.0
        assert np.array_equal(rho, want) and pur == 1.0
    # a product of two random halves: pure halves, a mixed straddling block
    a, b = _random_state(6, 1), _random_state(6, 2)
    psi = np.kron(b, a)     # site i = bit i: a on sites 0..5
    assert abs(pkg.engine.rdm_block_state(psi, L, 0, 6)[1] - 1.0) <= 1e-12
    assert abs(pkg.engine.rdm_block_state(psi, L, 6, 6)[1] - 1.0) <= 1e-12
    rho, pur = pkg.engine.rdm_block_state(psi, L, 0, 6)
    assert np.max(np.abs(rho - np.outer(a, a.conj()))) <= 1e-12
    assert pkg.engine.rdm_block_state(psi, L, 3, 6)[1] < 0.9


def test_block_einval(pkg):
    """Every DTC_EINVAL case of the contract that needs no device."""
    lib = pkg._capi.load_library()
    dp = pkg._capi.as_dptr
    L = 12
    psi = np.zeros(2 << L)
    psi[0] = 1.0
    rho = np.zeros(2 << 20)
    pur = np.zeros(1)
    assert lib.dtc_rdm_block_state(dp(psi), L, 0, 5, dp(rho), dp(pur)) == 0
    assert lib.dtc_rdm_block_state(dp(psi), L, 7, 5, None, dp(pur)) == 0   # rho is optional
    assert pur[0] == 1.0
    bad = [
        (None, L, 0, 5, dp(rho), dp(pur)),      # null state
        (dp(psi), L, 0, 5, dp(rho), None),      # null purity
        (dp(psi), L, 0, 4, dp(rho), dp(pur)),   # k < 5
        (dp(psi), L, 0, 11, dp(rho), dp(pur)),  # k > 10
        (dp(psi), L, 0, 7, dp(rho), dp(pur)),   # 2 k > L
        (dp(psi), 9, 0, 5, dp(rho), dp(pur)),   # 2 k > L
        (dp(psi), L, -1, 5, dp(rho), dp(pur)),  # start < 0
        (dp(psi), L, 8, 5, dp(rho), dp(pur)),   # start + k > L
        (dp(psi), 33, 0, 5, dp(rho), dp(pur)),  # L > 32
        (dp(psi), 0, 0, 5, dp(rho), dp(pur)),   # L < 1
    ]
    for args in bad:
        assert lib.dtc_rdm_block_state(*args) == -1, args[1:4]
        assert lib.dtc_last_error()
    # dtc_rdm_block_sums: null arguments fail before any device call
    for name in ("dtc_rdm_block_sums", "dtc_rdm_block_state"):
        assert name in pkg._capi.EXPORTED_SYMBOLS and hasattr(lib, name)
    rc = lib.dtc_rdm_block_sums(None, None, None, ctypes.c_uint64(1), ctypes.c_int64(0),
                                ctypes.c_int32(1), None, ctypes.c_int32(1), ctypes.c_int32(5),
                                None, None)
    assert rc == -1 and b"null" in lib.dtc_last_error()
    with pytest.raises(pkg._capi.DtcError):
        pkg.engine.rdm_block_state(psi[::2] + 0j, L, 8, 5)
    with pytest.raises(ValueError):
        pkg.engine.rdm_block_state(np.zeros(7), 3, 0, 5)


@pytest.mark.parametrize("L,start,k", SHAPES)
def test_index_algebra_numpy(L, start, k):
    """Every (row, column) pair is a distinct amplitude, together they are the
    whole state, the block's bits are the row, and every staged load of the Gram
    kernel is 64 consecutive amplitudes inside one aligned run of 64."""
    L_eff = max(L, 12)
    ae, ke, m = bm.geometry(start, k, L_eff)
    assert 0 <= ae and ae + ke <= L_eff
    rows = np.arange(1 << ke)[:, None]
    cols = np.arange(1 << (L_eff - ke))[None, :]
    x = bm.amp_index(ae, ke, rows, cols)
    assert x.min() == 0 and x.max() == (1 << L_eff) - 1
    assert np.unique(x).size == 1 << L_eff
    # the block's own bits, in the block's order, are in the row index
    alpha = (x >> start) & ((1 << k) - 1)
    shift = start - ae
    assert np.array_equal(alpha, np.broadcast_to((rows >> shift) & ((1 << k) - 1), x.shape))
    n_panels, n_chunks = (1 << ke) // 64, (1 << (L_eff - ke)) // 64
    seen = np.zeros(1 << L_eff, dtype=np.int32)
    for p in sorted({0, n_panels - 1}):
        for c in sorted({0, n_chunks // 2, n_chunks - 1}):
            loads = bm.staged_loads(start, k, L_eff, p, c)
            assert loads.shape == (64, 64)
            assert np.all(loads[:, 0] % 64 == 0)
            assert np.array_equal(loads, loads[:, :1] + np.arange(64)[None, :])
            want = bm.amp_index(ae, ke, p * 64 + np.arange(64)[:, None],
                                c * 64 + np.arange(64)[None, :])
            assert np.array_equal(np.sort(loads.ravel()), np.sort(want.ravel()))
            seen[loads.ravel()] += 1
    assert seen.max() == 1


def test_kernel_index_algebra_header(tmp_path):
    """tools/rdm_block_geometry_check.cpp walks the Gram kernel's addressing with
    csrc/dtc_rdm_block.h for every block of L_eff = 12 .. 20."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "rdm_block_geometry_check")
    pkg_dir = "noise-resilience-in-discrete-time-crystal-realizations-on-quantum-computers_amd"
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-O2", "-I",
                    os.path.join(root, pkg_dir, "csrc"),
                    os.path.join(root, "tools", "rdm_block_geometry_check.cpp"), "-o", exe],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout.strip())
    assert r.returncode == 0, (r.stdout[-400:], r.stderr[-400:])
    assert r.stdout.split()[:2] == ["cases", "383"] and r.stdout.split()[-1] == "0"


def test_profile_blocks(pkg):
    en = pkg.entanglement
    assert en.profile_blocks(2) == [(0, 1)]
    assert en.profile_blocks(5) == [(0, 1), (0, 2), (3, 2), (4, 1)]
    assert en.profile_blocks(11) == [(0, 1), (0, 2), (0, 3), (0, 4), (0, 5), (6, 5), (7, 4),
                                     (8, 3), (9, 2), (10, 1)]
    for L in (2, 7, 12, 20, 21):
        blocks = en.profile_blocks(L)
        assert len(blocks) == L - 1
        for cut, (a, k) in enumerate(blocks, start=1):
            # one side of the cut, the smaller one; a block the library takes
            assert (a, k) in ((0, cut), (cut, L - cut))
            assert k == min(cut, L - cut) and 2 * k <= L and k <= 10
    for L in (22, 23, 32):
        with pytest.raises(ValueError, match="more than the 10"):
            en.profile_blocks(L)


class _StubEngine:
    def __getattr__(self, name):
        raise AssertionError("the engine must not be reached")


def test_refusals_without_a_device(pkg):
    L = 12
    hs, phis = random_disorder(np.random.default_rng(3), L, 1)
    dev = pkg.SweepSpec(L=L, T=4, hs=hs, phis=phis, device=harsh_device(pkg, L))
    bond = pkg.SweepSpec(L=L, T=4, hs=hs, phis=phis, bond_noise=0.02)
    bare = pkg.DtcEngine.__new__(pkg.DtcEngine)
    stub = _StubEngine()
    for spec, word in ((dev, "device-like noise"), (bond, "bond noise")):
        with pytest.raises(NotImplementedError, match=word):
            bare.rdm_block_sums(spec, 2, [(0, 5)])
        with pytest.raises(NotImplementedError, match=word):
            pkg.entanglement.get_instances_block(spec, 2, [(0, 5)], engine=stub)
        with pytest.raises(NotImplementedError, match=word):
            pkg.entanglement.entanglement_profile(spec, 2, engine=stub)
    ok = pkg.SweepSpec(L=L, T=4, hs=hs, phis=phis)
    for bad in ([(0, 4)], [(0, 11)]):
        with pytest.raises(ValueError, match="block size"):
            bare.rdm_block_sums(ok, 2, bad)
    with pytest.raises(ValueError, match="share one size"):
        bare.rdm_block_sums(ok, 2, [(0, 5), (0, 6)])
    with pytest.raises(ValueError):
        bare.rdm_block_sums(ok, 2, [(0, 5, 1)])
    assert pkg.engine.block_array((3, 6)).tolist() == [[3, 6]]
    assert pkg.engine.block_array([(0, 5), (7, 5)]).dtype == np.int32
    hs22, phis22 = random_disorder(np.random.default_rng(4), 22, 1)
    with pytest.raises(ValueError, match="more than the 10"):
        pkg.entanglement.entanglement_profile(
            pkg.SweepSpec(L=22, T=3, hs=hs22, phis=phis22), 2, engine=stub)


def test_cli_block_flags(pkg):
    cli = pkg.entanglement_cli
    a = cli.build_parser().parse_args(["--L", "12", "--block_size", "6"])
    assert (a.block_size, a.block_start, a.profile) == (6, None, 0)
    assert cli.blocks_from_args(a).tolist() == [[0, 6]]
    a = cli.build_parser().parse_args(["--L", "20", "--block_size", "10", "--block_start", "0",
                                       "--block_start", "10", "--profile", "1"])
    assert cli.blocks_from_args(a).tolist() == [[0, 10], [10, 10]] and a.profile == 1
    assert cli.blocks_from_args(a).dtype == np.int32
    # without the new flags nothing changes
    a = cli.build_parser().parse_args(["--L", "5", "--window_size", "2"])
    assert cli.blocks_from_args(a) is None and a.profile == 0
    assert cli.windows_from_args(a).tolist() == [[0, 1], [1, 2], [2, 3], [3, 4]]
    for bad in (["--L", "12", "--block_size", "7"], ["--L", "12", "--block_size", "5",
                                                      "--block_start", "8"],
                ["--L", "12", "--block_size", "5", "--block_start", "-1"],
                ["--L", "12", "--block_start", "0"]):
        with pytest.raises(ValueError):
            cli.blocks_from_args(cli.build_parser().parse_args(bad))
    for bad in (["--block_size", "4"], ["--block_size", "11"], ["--profile", "2"]):
        with pytest.raises(SystemExit):
            cli.build_parser().parse_args(bad)
    assert cli.block_label((3, 6)) == "b3-8"
    assert cli.entanglement_file_name("entanglement_block_data", "csv", "neel", 0.97, 12, 1, 6, 1,
                                      0.0, 1.0, 0.05, 1) == (
        "entanglement_block_data_neel_g0.97_L12_inst1_tf6_randomphi1_delta0.0_amplitude1.0"
        "_noise0.05_usenoise1.csv")
