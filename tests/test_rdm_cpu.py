"""Reduced density matrices, the host side (no GPU): the contract's reference
dtc_rdm_state against numpy reshape-and-matmul, Hermiticity, the Gram kernel's
index algebra walked on the host, every DTC_EINVAL case, the helpers of entanglement.py on states of known entanglement, the
trajectory mean of the C oracle against the exact depolarizing channel,
refusals, null arguments and the command line's parser and file names."""
import ctypes
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import correlation_model as cm
from tests import rdm_model as rm
from tests.helpers import harsh_device, random_disorder


def _random_state(L, seed):
    rng = np.random.default_rng(seed)
    psi = rng.normal(size=1 << L) + 1j * rng.normal(size=1 << L)
    return psi / np.linalg.norm(psi)


def _windows(L, k):
    """Lowest sites, highest sites (with the top bit) and spread sites."""
    low = tuple(range(k))
    high = tuple(range(L - k, L))
    spread = tuple(sorted({(m * (L - 1)) // max(k - 1, 1) for m in range(k)}))
    if k == 1:
        spread = (L // 2,)
    return sorted({low, high, spread if len(spread) == k else low})


# both sides are plain sums of at most 2^13 products of modulus <= 1 of a
# normalised state: 1e-13
@pytest.mark.parametrize("L", [1, 2, 5, 12, 13])
def test_rdm_state_matches_numpy(pkg, L):
    psi = _random_state(L, 200 + L)
    worst = 0.0
    for k in range(1, min(4, L) + 1):
        for sites in _windows(L, k):
            rho = pkg.engine.rdm_state(psi, L, sites)
            want = rm.state_rdm(psi, L, sites)
            assert rho.shape == (1 << k, 1 << k) and rho.dtype == np.complex128
            err = float(np.max(np.abs(rho - want)))
            worst = max(worst, err)
            assert err <= 1e-13, (L, sites, err)
            # Hermitian bit for bit, the diagonal exactly real
            assert np.array_equal(rho, rho.conj().T), (L, sites)
            assert np.all(np.diag(rho).imag == 0.0), (L, sites)
            assert abs(np.trace(rho).real - 1.0) <= 1e-13
    print(f"L={L}: largest deviation {worst:.3e}")


@pytest.mark.parametrize("L,mask", [(1, 1), (5, 0b01010), (12, 0xA5C), (13, 0x1F31), (13, 0)])
def test_rdm_state_basis_state(pkg, L, mask):
    psi = np.zeros(1 << L, dtype=np.complex128)
    psi[mask] = 1.0
    for k in range(1, min(4, L) + 1):
        for sites in _windows(L, k):
            rho = pkg.engine.rdm_state(psi, L, sites)
            al = sum(((mask >> s) & 1) << m for m, s in enumerate(sites))
            want = np.zeros((1 << k, 1 << k), dtype=np.complex128)
            want[al, al] = 1.0
            assert np.array_equal(rho, want), (L, mask, sites)


def test_kernel_index_algebra(tmp_path):
    """tools/rdm_geometry_check.cpp walks the Gram kernel's addressing (tile, wave,
    lane, register) with csrc/dtc_rdm.h for every window at L_eff = 12, 13: every
    amplitude read exactly once, in bounds, at the LDS slot of its row and column."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "rdm_geometry_check")
    pkg_dir = "noise-resilience-in-discrete-time-crystal-realizations-on-quantum-computers_amd"
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-O2", "-I",
                    os.path.join(root, pkg_dir, "csrc"),
                    os.path.join(root, "tools", "rdm_geometry_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout.strip())
    assert r.returncode == 0, (r.stdout[-400:], r.stderr[-400:])
    assert r.stdout.split()[:2] == ["cases", "2370"] and r.stdout.split()[-1] == "0"


def test_rdm_state_einval(pkg):
    """Every DTC_EINVAL case of the contract that needs no device."""
    lib = pkg._capi.load_library()
    dp = pkg._capi.as_dptr
    ip = ctypes.POINTER(ctypes.c_int32)
    L = 5
    psi = np.zeros(2 << L)
    psi[0] = 1.0
    rho = np.zeros(2 * 256)

    def call(state, L_, sites, k, out):
        s = np.asarray(sites, dtype=np.int32) if sites is not None else None
        return lib.dtc_rdm_state(state, L_, s.ctypes.data_as(ip) if s is not None else None, k, out)

    assert call(dp(psi), L, [0, 1], 2, dp(rho)) == 0
    bad = [
        (None, L, [0, 1], 2, dp(rho)),            # null state
        (dp(psi), L, None, 2, dp(rho)),           # null sites
        (dp(psi), L, [0, 1], 2, None),            # null output
        (dp(psi), L, [0], 0, dp(rho)),            # k < 1
        (dp(psi), L, [0, 1, 2, 3, 4], 5, dp(rho)),  # k > 4
        (dp(psi), 3, [0, 1, 2, 3], 4, dp(rho)),   # k > L
        (dp(psi), L, [0, 5], 2, dp(rho)),         # site >= L
        (dp(psi), L, [-1, 2], 2, dp(rho)),        # site < 0
        (dp(psi), L, [2, 2], 2, dp(rho)),         # not strictly ascending
        (dp(psi), L, [3, 1], 2, dp(rho)),         # descending
        (dp(psi), 0, [0], 1, dp(rho)),            # L < 1
        (dp(psi), 33, [0], 1, dp(rho)),           # L > 32
    ]
    for args in bad:
        assert call(*args) == -1, args[1:4]
        assert lib.dtc_last_error()
    with pytest.raises(pkg._capi.DtcError):
        pkg.engine.rdm_state(psi[::2] + 0j, L, [1, 1])
    with pytest.raises(ValueError):
        pkg.engine.rdm_state(np.zeros(7), 3, [0])


def test_known_entanglement_values(pkg):
    en = pkg.entanglement
    ln2 = np.log(2.0)
    bell = np.zeros(4, dtype=np.complex128)
    bell[0] = bell[3] = np.sqrt(0.5)
    r2 = pkg.engine.rdm_state(bell, 2, [0, 1])
    for s in (0, 1):
        r1 = pkg.engine.rdm_state(bell, 2, [s])
        assert abs(en.von_neumann_entropy(r1) - ln2) <= 1e-12
        assert abs(en.purity(r1) - 0.5) <= 1e-12
        assert abs(en.renyi2(r1) - ln2) <= 1e-12
    assert abs(en.von_neumann_entropy(r2)) <= 1e-12
    assert abs(en.mutual_information(r2) - 2 * ln2) <= 1e-12
    # a product state of a longer chain: every window is pure
    L = 5
    rng = np.random.default_rng(4)
    prod = np.ones(1, dtype=np.complex128)
    for _ in range(L):
        v = rng.normal(size=2) + 1j * rng.normal(size=2)
        prod = np.kron(v / np.linalg.norm(v), prod)
    for k in range(1, 5):
        for sites in itertools.combinations(range(L), k):
            rho = pkg.engine.rdm_state(prod, L, sites)
            assert abs(en.von_neumann_entropy(rho)) <= 1e-12
            assert abs(en.purity(rho) - 1.0) <= 1e-12
    assert abs(en.mutual_information(pkg.engine.rdm_state(prod, L, [1, 3]))) <= 1e-12
    # a Bell pair on sites 1 and 3 of that chain, the other sites in |0>
    ent = np.zeros(1 << L, dtype=np.complex128)
    ent[0] = ent[(1 << 1) | (1 << 3)] = np.sqrt(0.5)
    assert abs(en.mutual_information(pkg.engine.rdm_state(ent, L, [1, 3])) - 2 * ln2) <= 1e-12
    assert abs(en.mutual_information(pkg.engine.rdm_state(ent, L, [0, 3]))) <= 1e-12
    assert abs(en.von_neumann_entropy(pkg.engine.rdm_state(ent, L, [0, 1, 2])) - ln2) <= 1e-12
    # maximally mixed
    for d in (2, 4, 8, 16):
        mixed = np.eye(d) / d
        assert abs(en.von_neumann_entropy(mixed) - np.log(d)) <= 1e-12
        assert abs(en.purity(mixed) - 1.0 / d) <= 1e-12
    # stacks keep their leading axes; a small negative eigenvalue is clipped
    stack = np.stack([np.eye(4) / 4, np.diag([1.0, 0, 0, 0])])
    assert np.allclose(en.von_neumann_entropy(stack), [np.log(4), 0.0], atol=1e-12)
    assert en.von_neumann_entropy(np.diag([1.0 + 1e-17, -1e-17])) == pytest.approx(0.0, abs=1e-15)
    with pytest.raises(ValueError):
        en.purity(np.zeros((3, 3)))
    with pytest.raises(ValueError):
        en.mutual_information(np.eye(2) / 2)


def test_partial_trace(pkg):
    en = pkg.entanglement
    L = 6
    psi = _random_state(L, 31)
    r2 = pkg.engine.rdm_state(psi, L, [1, 4])
    assert np.max(np.abs(en.partial_trace(r2, [0]) - pkg.engine.rdm_state(psi, L, [1]))) <= 1e-13
    assert np.max(np.abs(en.partial_trace(r2, [1]) - pkg.engine.rdm_state(psi, L, [4]))) <= 1e-13
    r4 = pkg.engine.rdm_state(psi, L, [0, 2, 3, 5])
    for keep in ([0], [3], [0, 1], [1, 3], [0, 2, 3], [0, 1, 2, 3]):
        want = rm.state_rdm(psi, L, [[0, 2, 3, 5][m] for m in keep])
        assert np.max(np.abs(en.partial_trace(r4, keep) - want)) <= 1e-13, keep
    stack = np.stack([r4, 2 * r4])
    assert np.allclose(en.partial_trace(stack, [1, 2])[1], 2 * en.partial_trace(r4, [1, 2]))
    for bad in ([], [4], [1, 1], [2, 0]):
        with pytest.raises(ValueError):
            en.partial_trace(r4, bad)


def test_pauli_expectations_reproduce_the_correlators(pkg):
    """Z, ZZ, X, XX of tests/correlation_model.state_correlators, and every other
    string against the explicit operator."""
    en = pkg.entanglement
    L = 6
    psi = _random_state(L, 77)
    z, zz = cm.state_correlators(psi, L, 0)
    x, xx = cm.state_correlators(psi, L, 1)
    for i in range(L):
        e = en.pauli_expectations(pkg.engine.rdm_state(psi, L, [i]))
        assert e.shape == (4,)
        assert abs(e[0] - 1.0) <= 1e-13 and abs(e[3] - z[i]) <= 1e-13
        assert abs(e[1] - x[i]) <= 1e-13
    pi, pj = cm.pairs(L)
    for n, (i, j) in enumerate(zip(pi, pj)):
        e = en.pauli_expectations(pkg.engine.rdm_state(psi, L, [i, j]))
        assert e.shape == (16,)
        assert abs(e[3 + 4 * 3] - zz[n]) <= 1e-13 and abs(e[1 + 4 * 1] - xx[n]) <= 1e-13
        assert abs(e[3] - z[i]) <= 1e-13 and abs(e[4 * 3] - z[j]) <= 1e-13
    assert en.pauli_strings(2)[7] == "ZX" and en.pauli_strings(1) == ["I", "X", "Y", "Z"]
    sites = [0, 2, 5]
    rho = pkg.engine.rdm_state(psi, L, sites)
    e = en.pauli_expectations(rho)
    for q, letters in enumerate(en.pauli_strings(3)):
        full = np.ones((1, 1), dtype=np.complex128)
        for s in range(L):
            c = letters[sites.index(s)] if s in sites else "I"
            full = np.kron(rm.PAULI[c], full)
        want = np.vdot(psi, full @ psi).real
        assert abs(e[q] - want) <= 1e-12, letters
        assert np.array_equal(en.pauli_operator(q, 3), rm.window_operator(letters))


def test_trajectory_mean_against_exact_channel(pkg):
    """L = 4, T = 4, p = 0.05: the mean over n C-oracle trajectories of every
    entry of rho_A against the partial trace of the exact density matrix: rho_A
    is linear in |psi><psi|, so the mean estimates the channel's reduced state.
    Every summand has modulus <= 1: real and imaginary parts within 5 / sqrt(n)."""
    c = rm.CHANNEL
    hs, phis = random_disorder(np.random.default_rng(c["seed"]), c["L"])
    spec = pkg.energy.energy_spec(c["L"], c["T"], hs, phis, 0.94, "vacuum", noise_prob=c["p"])
    exact = rm.exact_channel(spec, rm.CHANNEL_WINDOWS)
    acc = {w: np.zeros_like(v) for w, v in exact.items()}
    from tests import sample_model as sm

    for tr in range(c["n"]):
        for t, psi in sm.trajectory_states(spec, 0, tr, c["seed"]):
            for w in acc:
                acc[w][t] += pkg.engine.rdm_state(psi, c["L"], w)
    bound = 5.0 / np.sqrt(c["n"])
    for w in acc:
        diff = acc[w] / c["n"] - exact[w]
        dev = float(max(np.max(np.abs(diff.real)), np.max(np.abs(diff.imag))))
        print(f"{w}: largest deviation {dev:.4f}, bound {bound:.4f}")
        assert dev <= bound, w
    # the channel is not trivial here: the noisy state differs from the noiseless one
    clean_spec = pkg.energy.energy_spec(c["L"], c["T"], hs, phis, 0.94, "vacuum", noise_prob=0.0,
                                        use_noise=0)
    clean = rm.trajectory_rows(clean_spec, 0, 0, 1, [(0, 1, 2, 3)])[:, 0]
    assert np.max(np.abs(clean - exact[(0, 1, 2, 3)])) > 0.02
    # and the noise-averaged window is mixed: its entropy exceeds the pure state's
    en = pkg.entanglement
    assert en.von_neumann_entropy(exact[(0, 1, 2, 3)][-1]) > 0.05
    assert en.von_neumann_entropy(clean[-1]) <= 1e-9


class _StubEngine:
    def __init__(self):
        self.calls = []

    def rdm_sums(self, *a, **k):
        self.calls.append((a, k))
        raise AssertionError("the engine must not be reached")


def test_refusals_without_a_device(pkg):
    L = 5
    hs, phis = random_disorder(np.random.default_rng(3), L, 1)
    dev = pkg.SweepSpec(L=L, T=4, hs=hs, phis=phis, device=harsh_device(pkg, L))
    bond = pkg.SweepSpec(L=L, T=4, hs=hs, phis=phis, bond_noise=0.02)
    bare = pkg.DtcEngine.__new__(pkg.DtcEngine)
    stub = _StubEngine()
    for spec, word in ((dev, "device-like noise"), (bond, "bond noise")):
        with pytest.raises(NotImplementedError, match=word):
            pkg.engine.refuse_rdm(spec, "x")
        with pytest.raises(NotImplementedError, match=word):
            bare.rdm(spec, 2, [(0, 1)])
        with pytest.raises(NotImplementedError, match=word):
            bare.rdm_sums(spec, 2, [(0, 1)])
        with pytest.raises(NotImplementedError, match=word):
            pkg.entanglement.get_instances_rdm(spec, 2, [(0, 1)], engine=stub)
    assert stub.calls == []
    ok = pkg.SweepSpec(L=L, T=4, hs=hs, phis=phis)
    pkg.engine.refuse_rdm(ok, "x")
    with pytest.raises(ValueError, match="window size"):
        bare.rdm(ok, 2, [(0, 1, 2, 3, 4)])
    with pytest.raises(ValueError):
        bare.rdm(ok, 2, [[]])
    assert pkg.engine.window_array((1, 2)).shape == (1, 2)
    assert pkg.engine.window_array([(0,), (4,)]).dtype == np.int32


def test_symbols_and_null_arguments(pkg):
    """Exported by the built library; null arguments fail with -1 before any
    device call."""
    names = ("dtc_rdm", "dtc_rdm_sums", "dtc_rdm_state")
    lib = pkg._capi.load_library()
    for name in names:
        assert name in pkg._capi.EXPORTED_SYMBOLS
        assert hasattr(lib, name)
    for fn in (lib.dtc_rdm, lib.dtc_rdm_sums):
        rc = fn(None, None, None, ctypes.c_uint64(1), ctypes.c_int64(0), ctypes.c_int32(1),
                None, ctypes.c_int32(1), ctypes.c_int32(1), None)
        assert rc == -1
        assert b"null" in lib.dtc_last_error()


def test_cli_parser_and_names(pkg):
    cli = pkg.entanglement_cli
    a = cli.build_parser().parse_args(["--L", "5", "--window_size", "2"])
    assert (a.L, a.window_size, a.initial_state, a.polarization) == (5, 2, "vacuum", "x")
    assert cli.windows_from_args(a).tolist() == [[0, 1], [1, 2], [2, 3], [3, 4]]
    a = cli.build_parser().parse_args(["--L", "6", "--window_size", "3", "--window_start", "1",
                                       "--window_stride", "2"])
    assert cli.windows_from_args(a).tolist() == [[1, 2, 3], [3, 4, 5]]
    a = cli.build_parser().parse_args(["--L", "5", "--window_sites", "0,1", "2,4"])
    assert cli.windows_from_args(a).tolist() == [[0, 1], [2, 4]]
    for bad in (["0,1", "2"], ["1,0"], ["0,5"], ["0,1,2,3,4"]):
        with pytest.raises(ValueError):
            cli.windows_from_args(cli.build_parser().parse_args(["--L", "5", "--window_sites", *bad]))
    assert cli.window_label([1, 3]) == "s1-3"
    assert cli.entanglement_folder(5) == "entanglement-data_L5"
    assert cli.entanglement_file_name("entanglement_data", "csv", "neel", 0.97, 5, 1, 6, 1, 0.0,
                                      1.0, 0.05, 1) == (
        "entanglement_data_neel_g0.97_L5_inst1_tf6_randomphi1_delta0.0_amplitude1.0_noise0.05"
        "_usenoise1.csv")
