"""All-pair correlators, the host side (no GPU): the contract's reference
dtc_correlations_state -- which forms the chunk partials by plain loops and
combines them with the kernels' own index algebra (csrc/dtc_corr.h) -- against
direct numpy sums, the host helpers of correlations.py, the trajectory mean of
the C oracle against the exact depolarizing channel, refusals and null
arguments."""
import ctypes

import numpy as np
import pytest

from tests import correlation_model as cm
from tests.helpers import harsh_device, random_disorder


def _random_state(L, seed):
    rng = np.random.default_rng(seed)
    psi = rng.normal(size=1 << L) + 1j * rng.normal(size=1 << L)
    return psi / np.linalg.norm(psi)


# L = 5: padding, lane bits only; 12: every in-chunk class (lane, wave,
# register); 14: two global bits -- chunk x global and global x global pairs
@pytest.mark.parametrize("L", [1, 5, 12, 14])
@pytest.mark.parametrize("basis", [0, 1])
def test_correlations_state_matches_numpy(pkg, L, basis):
    psi = _random_state(L, 100 + L)
    z, zz = pkg.engine.correlations_state(psi, L, basis)
    wz, wzz = cm.state_correlators(psi, L, basis)
    assert z.shape == (L,) and zz.shape == (L * (L - 1) // 2,)
    err = max(np.max(np.abs(z - wz)), np.max(np.abs(zz - wzz)) if L > 1 else 0.0)
    print(f"L={L} basis {basis}: largest deviation {err:.3e}")
    assert err <= cm.EPS


def test_reference_by_transform_agrees_with_direct_sums():
    """The oracle side's two ways to the same numbers (tests/correlation_model.py:
    direct sums up to L = 14, the numpy Walsh-Hadamard transform above)."""
    L = cm.DIRECT_MAX_L
    w = np.abs(_random_state(L, 3)) ** 2
    z, zz = cm.weights_correlators_direct(w, L)
    tz, tzz = cm.weights_correlators_wht(w, L)
    assert np.max(np.abs(z - tz)) <= 1e-13 and np.max(np.abs(zz - tzz)) <= 1e-13


@pytest.mark.parametrize("L,mask", [(5, 0b01010), (12, 0xA5C), (14, 0x2F31), (14, 0)])
def test_correlations_state_basis_state(pkg, L, mask):
    psi = np.zeros(1 << L, dtype=np.complex128)
    psi[mask] = 1.0
    z, zz = pkg.engine.correlations_state(psi, L, 0)
    s = np.array([1.0 - 2.0 * ((mask >> i) & 1) for i in range(L)])
    i, j = cm.pairs(L)
    assert np.array_equal(z, s)
    assert np.array_equal(zz, s[i] * s[j])
    # in X every site and pair of a basis state is 0
    x, xx = pkg.engine.correlations_state(psi, L, 1)
    assert np.max(np.abs(x)) <= cm.EPS and np.max(np.abs(xx)) <= cm.EPS


def test_pair_index_and_matrix_round_trip(pkg):
    co = pkg.correlations
    for L in (2, 5, 14):
        i, j = co.pair_index(L)
        wi, wj = cm.pairs(L)
        assert np.array_equal(i, wi) and np.array_equal(j, wj)
        # the C ABI's closed form
        assert np.array_equal(i * (2 * L - i - 1) // 2 + j - i - 1, np.arange(i.size))
        rng = np.random.default_rng(L)
        zz = rng.uniform(-1, 1, (3, 2, i.size))
        C = co.pair_matrix(zz, L)
        assert C.shape == (3, 2, L, L)
        assert np.array_equal(C, np.swapaxes(C, -1, -2))
        assert np.all(C[..., np.arange(L), np.arange(L)] == 1.0)
        assert np.array_equal(co.pair_vector(C), zz)
        assert C[1, 1, 0, L - 1] == zz[1, 1, L - 2]
    with pytest.raises(ValueError):
        co.pair_matrix(np.zeros(4), 4)


def test_spin_glass_order_known_values(pkg):
    co = pkg.correlations
    L = 6
    assert co.spin_glass_order(np.ones((L, L))) == pytest.approx(1.0, abs=1e-15)
    assert co.spin_glass_order(np.eye(L)) == 0.0
    stack = np.stack([np.ones((L, L)), np.eye(L), 0.5 * np.ones((L, L))])
    assert np.allclose(co.spin_glass_order(stack), [1.0, 0.0, 0.25], atol=1e-15)


def test_connected_of_a_product_state_is_zero(pkg):
    """|psi> = tensor of single-site states: <Z_i Z_j> = <Z_i><Z_j>."""
    co = pkg.correlations
    L = 5
    rng = np.random.default_rng(9)
    psi = np.ones(1, dtype=np.complex128)
    for _ in range(L):
        v = rng.normal(size=2) + 1j * rng.normal(size=2)
        psi = np.kron(v / np.linalg.norm(v), psi)
    z, zz = pkg.engine.correlations_state(psi, L, 0)
    assert np.max(np.abs(z)) > 0.05
    assert np.max(np.abs(co.connected(zz, z))) <= 1e-12


def test_unbiased_estimator_removes_the_variance_bias(pkg):
    """Synthetic +-1 rows with known means m: over many resamples of n = 8 rows
    the U-statistic averages to mean(m^2), the plain mean-then-square to
    mean(m^2 + (1 - m^2) / n).  2000 resamples: each estimate lies in [-1, 1],
    so the resample mean is within 5 / sqrt(2000) = 0.112 -- far looser than
    needed; the two expectations differ by mean(1 - m^2) / n = 0.0916 and the
    measured standard error is about 0.005, so the assertion is 0.03."""
    co = pkg.correlations
    rng = np.random.default_rng(5)
    m = np.array([0.7, -0.4, 0.1, 0.0, -0.9, 0.5])
    n, reps = 8, 2000
    rows = np.where(rng.uniform(size=(reps, n, m.size)) < (1 + m) / 2, 1.0, -1.0)
    unb = co.spin_glass_order_unbiased(rows, axis=1)
    assert unb.shape == (reps,)
    plain = (rows.mean(axis=1) ** 2).mean(axis=-1)
    truth = float(np.mean(m * m))
    bias = float(np.mean(1 - m * m)) / n
    print(f"truth {truth:.4f}: unbiased {unb.mean():.4f}, plain {plain.mean():.4f} "
          f"(expected bias {bias:.4f})")
    assert abs(unb.mean() - truth) < 0.03
    assert abs(plain.mean() - truth - bias) < 0.03
    with pytest.raises(ValueError):
        co.spin_glass_order_unbiased(rows[:, :1], axis=1)


def test_trajectory_mean_against_exact_channel(pkg):
    """L = 4, T = 4, p = 0.05: the mean over n C-oracle trajectories of every
    site and pair, both bases, against the exact density matrix: C_ij is linear
    in rho, so the mean estimates the channel's value; bound 5 / sqrt(n)."""
    c = cm.CHANNEL
    hs, phis = random_disorder(np.random.default_rng(c["seed"]), c["L"])
    spec = pkg.energy.energy_spec(c["L"], c["T"], hs, phis, 0.94, "vacuum", noise_prob=c["p"])
    exact = cm.exact_channel(spec)
    acc = {k: np.zeros_like(v) for k, v in exact.items()}
    for tr in range(c["n"]):
        rows = cm.trajectory_rows(spec, 0, tr, c["seed"])
        for k in acc:
            acc[k] += rows[k]
    bound = 5.0 / np.sqrt(c["n"])
    for k in acc:
        dev = float(np.max(np.abs(acc[k] / c["n"] - exact[k])))
        print(f"{k}: largest deviation {dev:.4f}, bound {bound:.4f}")
        assert dev <= bound, k
    # the channel is not trivial here: the noisy values differ from the noiseless ones
    clean = cm.trajectory_rows(pkg.energy.energy_spec(c["L"], c["T"], hs, phis, 0.94, "vacuum",
                                                      noise_prob=0.0, use_noise=0), 0, 0, 1)
    assert np.max(np.abs(clean["zz"] - exact["zz"])) > 0.02


class _StubEngine:
    def __init__(self):
        self.calls = []

    def correlation_sums(self, *a, **k):
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
            pkg.engine.refuse_correlations(spec, "x")
        with pytest.raises(NotImplementedError, match=word):
            bare.correlations(spec, 2)
        with pytest.raises(NotImplementedError, match=word):
            bare.correlation_sums(spec, 2)
        with pytest.raises(NotImplementedError, match=word):
            pkg.correlations.get_instances_correlations(spec, 2, engine=stub)
    assert stub.calls == []
    ok = pkg.SweepSpec(L=L, T=4, hs=hs, phis=phis)
    pkg.engine.refuse_correlations(ok, "x")
    for bad in ("y", "", "zq"):
        with pytest.raises(ValueError, match="bases"):
            bare.correlations(ok, 2, bases=bad)


def test_symbols_and_null_arguments(pkg):
    """Exported by the built library; null arguments fail with -1 before any
    device call."""
    names = ("dtc_correlations", "dtc_correlation_sums", "dtc_correlations_state")
    lib = pkg._capi.load_library()
    for name in names:
        assert name in pkg._capi.EXPORTED_SYMBOLS
        assert hasattr(lib, name)
    for fn in (lib.dtc_correlations, lib.dtc_correlation_sums):
        rc = fn(None, None, None, ctypes.c_uint64(1), ctypes.c_int64(0), ctypes.c_int32(1),
                None, None, None, None)
        assert rc == -1
        assert b"null" in lib.dtc_last_error()
    dp = pkg._capi.as_dptr
    psi = np.zeros(8)
    psi[0] = 1.0
    z, zz = np.zeros(2), np.zeros(1)
    assert lib.dtc_correlations_state(None, 2, 0, dp(z), dp(zz)) == -1
    assert lib.dtc_correlations_state(dp(psi), 2, 0, None, dp(zz)) == -1
    assert lib.dtc_correlations_state(dp(psi), 2, 0, dp(z), None) == -1
    assert lib.dtc_correlations_state(dp(psi), 33, 0, dp(z), dp(zz)) == -1
    assert lib.dtc_correlations_state(dp(psi), 2, 2, dp(z), dp(zz)) == -1
    assert lib.dtc_correlations_state(dp(psi), 2, 0, dp(z), dp(zz)) == 0
    assert lib.dtc_correlations_state(dp(psi), 1, 0, dp(z), None) == 0


def test_cli_parser_and_names(pkg):
    cli = pkg.correlation_cli
    a = cli.build_parser().parse_args(["--L", "5", "--bases", "zx"])
    assert (a.L, a.bases, a.initial_state, a.polarization) == (5, "zx", "vacuum", "x")
    assert cli.correlation_folder(5) == "correlation-data_L5"
    assert cli.correlation_file_name("correlation_data", "csv", "neel", 0.97, 5, 1, 6, 1, 0.0, 1.0,
                                     0.05, 1) == (
        "correlation_data_neel_g0.97_L5_inst1_tf6_randomphi1_delta0.0_amplitude1.0_noise0.05"
        "_usenoise1.csv")
