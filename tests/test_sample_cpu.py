"""Measurement sampling without a GPU: the host entry points of the contract
(dtc_sample_draws, dtc_sample_state), the estimator's host side in energy.py,
the CLI switch, and the refusals (include/dtc.h dtc_sample)."""
import ctypes

import numpy as np
import pytest

from tests.helpers import harsh_device, random_disorder

STREAM_MEASURE = 0xFFFFFFFE
M32 = 0xFFFFFFFF


def philox4x32_10(c, k):
    """Philox4x32-10 (Salmon et al., SC'11) on python ints: counter c[4], key k[2]."""
    c0, c1, c2, c3 = c
    k0, k1 = k
    for _ in range(10):
        p0 = 0xD2511F53 * c0
        p1 = 0xCD9E8D57 * c2
        c0, c1, c2, c3 = ((p1 >> 32) ^ c1 ^ k0) & M32, p1 & M32, ((p0 >> 32) ^ c3 ^ k1) & M32, p0 & M32
        k0 = (k0 + 0x9E3779B9) & M32
        k1 = (k1 + 0xBB67AE85) & M32
    return c0, c1, c2, c3


def uniform(seed, traj, p, basis, shot):
    """The formula of include/dtc.h: the words and the uniform of one shot."""
    w = philox4x32_10((shot | basis << 30, p, STREAM_MEASURE, traj & M32),
                      (seed & M32, ((seed >> 32) ^ (traj >> 32)) & M32))
    return w[:2], ((w[0] << 21) | (w[1] >> 11)) * 2.0 ** -53


def test_philox_known_answer():
    """The test's Philox against the Random123 known-answer vectors."""
    assert philox4x32_10((0, 0, 0, 0), (0, 0)) == (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)
    assert philox4x32_10((M32,) * 4, (M32, M32)) == (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)


@pytest.mark.parametrize("seed,traj,p,basis", [
    (0x5EED0001, 0, 0, 0), (0x5EED0001, 0, 0, 1), (0xDEADBEEF12345678, 5, 7, 1),
    (3, (1 << 33) + 9, 2, 0)])
def test_sample_draws_formula(pkg, seed, traj, p, basis):
    u = pkg.engine.sample_draws(seed, traj, p, basis, 33)
    want = np.array([uniform(seed, traj, p, basis, k)[1] for k in range(33)])
    assert np.array_equal(u, want)
    assert np.all(u >= 0.0) and np.all(u < 1.0)


def test_sample_draws_distinct(pkg):
    """Distinct (traj, p, basis, shot) give distinct words (and uniforms)."""
    seed = 0x5EED0001
    words, us = set(), []
    n = 0
    for traj in range(4):
        for p in range(4):
            for basis in range(2):
                us.append(pkg.engine.sample_draws(seed, traj, p, basis, 16))
                for shot in range(16):
                    words.add(uniform(seed, traj, p, basis, shot)[0])
                    n += 1
    assert len(words) == n
    assert len(np.unique(np.concatenate(us))) == n


def test_sample_draws_arguments(pkg):
    lib = pkg._capi.load_library()
    u = np.zeros(4)
    assert lib.dtc_sample_draws(1, 0, 0, 0, 0, pkg._capi.as_dptr(u)) == -1
    assert lib.dtc_sample_draws(1, 0, 0, 2, 4, pkg._capi.as_dptr(u)) == -1
    assert lib.dtc_sample_draws(1, 0, 0, 0, 4, None) == -1


def _hadamard_all(psi, L):
    a = psi.reshape([2] * L).copy()
    for ax in range(L):
        a0, a1 = np.take(a, 0, axis=ax), np.take(a, 1, axis=ax)
        a = np.stack([a0 + a1, a0 - a1], axis=ax) / np.sqrt(2.0)
    return a.reshape(-1)


def _random_state(rng, L):
    """A normalised random state whose blocks (and a few single entries) are exact zeros."""
    n = 1 << L
    psi = rng.normal(size=n) + 1j * rng.normal(size=n)
    if L >= 2:
        q = n // 4
        psi[:q // 2 + 1] = 0.0        # the first indices
        psi[2 * q:3 * q] = 0.0        # a block in the middle
        psi[n - max(q // 3, 1):] = 0.0  # the last indices
        psi[rng.integers(0, n, size=max(n // 16, 1))] = 0.0
    return psi / np.linalg.norm(psi)


@pytest.mark.parametrize("L", [1, 5, 10])
def test_sample_state_matches_searchsorted(pkg, L):
    rng = np.random.default_rng(100 + L)
    psi = _random_state(rng, L)
    w = psi.real * psi.real + psi.imag * psi.imag
    cs = np.cumsum(w)
    u = rng.random(512)
    got = pkg.engine.sample_state(psi, L, 0, u)
    want = np.searchsorted(cs, u * cs[-1], side="right")
    assert got.dtype == np.uint64
    assert np.array_equal(got, want.astype(np.uint64))
    assert np.all(w[got.astype(np.int64)] > 0.0)
    nz = np.flatnonzero(w)
    edge = pkg.engine.sample_state(psi, L, 0, np.array([0.0, 1.0 - 2.0 ** -53]))
    assert int(edge[0]) == nz[0] and int(edge[1]) == nz[-1]


@pytest.mark.parametrize("L", [1, 5, 10])
def test_sample_state_x_basis(pkg, L):
    """Basis 1 is the rule on H^L psi (a boundary case within the rounding of
    the transformed weights may fall either way: none with these uniforms)."""
    rng = np.random.default_rng(200 + L)
    psi = _random_state(rng, L)
    hpsi = _hadamard_all(psi, L)
    cs = np.cumsum(hpsi.real ** 2 + hpsi.imag ** 2)
    u = rng.random(256)
    got = pkg.engine.sample_state(psi, L, 1, u).astype(np.int64)
    tgt = u * cs[-1]
    lo = np.where(got > 0, cs[got - 1], 0.0)
    assert np.all(lo <= tgt + 1e-13) and np.all(tgt <= cs[got] + 1e-13)


@pytest.mark.parametrize("L", [1, 5, 10])
def test_sample_state_basis_states(pkg, L):
    rng = np.random.default_rng(300 + L)
    u = np.concatenate([[0.0, 1.0 - 2.0 ** -53], rng.random(64)])
    for m in {0, (1 << L) - 1, int(rng.integers(0, 1 << L))}:
        psi = np.zeros(1 << L, dtype=np.complex128)
        psi[m] = 1.0
        assert np.all(pkg.engine.sample_state(psi, L, 0, u) == m)
        got = pkg.engine.sample_state(psi, L, 1, u)
        assert np.array_equal(got, np.floor(u * 2.0 ** L).astype(np.uint64))


def test_histogram_condition_on_host(pkg):
    """The GPU histogram test's seed: dtc_sample_state on the oracle's state with
    the same uniforms meets the chi^2 bound in both bases (16 outcomes)."""
    from tests import sample_model as sm

    h = sm.HIST
    spec, psi = sm.hist_state(pkg)
    for basis in (0, 1):
        u = pkg.engine.sample_draws(h["seed"], 0, h["t"], basis, h["n_shots"])
        bits = pkg.engine.sample_state(psi, h["L"], basis, u)
        ref = sm.hadamard_all(psi, h["L"]) if basis else psi
        prob = np.abs(ref) ** 2
        chi2 = sm.pearson_chi2(bits, prob / prob.sum())
        print(f"basis {basis}: chi2 = {chi2:.2f} (bound {sm.chi2_bound(15):.2f}), "
              f"min expected count {h['n_shots'] * prob.min():.1f}")
        assert chi2 <= sm.chi2_bound(15)
        sm.check_outcomes(bits, ref, u)


def test_sample_state_arguments(pkg):
    lib = pkg._capi.load_library()
    psi = np.zeros(4)
    psi[0] = 1.0
    u = np.zeros(1)
    bits = np.zeros(1, dtype=np.uint64)
    bp = bits.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
    dp = pkg._capi.as_dptr
    assert lib.dtc_sample_state(None, 1, 0, dp(u), 1, bp) == -1
    assert lib.dtc_sample_state(dp(psi), 1, 0, None, 1, bp) == -1
    assert lib.dtc_sample_state(dp(psi), 1, 0, dp(u), 1, None) == -1
    assert lib.dtc_sample_state(dp(psi), 33, 0, dp(u), 1, bp) == -1
    assert lib.dtc_sample_state(dp(psi), 1, 0, dp(u), 0, bp) == -1
    assert lib.dtc_sample_state(dp(psi), 1, 0, dp(u), 1, bp) == 0


def test_sample_symbol_and_null_arguments(pkg):
    """Exported; null arguments fail with -1 before any device call."""
    for name in ("dtc_sample", "dtc_sample_draws", "dtc_sample_state"):
        assert name in pkg._capi.EXPORTED_SYMBOLS
    lib = pkg._capi.load_library()
    rc = lib.dtc_sample(None, None, None, ctypes.c_uint64(1), ctypes.c_int64(0),
                        ctypes.c_int32(1), ctypes.c_int32(1), None, None)
    assert rc == -1
    assert b"null" in lib.dtc_last_error()


def test_observables_from_samples(pkg):
    rng = np.random.default_rng(7)
    L, n_inst, n_traj, T, n_shots = 6, 2, 5, 3, 4
    bz = rng.integers(0, 1 << L, size=(n_inst, n_traj, T, n_shots)).astype(np.uint64)
    bx = rng.integers(0, 1 << L, size=(n_inst, n_traj, T, n_shots)).astype(np.uint64)
    obs = pkg.energy.observables_from_samples(bz, bx, L)
    assert obs["z"].shape == (n_inst, T, L) and obs["zz"].shape == (n_inst, T, L - 1)
    assert obs["x"].shape == (n_inst, T, L)
    for i in range(n_inst):
        for t in range(T):
            for q in range(L):
                zq = [1 - 2 * ((int(b) >> q) & 1) for b in bz[i, :, t].reshape(-1)]
                xq = [1 - 2 * ((int(b) >> q) & 1) for b in bx[i, :, t].reshape(-1)]
                assert obs["z"][i, t, q] == pytest.approx(np.mean(zq), abs=1e-15)
                assert obs["x"][i, t, q] == pytest.approx(np.mean(xq), abs=1e-15)
                if q + 1 < L:
                    zn = [1 - 2 * ((int(b) >> (q + 1)) & 1) for b in bz[i, :, t].reshape(-1)]
                    assert obs["zz"][i, t, q] == pytest.approx(np.mean(np.multiply(zq, zn)), abs=1e-15)
    only_z = pkg.energy.observables_from_samples(bz, None, L)
    assert np.array_equal(only_z["z"], obs["z"]) and not only_z["x"].any()
    # the shapes energy_from_observables takes
    hs, phis = random_disorder(np.random.default_rng(1), L, n_inst)
    e = pkg.energy.energy_from_observables({k: v[0] for k, v in obs.items()}, L, 0.97, hs[0], phis[0])
    assert e.shape == (T,)


def test_counts_from_samples_bit_order(pkg):
    """Qubit 0 is the rightmost character, as qiskit's get_counts writes it."""
    bits = np.array([1, 1, 4, 6, 1], dtype=np.uint64)
    assert pkg.energy.counts_from_samples(bits, 3) == {"001": 3, "100": 1, "110": 1}
    counts = pkg.energy.counts_from_samples(np.array([[2, 2], [2, 3]], dtype=np.uint64), 4)
    assert counts == {"0010": 3, "0011": 1}
    # the reference's compute_z_expectation reads character num_qubits - 1 - q for qubit q
    z0 = sum(c * (1 - 2 * int(s[4 - 1 - 0])) for s, c in counts.items()) / 4
    z1 = sum(c * (1 - 2 * int(s[4 - 1 - 1])) for s, c in counts.items()) / 4
    assert z0 == 0.5 and z1 == -1.0


class _StubEngine:
    """Records the calls; ``sample`` returns the all-zero outcomes."""

    def __init__(self):
        self.calls = []

    def sample(self, spec, n_traj, **kw):
        self.calls.append(("sample", n_traj, kw))
        shape = (spec.n_inst, n_traj, spec.T, kw.get("n_shots", 1))
        return {"z": np.zeros(shape, dtype=np.uint64), "x": np.zeros(shape, dtype=np.uint64)}

    def energy_sums(self, spec, n_traj, **kw):
        self.calls.append(("energy_sums", n_traj, kw))
        T, L, n = spec.T, spec.L, spec.n_inst
        return {"z": np.zeros((n, T, L)), "zz": np.zeros((n, T, L - 1)), "x": np.zeros((n, T, L))}


def test_run_energy_sampled_flag(pkg):
    en = pkg.energy
    hs, phis = random_disorder(np.random.default_rng(2), 5, 2)
    stub = _StubEngine()
    res = en.run_energy(5, 0.95, hs, phis, 4, nprobs=(0, 0.01), n_traj=8, engine=stub, sampled=True)
    assert [c[0] for c in stub.calls] == ["sample"] * 2
    assert all(c[1] == 8 and c[2]["n_shots"] == 1 and c[2]["bases"] == "zx" for c in stub.calls)
    # all outcomes 0: z = zz = x = +1 on every site
    cz, czz, cx = en.hamiltonian_coefficients(5, 0.95, hs[0], phis[0])
    cz1, czz1, cx1 = en.hamiltonian_coefficients(5, 0.95, hs[1], phis[1])
    want = (cz.sum() + czz.sum() + cx.sum() + cz1.sum() + czz1.sum() + cx1.sum()) / 2 / 5
    assert res[("full", 0)] == pytest.approx(np.full(4, want), abs=1e-12)
    stub = _StubEngine()
    en.run_energy(5, 0.95, hs, phis, 4, nprobs=(0,), n_traj=8, engine=stub)
    en.run_energy(5, 0.95, hs, phis, 4, nprobs=(0,), n_traj=8, engine=stub, sampled=False)
    assert [c[0] for c in stub.calls] == ["energy_sums"] * 2
    out = en.get_instances_energy_sampled(en.energy_spec(5, 4, hs, phis, 0.95), 6, ("full", "z_zz"),
                                          engine=stub, n_shots=3)
    assert out["full"].shape == (2, 4) and set(out) == {"full", "z_zz"}
    assert stub.calls[-1][2]["n_shots"] == 3


def test_sampled_refusals_without_a_device(pkg):
    """Raised before any engine is touched; DtcEngine.sample on an engine object
    that has no context."""
    en = pkg.energy
    L = 5
    hs, phis = random_disorder(np.random.default_rng(3), L, 1)
    dev = pkg.SweepSpec(L=L, T=4, hs=hs, phis=phis, device=harsh_device(pkg, L))
    bond = pkg.SweepSpec(L=L, T=4, hs=hs, phis=phis, bond_noise=0.02)
    bare = pkg.DtcEngine.__new__(pkg.DtcEngine)
    stub = _StubEngine()
    for spec, word in ((dev, "device-like noise"), (bond, "bond noise")):
        with pytest.raises(NotImplementedError, match=word):
            bare.sample(spec, 2)
        with pytest.raises(NotImplementedError, match=word):
            en.get_instances_energy_sampled(spec, 2, engine=stub)
    with pytest.raises(NotImplementedError, match="bond noise"):
        en.run_energy(L, 0.95, hs, phis, 4, nprobs=(0.01,), n_traj=4, engine=stub, sampled=True,
                      bond_noise=0.02)
    cal = pkg.device_noise.DeviceCalibration.from_json(pkg.cli.DEFAULT_CALIBRATION)
    with pytest.raises(NotImplementedError, match="device-like noise"):
        en.run_energy(L, 0.95, hs, phis, 4, nprobs=(0.01,), n_traj=4, engine=stub, sampled=True,
                      calibration=cal)
    with pytest.raises(NotImplementedError, match="echo"):
        en.run_energy(L, 0.95, hs, phis, 4, nprobs=(0.01,), n_traj=4, engine=stub, sampled=True,
                      echo=True)
    assert stub.calls == []
    with pytest.raises(ValueError, match="bases"):
        bare.sample(pkg.SweepSpec(L=L, T=4, hs=hs, phis=phis), 2, bases="y")


def test_energy_csv_name_and_cli_sampled(pkg, tmp_path):
    args = ("energy_data", "neel", 0.97, 5, 1, 1, 0.0, 1.0, 0.05, 1)
    plain = pkg.energy.energy_csv_name(*args)
    assert pkg.energy.energy_csv_name(*args, sampled=False) == plain
    assert pkg.energy.energy_csv_name(*args, sampled=True) == plain[:-4] + "_sampled.csv"
    bond = pkg.energy.energy_csv_name(*args, bond_noise_prob=0.01, sampled=True)
    assert bond.endswith("_bond0.01_sampled.csv")
    p = pkg.energy_cli.build_parser()
    assert p.parse_args([]).sampled == 0 and p.parse_args(["--sampled", "1"]).sampled == 1
    # refused before the disorder is used or an engine opened
    import pandas as pd

    dis = tmp_path / "dis"
    dis.mkdir()
    hs, phis = random_disorder(np.random.default_rng(6), 5)
    pd.DataFrame(hs).to_csv(dis / "hs_L5.csv", index=False)
    pd.DataFrame(phis).to_csv(dis / "phis_L5.csv", index=False)
    common = ["--L", "5", "--tf", "4", "--trajectories", "4", "--disorder_folder", str(dis),
              "--out_dir", str(tmp_path / "no"), "--sampled", "1"]
    for extra in (["--echo", "1"], ["--use_fakebackend", "1"], ["--bond_noise_prob", "0.01"],
                  ["--mode", "fakebrisbane"]):
        with pytest.raises(SystemExit, match="does not support"):
            pkg.energy_cli.main(common + extra)
    assert not (tmp_path / "no").exists()
