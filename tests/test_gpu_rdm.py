"""dtc_rdm (HIP): the reduced density matrix of site windows of every
trajectory's state at every time point of the forward sweep.

Against the gate-by-gate oracle (tests/rdm_model.py: the trajectory's states
from the C oracle, rho by numpy reshape and matmul) at eps = 1e-10, the
project's standing figure for engine against oracle; rows are bit-identical
under batching, trajectory splits and both batch layouts; one- and two-site
matrices reproduce dtc_energy's and dtc_correlations' numbers.

The four-site windows of the parity test are generic Hermitian 16 x 16 matrices
with no symmetry between rows, so they pin the accumulator (C/D) lane map of the
FP64 MFMA: a store by another map moves entries between rows and misses the
bound by orders of magnitude.
"""
import os

import numpy as np
import pytest

from tests import correlation_model as cm
from tests import rdm_model as rm
from tests import sample_model as sm
from tests.helpers import random_disorder

pytestmark = pytest.mark.gpu


def _states(spec, inst, tid, seed):
    return list(sm.trajectory_states(spec, inst, tid, seed))


def _check_rows(got, states, L, windows, what):
    """got [T][n_win][d][d] of one trajectory against rho of the oracle's states."""
    worst = 0.0
    for t, psi in states:
        for w, sites in enumerate(windows):
            want = rm.state_rdm(psi, L, sites)
            worst = max(worst, float(np.max(np.abs(got[t, w] - want))))
    print(f"{what}: largest deviation {worst:.3e}")
    assert worst <= rm.EPS, what


def _check_form(rho):
    """Hermitian bit for bit, the diagonal exactly real."""
    assert np.array_equal(rho, np.conj(np.swapaxes(rho, -1, -2)))
    d = np.arange(rho.shape[-1])
    assert np.all(rho[..., d, d].imag == 0.0)


# workgroups per state (8 tiles of 4096 amplitudes each, or all of a smaller state):
@pytest.mark.parametrize("L,T,pol,state,n", [
    (5, 4, "x", "neel", 3),       # one tile, pad bits beyond the state's sites
    (13, 4, "y", "vacuum", 3),    # two tiles, one workgroup
    (16, 3, "x", "vacuum", 2),    # two workgroups
    (21, 3, "x", "neel", 2),      # 64 workgroups: the reduce loops
])
def test_rdm_matches_oracle(pkg, engine, L, T, pol, state, n):
    rng = np.random.default_rng(L + 900)
    hs, phis = random_disorder(rng, L)
    spec = pkg.energy.energy_spec(L, T, hs, phis, 0.94, state, noise_prob=0.05, polarization=pol)
    states = [_states(spec, 0, tr, 21) for tr in range(n)]
    for k, windows in rm.standard_windows(L).items():
        got = engine.rdm(spec, n, windows, seed=21)
        d = 1 << k
        assert got.shape == (1, n, T, len(windows), d, d) and got.dtype == np.complex128
        _check_form(got)
        for tr in range(n):
            _check_rows(got[0, tr], states[tr], L, windows, f"L={L} k={k} traj {tr}")


def test_rdm_L20_both_layouts(pkg, engine):
    """L = 20: eight trajectories in one batch run in the octet layout, in
    batches of four contiguous; the rows are the same bits, and the oracle's."""
    rng = np.random.default_rng(2320)
    L = 20
    hs, phis = random_disorder(rng, L, 1)
    spec = pkg.SweepSpec(L=L, T=3, hs=hs, phis=phis, g=0.97, noise_prob=0.05, polarization="x")
    windows = [(0, 1, 2, 3), (16, 17, 18, 19), (3, 7, 18, 19), (2, 5, 11, 14)]
    a8 = engine.rdm(spec, 8, windows, seed=33, batch=8)
    a4 = engine.rdm(spec, 8, windows, seed=33, batch=4)
    assert np.array_equal(a8, a4)
    for tr in (0, 7):
        _check_rows(a8[0, tr], _states(spec, 0, tr, 33), L, windows, f"L=20 traj {tr}")


@pytest.mark.parametrize("L,pol,state", [(9, "y", "neel"), (14, "x", "vacuum")])
def test_rdm_octet_layout(pkg, engine, L, pol, state):
    """Nine trajectories in one batch run in the octet layout (a full octet and
    a partial one), in batches of three contiguous; the rows are the same bits,
    and trajectory 8 (the partial octet's) is the oracle's."""
    rng = np.random.default_rng(L + 940)
    hs, phis = random_disorder(rng, L)
    spec = pkg.energy.energy_spec(L, 3, hs, phis, 0.94, state, noise_prob=0.1, polarization=pol)
    st8 = _states(spec, 0, 8, 35)
    for k, windows in rm.standard_windows(L).items():
        a9 = engine.rdm(spec, 9, windows, seed=35, batch=0)
        a3 = engine.rdm(spec, 9, windows, seed=35, batch=3)
        assert np.any(a9[:, :, 1:] != 0.0)
        assert np.array_equal(a9, a3), k
        _check_rows(a9[0, 8], st8, L, windows, f"L={L} k={k} traj 8")


def test_rdm_invariance(pkg, engine):
    rng = np.random.default_rng(43)
    L, n = 13, 24
    hs, phis = random_disorder(rng, L, 2)
    spec = pkg.SweepSpec(L=L, T=4, hs=hs, phis=phis, g=0.95, noise_prob=0.05)
    windows = [(0, 1, 2, 3), (9, 10, 11, 12), (1, 6, 11, 12)]
    a = engine.rdm(spec, n, windows, seed=8, batch=24)
    b = engine.rdm(spec, n, windows, seed=8, batch=8)
    lo = engine.rdm(spec, 12, windows, seed=8, traj_offset=0)
    hi = engine.rdm(spec, 12, windows, seed=8, traj_offset=12)
    assert np.any(a[:, :, 1:].imag != 0.0)
    assert np.array_equal(a, b)
    assert np.array_equal(a[:, :12], lo)
    assert np.array_equal(a[:, 12:], hi)
    # a window alone gives the rows it gives among others
    assert np.array_equal(engine.rdm(spec, n, windows[2], seed=8)[:, :, :, 0], a[:, :, :, 2])


@pytest.mark.parametrize("L", [7, 14])
def test_rdm_consistent_with_energy_and_correlations(pkg, engine, L):
    """One-site rho gives engine.energy's z and x, two-site rho gives
    engine.correlations' zz and xx; Tr rho = 1."""
    en = pkg.entanglement
    rng = np.random.default_rng(18 + L)
    hs, phis = random_disorder(rng, L, 2)
    spec = pkg.SweepSpec(L=L, T=4, hs=hs, phis=phis, g=0.97, noise_prob=0.1)
    n = 5
    ref = engine.energy(spec, n, seed=3)
    cor = engine.correlations(spec, n, bases="zx", seed=3)
    one = engine.rdm(spec, n, [(i,) for i in range(L)], seed=3)
    e1 = en.pauli_expectations(one)          # [inst][traj][T][L][4]
    i, j = cm.pairs(L)
    two = engine.rdm(spec, n, list(zip(i.tolist(), j.tolist())), seed=3)
    e2 = en.pauli_expectations(two)          # [inst][traj][T][pairs][16]
    checks = (("trace 1", e1[..., 0], 1.0), ("trace 2", e2[..., 0], 1.0),
              ("z", e1[..., 3], ref["z"]), ("x", e1[..., 1], ref["x"]),
              ("zz", e2[..., 15], cor["zz"]), ("xx", e2[..., 5], cor["xx"]),
              ("z from pairs", e2[..., 3], cor["z"][..., i]))
    for what, a, b in checks:
        dev = float(np.max(np.abs(a - b)))
        print(f"L={L} {what}: largest deviation {dev:.3e}")
        assert dev <= rm.EPS, what
    # the X rows of p = 0 are 0 by the energy contract, and rho's too (a basis state)
    assert not e1[:, :, 0, :, 1].any()
    # the one-site matrix is the partial trace of the two-site one
    p01 = int(np.flatnonzero((i == 0) & (j == 1))[0])
    assert np.max(np.abs(en.partial_trace(two[..., p01, :, :], [1]) - one[..., 1, :, :])) <= rm.EPS


def test_rdm_sums(pkg, engine):
    rng = np.random.default_rng(79)
    L, n = 13, 10
    hs, phis = random_disorder(rng, L, 3)
    spec = pkg.SweepSpec(L=L, T=4, hs=hs, phis=phis, g=0.95, noise_prob=0.05,
                         initial_state="neel")
    windows = [(0, 1, 2), (4, 8, 12)]
    rows = engine.rdm(spec, n, windows, seed=6)
    for batch in (0, 8):  # one batch; batches that cut through the instances
        sums = engine.rdm_sums(spec, n, windows, seed=6, batch=batch)
        assert sums.shape == rows.shape[:1] + rows.shape[2:]
        dev = float(np.max(np.abs(sums - rows.sum(axis=1))))
        print(f"batch {batch}: largest deviation {dev:.3e}")
        assert dev <= rm.EPS * n, batch
    res = pkg.entanglement.get_instances_rdm(spec, n, windows, seed=6, engine=engine)
    mean = rows.mean(axis=1)
    assert res["rho"].shape == (3, 4, 2, 8, 8)
    assert res["entropy"].shape == (3, 4, 2) and res["purity"].shape == (3, 4, 2)
    assert res["windows"].tolist() == [[0, 1, 2], [4, 8, 12]]
    assert np.max(np.abs(res["rho"] - mean)) <= rm.EPS
    assert np.max(np.abs(res["purity"] - pkg.entanglement.purity(mean))) <= 10 * rm.EPS
    # ten noisy trajectories: the mean state is mixed after the first period, and
    # its entropy is bounded by ln(min(n, d))
    assert np.all(res["purity"][:, 1:] < 1.0 - 1e-6)
    assert np.all(res["entropy"][:, 1:] > 1e-6)
    assert np.all(res["entropy"] <= np.log(8) + 1e-9)


def test_rdm_t_offset_and_t_first(pkg, engine):
    rng = np.random.default_rng(37)
    L = 13
    hs, phis = random_disorder(rng, L)
    plain = pkg.SweepSpec(L=L, T=5, hs=hs, phis=phis, g=0.95, noise_prob=0.05)
    shifted = pkg.SweepSpec(L=L, T=4, hs=hs, phis=phis, g=0.95, noise_prob=0.05, t_offset=1)
    windows = [(0, 5), (11, 12)]
    a = engine.rdm(plain, 3, windows, seed=9)
    b = engine.rdm(shifted, 3, windows, seed=9)
    late = engine.rdm(plain, 3, windows, seed=9, t_first=2)
    assert np.any(b != 0.0)
    assert np.array_equal(b, a[:, :, 1:])
    assert not late[:, :, :2].any()
    assert np.array_equal(late[:, :, 2:], a[:, :, 2:])
    _check_rows(b[0, 1], _states(shifted, 0, 1, 9), L, windows, "t_offset 1, traj 1")


@pytest.mark.parametrize("L,state", [(5, "neel"), (13, "vacuum"), (13, "neel")])
def test_rdm_noiseless_initial_row(pkg, engine, L, state):
    rng = np.random.default_rng(57 + L)
    hs, phis = random_disorder(rng, L)
    spec = pkg.energy.energy_spec(L, 3, hs, phis, 0.95, state, noise_prob=0.0, use_noise=0)
    windows = [(0, 1, 2), (1, 2, L - 1)]
    got = engine.rdm(spec, 2, windows, seed=3)
    m = spec.init_mask
    for w, sites in enumerate(windows):
        al = sum(((m >> s) & 1) << q for q, s in enumerate(sites))
        want = np.zeros((8, 8), dtype=np.complex128)
        want[al, al] = 1.0
        assert np.all(got[:, :, 0, w] == want)
    sums = engine.rdm_sums(spec, 2, windows, seed=3)
    assert np.array_equal(sums[:, 0], 2.0 * got[:, 0, 0])
    # a pure state all along: every window's rho has the spectrum of its complement
    assert np.max(np.abs(np.trace(got, axis1=-2, axis2=-1) - 1.0)) <= rm.EPS
    for tr in range(2):
        _check_rows(got[0, tr], _states(spec, 0, tr, 3), L, windows, f"noiseless L={L}")


def test_rdm_einval_with_a_device(pkg, engine):
    """The window checks of dtc_rdm itself (dtc_rdm_state's: test_rdm_cpu.py)."""
    rng = np.random.default_rng(5)
    L = 5
    hs, phis = random_disorder(rng, L)
    spec = pkg.SweepSpec(L=L, T=3, hs=hs, phis=phis, g=0.95, noise_prob=0.05)
    for bad in ([(0, 5)], [(-1, 2)], [(2, 2)], [(3, 1)], [(0, 1), (4, 3)]):
        with pytest.raises(pkg._capi.DtcError):
            engine.rdm(spec, 2, bad, seed=1)
    small = pkg.SweepSpec(L=3, T=3, hs=hs[:, :3], phis=phis[:, :2], g=0.95, noise_prob=0.05)
    with pytest.raises(pkg._capi.DtcError):
        engine.rdm(small, 2, [(0, 1, 2, 3)], seed=1)
    assert engine.rdm(small, 2, [(0, 1, 2)], seed=1).shape == (1, 2, 3, 1, 8, 8)


def test_rdm_profiling_books_reduce(pkg):
    """The launches are booked under the reduce kind: two per measured state and
    window, the Gram kernel with 16 B per amplitude."""
    rng = np.random.default_rng(14)
    L, T, n = 16, 4, 2
    hs, phis = random_disorder(rng, L)
    spec = pkg.SweepSpec(L=L, T=T, hs=hs, phis=phis, g=0.95, noise_prob=0.05)
    windows = [(0, 1), (3, 15), (7, 8)]
    with pkg.DtcEngine(0) as eng:
        eng.set_profiling(True)
        eng.rdm(spec, n, windows, seed=1)
        st = eng.kernel_stats()[pkg._capi.KERNEL_REDUCE]
    assert st["launches"] == 2 * len(windows) * (T - 1)
    n_wg = (1 << (L - 12)) // 8
    per = 16.0 * (1 << L) * n + 8.0 * n * (n_wg * 512 + 2 * 4 * 4)
    assert st["bytes"] == pytest.approx(len(windows) * (T - 1) * per)


def test_entanglement_cli(pkg, tmp_path):
    import pandas as pd

    dis = tmp_path / "dis"
    dis.mkdir()
    rng = np.random.default_rng(6)
    L, T = 5, 6
    hs, phis = random_disorder(rng, L)
    pd.DataFrame(hs).to_csv(dis / "hs_L5.csv", index=False)
    pd.DataFrame(phis).to_csv(dis / "phis_L5.csv", index=False)
    out = tmp_path / "out"
    assert pkg.entanglement_cli.main([
        "--L", "5", "--tf", str(T), "--trajectories", "32", "--disorder_folder", str(dis),
        "--out_dir", str(out), "--window_size", "2", "--window_stride", "3",
        "--initial_state", "neel"]) == 0
    folder = out / "entanglement-data_L5"
    files = sorted(os.listdir(folder))
    assert len(files) == 2
    csv = [f for f in files if f.endswith(".csv")]
    assert len(csv) == 1 and csv[0].startswith("entanglement_data_neel_g0.97_L5_inst1_tf6_")
    df = pd.read_csv(folder / csv[0])
    assert list(df.columns) == ["time", "entropy_s0-1", "entropy_s3-4", "purity_s0-1",
                                "purity_s3-4"]
    assert len(df) == T and np.all(np.isfinite(df.values))
    assert np.all(df.values[:, 1:3] >= 0.0) and np.all(df.values[:, 1:3] <= np.log(4) + 1e-9)
    assert np.all(df.values[:, 3:] >= 0.25 - 1e-9) and np.all(df.values[:, 3:] <= 1.0 + 1e-9)
    npy = [f for f in files if f.startswith("entanglement_rho_") and f.endswith(".npy")]
    assert len(npy) == 1
    m = np.load(folder / npy[0])
    assert m.shape == (T, 2, 4, 4) and m.dtype == np.complex128
    assert np.array_equal(m, np.conj(np.swapaxes(m, -1, -2)))
    assert np.max(np.abs(np.trace(m, axis1=-2, axis2=-1) - 1.0)) <= rm.EPS
    # without noise one trajectory runs: t = 0 is a basis state, purity 1 and entropy 0
    out0 = tmp_path / "out0"
    assert pkg.entanglement_cli.main([
        "--L", "5", "--tf", "3", "--use_noise", "0", "--disorder_folder", str(dis),
        "--out_dir", str(out0), "--window_sites", "0,2,4"]) == 0
    f0 = [f for f in os.listdir(out0 / "entanglement-data_L5") if f.endswith(".csv")]
    d0 = pd.read_csv(out0 / "entanglement-data_L5" / f0[0])
    assert list(d0.columns) == ["time", "entropy_s0-2-4", "purity_s0-2-4"]
    assert d0["purity_s0-2-4"][0] == 1.0 and d0["entropy_s0-2-4"][0] == 0.0
