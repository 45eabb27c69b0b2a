"""dtc_rdm_block_sums (HIP): the reduced density matrix of blocks of 5..10
contiguous sites -- the trajectory sums per instance and the purity of every
trajectory's own state -- at every time point of the forward sweep.

Against the gate-by-gate oracle (tests/sample_model.trajectory_states,
tests/rdm_model.state_rdm) at eps = 1e-10, the project's standing figure for
engine against oracle.  The states are generic (p = 0.05, disordered angles), so
the matrices have no symmetry between rows: a wrong accumulator (C/D) or tile
map moves entries between rows and misses the bound by orders of magnitude.
Purity rows are bit-identical under batching, trajectory splits and both batch
layouts; the sums agree to 1e-12.
"""
import numpy as np
import pytest

from tests import rdm_model as rm
from tests import sample_model as sm
from tests.helpers import random_disorder

pytestmark = pytest.mark.gpu


def _sites(a, k):
    return list(range(a, a + k))


def _check_form(rho):
    """Hermitian bit for bit, the diagonal exactly real."""
    assert np.array_equal(rho, np.conj(np.swapaxes(rho, -1, -2)))
    d = np.arange(rho.shape[-1])
    assert np.all(rho[..., d, d].imag == 0.0)


@pytest.mark.parametrize("L,T,pol,state,k,starts,n", [
    (10, 4, "x", "neel", 5, (0, 5, 2), 1),      # padded to L_eff = 12; the pad bit above
    (13, 3, "y", "vacuum", 6, (0, 7, 3), 1),    # one tile, two chunks
    (16, 3, "x", "vacuum", 8, (0, 8, 5), 1),    # ten tiles of four panels
    (16, 3, "y", "neel", 6, (0, 10, 5), 1),     # four column splits: the finish kernel
    (16, 3, "x", "neel", 7, (0, 9, 4), 1),      # three tiles, two splits
    (20, 3, "x", "vacuum", 10, (0, 10), 2),     # 136 tiles, straight into the work matrix
])
def test_rdm_block_matches_oracle(pkg, engine, L, T, pol, state, k, starts, n):
    rng = np.random.default_rng(L + 1900)
    hs, phis = random_disorder(rng, L)
    spec = pkg.SweepSpec(L=L, T=T, hs=hs, phis=phis, g=0.94, noise_prob=0.05, polarization=pol,
                         initial_state=state)
    blocks = [(a, k) for a in starts]
    got = engine.rdm_block_sums(spec, n, blocks, seed=21)
    d = 1 << k
    assert got["rho_sum"].shape == (1, T, len(starts), d, d)
    assert got["rho_sum"].dtype == np.complex128
    assert got["purity"].shape == (1, n, T, len(starts))
    assert got["blocks"].tolist() == [[a, k] for a in starts]
    _check_form(got["rho_sum"])
    want_sum = np.zeros((T, len(starts), d, d), dtype=np.complex128)
    worst_p = 0.0
    for tr in range(n):
        for t, psi in sm.trajectory_states(spec, 0, tr, 21):
            for w, a in enumerate(starts):
                rho = rm.state_rdm(psi, L, _sites(a, k))
                want_sum[t, w] += rho
                want_p = float((rho.real ** 2 + rho.imag ** 2).sum())
                worst_p = max(worst_p, abs(got["purity"][0, tr, t, w] - want_p))
    worst = float(np.max(np.abs(got["rho_sum"][0] - want_sum)))
    print(f"L={L} k={k}: rho_sum deviates by {worst:.3e}, purity by {worst_p:.3e}")
    assert worst <= rm.EPS
    assert worst_p <= rm.EPS
    # the states are entangled and generic: nothing here is a basis state's answer
    assert np.all(got["purity"][:, :, 1:] < 1.0 - 1e-6)
    assert np.any(np.abs(got["rho_sum"][:, 1:].imag) > 1e-6)


def test_rdm_block_sum_of_trajectories(pkg, engine):
    """rho_sum of three trajectories is the sum of three one-trajectory calls."""
    rng = np.random.default_rng(1913)
    L, k = 13, 6
    hs, phis = random_disorder(rng, L)
    spec = pkg.SweepSpec(L=L, T=3, hs=hs, phis=phis, g=0.95, noise_prob=0.05)
    blocks = [(0, k), (7, k), (3, k)]
    all3 = engine.rdm_block_sums(spec, 3, blocks, seed=5)
    one = [engine.rdm_block_sums(spec, 1, blocks, seed=5, traj_offset=tr) for tr in range(3)]
    dev = float(np.max(np.abs(all3["rho_sum"] - sum(o["rho_sum"] for o in one))))
    print(f"sum of three calls: largest deviation {dev:.3e}")
    assert dev <= 1e-12
    for tr in range(3):
        assert np.array_equal(all3["purity"][:, tr], one[tr]["purity"][:, 0])


@pytest.mark.parametrize("L,k,starts,n", [(12, 5, (0, 7, 3), 3), (14, 7, (0, 7, 4), 2)])
def test_rdm_block_form(pkg, engine, L, k, starts, n):
    """Hermitian bit for bit, a real diagonal, trace n_traj, purities of a
    k-site state.  (L = 12, start 7, k = 5: the pad bit below the block.)"""
    rng = np.random.default_rng(L + 1920)
    hs, phis = random_disorder(rng, L, 2)
    spec = pkg.SweepSpec(L=L, T=4, hs=hs, phis=phis, g=0.95, noise_prob=0.05,
                         initial_state="neel", polarization="y")
    got = engine.rdm_block_sums(spec, n, [(a, k) for a in starts], seed=2)
    _check_form(got["rho_sum"])
    tr = np.trace(got["rho_sum"], axis1=-2, axis2=-1)
    assert np.max(np.abs(tr - n)) <= 1e-10
    assert np.all(got["purity"] > 2.0 ** -k) and np.all(got["purity"] <= 1.0 + 1e-12)
    assert np.all(got["purity"][:, :, 0] == 1.0)


def test_rdm_block_invariance(pkg, engine):
    rng = np.random.default_rng(1943)
    L, k, n = 13, 6, 24
    hs, phis = random_disorder(rng, L, 2)
    spec = pkg.SweepSpec(L=L, T=3, hs=hs, phis=phis, g=0.95, noise_prob=0.05)
    blocks = [(0, k), (7, k), (4, k)]
    a = engine.rdm_block_sums(spec, n, blocks, seed=8, batch=24)
    b = engine.rdm_block_sums(spec, n, blocks, seed=8, batch=8)
    lo = engine.rdm_block_sums(spec, 12, blocks, seed=8, traj_offset=0)
    hi = engine.rdm_block_sums(spec, 12, blocks, seed=8, traj_offset=12)
    assert np.all(a["purity"][:, :, 1:] < 1.0 - 1e-6)
    assert np.array_equal(a["purity"], b["purity"])
    assert np.array_equal(a["purity"][:, :12], lo["purity"])
    assert np.array_equal(a["purity"][:, 12:], hi["purity"])
    assert np.max(np.abs(a["rho_sum"] - b["rho_sum"])) <= 1e-12
    assert np.max(np.abs(a["rho_sum"] - (lo["rho_sum"] + hi["rho_sum"]))) <= 1e-12
    # a block alone gives what it gives among others
    alone = engine.rdm_block_sums(spec, n, blocks[2], seed=8, batch=24)
    assert np.array_equal(alone["purity"][..., 0], a["purity"][..., 2])
    assert np.max(np.abs(alone["rho_sum"][:, :, 0] - a["rho_sum"][:, :, 2])) <= 1e-12
    # nine trajectories in one batch run in the octet layout, in batches of three
    # contiguous (as test_rdm_octet_layout)
    o9 = engine.rdm_block_sums(spec, 9, blocks, seed=8, batch=0)
    o3 = engine.rdm_block_sums(spec, 9, blocks, seed=8, batch=3)
    assert np.array_equal(o9["purity"], o3["purity"])
    assert np.array_equal(o9["purity"], a["purity"][:, :9])
    assert np.max(np.abs(o9["rho_sum"] - o3["rho_sum"])) <= 1e-12


@pytest.mark.parametrize("k", [5, 7])
def test_rdm_block_consistent_with_windows(pkg, engine, k):
    """Tracing a block down to its four lowest sites gives dtc_rdm_sums' window."""
    rng = np.random.default_rng(1950 + k)
    L, n = 14, 5
    hs, phis = random_disorder(rng, L, 2)
    spec = pkg.SweepSpec(L=L, T=3, hs=hs, phis=phis, g=0.97, noise_prob=0.1)
    starts = (0, 3, L - k)
    blk = engine.rdm_block_sums(spec, n, [(a, k) for a in starts], seed=3)["rho_sum"]
    win = engine.rdm_sums(spec, n, [(a, a + 1, a + 2, a + 3) for a in starts], seed=3)
    dev = float(np.max(np.abs(pkg.entanglement.partial_trace(blk, [0, 1, 2, 3]) - win)))
    print(f"k={k}: largest deviation from the four-site windows {dev:.3e}")
    assert dev <= 1e-10 * n


@pytest.mark.parametrize("L,n", [(14, 3), (20, 1)])
def test_rdm_block_half_chain_symmetry(pkg, engine, L, n):
    """A pure state's two halves have the same purity."""
    rng = np.random.default_rng(1960 + L)
    hs, phis = random_disorder(rng, L)
    spec = pkg.SweepSpec(L=L, T=3, hs=hs, phis=phis, g=0.95, noise_prob=0.05)
    pur = engine.rdm_block_sums(spec, n, [(0, L // 2), (L // 2, L // 2)], seed=4)["purity"]
    assert np.all(pur[:, :, 1:] < 1.0 - 1e-6)
    dev = float(np.max(np.abs(pur[..., 0] - pur[..., 1])))
    print(f"L={L}: the halves' purities differ by {dev:.3e}")
    assert dev <= 1e-10


def test_rdm_block_known_answer(pkg, engine):
    """g = 1, no noise: the kicks are exact flips, the state stays a basis state."""
    rng = np.random.default_rng(1970)
    L, k, T = 12, 6, 4
    hs, phis = random_disorder(rng, L)
    spec = pkg.SweepSpec(L=L, T=T, hs=hs, phis=phis, g=1.0, noise_prob=0.0, use_noise=0)
    got = engine.rdm_block_sums(spec, 1, [(0, k), (6, k), (3, k)], seed=1)
    assert np.max(np.abs(got["purity"] - 1.0)) <= 1e-10
    ent = pkg.entanglement.von_neumann_entropy(got["rho_sum"])
    assert np.max(np.abs(ent)) <= 1e-10
    res = pkg.entanglement.get_instances_block(spec, 1, [(0, k)], seed=1, engine=engine)
    assert np.max(np.abs(res["renyi2_traj"])) <= 1e-10 and np.max(np.abs(res["entropy"])) <= 1e-10


def test_rdm_block_einval_with_a_device(pkg, engine):
    rng = np.random.default_rng(5)
    L = 12
    hs, phis = random_disorder(rng, L)
    spec = pkg.SweepSpec(L=L, T=3, hs=hs, phis=phis, g=0.95, noise_prob=0.05)
    for bad in ([(8, 5)], [(-1, 5)], [(0, 5), (9, 5)]):
        with pytest.raises(pkg._capi.DtcError):
            engine.rdm_block_sums(spec, 2, bad, seed=1)
    for bad in ([(0, 7)], [(0, 4)], [(0, 11)]):   # 2 k > L; k outside 5..10
        with pytest.raises((pkg._capi.DtcError, ValueError)):
            engine.rdm_block_sums(spec, 2, bad, seed=1)
    # T n_blk d d > 2^25: refused before any device call
    L = 20
    hs, phis = random_disorder(rng, L)
    big = pkg.SweepSpec(L=L, T=33, hs=hs, phis=phis, g=0.95, noise_prob=0.05)
    with pytest.raises(pkg._capi.DtcError, match="2\\^25"):
        engine.rdm_block_sums(big, 1, [(0, 10)], seed=1)


def test_rdm_block_profile(pkg, engine):
    """entanglement_profile: every cut of L = 11, sizes 1..5, through rdm and the
    block path; a noiseless run's Renyi-2 is that of the single state."""
    rng = np.random.default_rng(1980)
    L, T = 11, 3
    hs, phis = random_disorder(rng, L)
    spec = pkg.SweepSpec(L=L, T=T, hs=hs, phis=phis, g=0.95, noise_prob=0.0, use_noise=0)
    res = pkg.entanglement.entanglement_profile(spec, 1, seed=1, engine=engine)
    assert res["renyi2_traj"].shape == (1, T, L - 1) and res["entropy"].shape == (1, T, L - 1)
    for t, psi in sm.trajectory_states(spec, 0, 0, 1):
        for cut in range(1, L):
            sites = list(range(cut)) if cut <= L - cut else list(range(cut, L))
            rho = rm.state_rdm(psi, L, sites)
            want = -np.log((np.abs(rho) ** 2).sum())
            assert abs(res["renyi2_traj"][0, t, cut - 1] - want) <= 1e-9, (t, cut)
    assert np.all(res["entropy"] >= -1e-10)
    assert np.all(res["entropy"] + 1e-9 >= res["renyi2_traj"])


def test_entanglement_cli_blocks_and_profile(pkg, tmp_path):
    import os

    import pandas as pd

    dis = tmp_path / "dis"
    dis.mkdir()
    rng = np.random.default_rng(6)
    L, T = 10, 4
    hs, phis = random_disorder(rng, L)
    pd.DataFrame(hs).to_csv(dis / "hs_L10.csv", index=False)
    pd.DataFrame(phis).to_csv(dis / "phis_L10.csv", index=False)
    out = tmp_path / "out"
    assert pkg.entanglement_cli.main([
        "--L", "10", "--tf", str(T), "--trajectories", "8", "--disorder_folder", str(dis),
        "--out_dir", str(out), "--block_size", "5", "--block_start", "0", "--block_start", "5",
        "--profile", "1"]) == 0
    folder = out / "entanglement-data_L10"
    files = sorted(os.listdir(folder))
    assert len(files) == 3, files
    tail = "_vacuum_g0.97_L10_inst1_tf4_randomphi1_delta0.0_amplitude1.0_noise0.05_usenoise1"
    df = pd.read_csv(folder / ("entanglement_block_data" + tail + ".csv"))
    assert list(df.columns) == ["time", "entropy_b0-4", "entropy_b5-9", "purity_b0-4",
                                "purity_b5-9", "renyi2_traj_b0-4", "renyi2_traj_b5-9"]
    assert len(df) == T and np.all(np.isfinite(df.values))
    assert df["purity_b0-4"][0] == 1.0 and df["renyi2_traj_b5-9"][0] == 0.0
    # pure trajectories: the two halves have one Renyi-2 entropy
    assert np.max(np.abs(df["renyi2_traj_b0-4"] - df["renyi2_traj_b5-9"])) <= 1e-9
    m = np.load(folder / ("entanglement_block_rho" + tail + ".npy"))
    assert m.shape == (T, 2, 32, 32) and np.array_equal(m, np.conj(np.swapaxes(m, -1, -2)))
    assert np.max(np.abs(np.trace(m, axis1=-2, axis2=-1) - 1.0)) <= rm.EPS
    prof = pd.read_csv(folder / ("entanglement_profile" + tail + ".csv"))
    assert list(prof.columns) == ["time"] + [f"renyi2_traj_cut{c}" for c in range(1, L)]
    # the middle cut is the block [0, 5)
    assert np.max(np.abs(prof["renyi2_traj_cut5"] - df["renyi2_traj_b0-4"])) <= 1e-9
