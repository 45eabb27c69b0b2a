"""dtc_correlations (HIP): <Z_i>, <Z_i Z_j>, <X_i>, <X_i X_j> over all pairs of
every trajectory's state at every time point of the forward sweep.

Against the gate-by-gate oracle (tests/correlation_model.py: the trajectory's
states from the C oracle, the correlators by direct numpy sums, H^L for the X
basis) at eps = 1e-10, the project's standing figure for engine against oracle;
rows are bit-identical under batching, trajectory splits and both batch layouts;
the nearest-neighbour entries are dtc_energy's.
"""
import os

import numpy as np
import pytest

from tests import correlation_model as cm
from tests.helpers import random_disorder

pytestmark = pytest.mark.gpu

KEYS = ("z", "zz", "x", "xx")


def _check_traj(got, spec, inst, tid, seed, row=None, keys=KEYS):
    r = tid if row is None else row
    want = cm.trajectory_rows(spec, inst, tid, seed, bases="".join(k for k in "zx" if k in keys))
    worst = 0.0
    for k in keys:
        if want[k].size:
            worst = max(worst, float(np.max(np.abs(got[k][inst, r] - want[k]))))
    print(f"L={spec.L} inst {inst} traj {tid}: largest deviation {worst:.3e}")
    assert worst <= cm.EPS, (spec.L, inst, tid)


@pytest.mark.parametrize("L,T,pol,state,n", [
    (5, 4, "x", "neel", 3),       # one chunk, seven padding sites
    (13, 4, "y", "vacuum", 3),    # one global bit
    (14, 3, "x", "vacuum", 2),    # two global bits: every class of pair
    (21, 3, "x", "neel", 2),      # a further group split
])
def test_correlations_match_oracle(pkg, engine, L, T, pol, state, n):
    rng = np.random.default_rng(L + 700)
    hs, phis = random_disorder(rng, L)
    spec = pkg.energy.energy_spec(L, T, hs, phis, 0.94, state, noise_prob=0.05, polarization=pol)
    got = engine.correlations(spec, n, bases="zx", seed=21)
    assert set(got) == set(KEYS)
    n_pair = L * (L - 1) // 2
    for k in KEYS:
        assert got[k].shape == (1, n, T, L if len(k) == 1 else n_pair)
    for tr in range(n):
        _check_traj(got, spec, 0, tr, 21)


def test_correlations_L20_both_layouts(pkg, engine):
    """L = 20: eight trajectories in one batch run in the octet layout, in
    batches of four contiguous; the rows are the same bits, and the oracle's."""
    rng = np.random.default_rng(2120)
    hs, phis = random_disorder(rng, 20, 1)
    spec = pkg.SweepSpec(L=20, T=3, hs=hs, phis=phis, g=0.97, noise_prob=0.05, polarization="x")
    a8 = engine.correlations(spec, 8, bases="zx", seed=33, batch=8)
    a4 = engine.correlations(spec, 8, bases="zx", seed=33, batch=4)
    for k in KEYS:
        assert np.array_equal(a8[k], a4[k]), k
    for tr in (0, 7):
        _check_traj(a8, spec, 0, tr, 33)


@pytest.mark.parametrize("L,pol,state", [(9, "y", "neel"), (14, "x", "vacuum")])
def test_correlations_octet_layout(pkg, engine, L, pol, state):
    """One chunk per state (L = 9) and two global bits (L = 14): nine
    trajectories in one batch run in the octet layout (a full octet and a
    partial one), in batches of three contiguous; the rows are the same bits,
    and trajectory 8 (the partial octet's) is the oracle's."""
    rng = np.random.default_rng(L + 740)
    hs, phis = random_disorder(rng, L)
    spec = pkg.energy.energy_spec(L, 3, hs, phis, 0.94, state, noise_prob=0.1, polarization=pol)
    a9 = engine.correlations(spec, 9, bases="zx", seed=35, batch=0)
    a3 = engine.correlations(spec, 9, bases="zx", seed=35, batch=3)
    for k in KEYS:
        assert np.any(a9[k][:, :, 1:] != 0.0), k
        assert np.array_equal(a9[k], a3[k]), k
    _check_traj(a9, spec, 0, 8, 35)


def test_correlations_invariance(pkg, engine):
    rng = np.random.default_rng(41)
    L, n = 13, 24
    hs, phis = random_disorder(rng, L, 2)
    spec = pkg.SweepSpec(L=L, T=4, hs=hs, phis=phis, g=0.95, noise_prob=0.05)
    a = engine.correlations(spec, n, bases="zx", seed=8, batch=24)
    b = engine.correlations(spec, n, bases="zx", seed=8, batch=8)
    lo = engine.correlations(spec, 12, bases="zx", seed=8, traj_offset=0)
    hi = engine.correlations(spec, 12, bases="zx", seed=8, traj_offset=12)
    for k in KEYS:
        assert np.any(a[k][:, :, 1:] != 0.0), k
        assert np.array_equal(a[k], b[k]), k
        assert np.array_equal(a[k][:, :12], lo[k]), k
        assert np.array_equal(a[k][:, 12:], hi[k]), k


@pytest.mark.parametrize("L", [7, 14])
def test_correlations_same_trajectories_as_energy(pkg, engine, L):
    rng = np.random.default_rng(8 + L)
    hs, phis = random_disorder(rng, L, 2)
    spec = pkg.SweepSpec(L=L, T=4, hs=hs, phis=phis, g=0.97, noise_prob=0.1)
    got = engine.correlations(spec, 5, bases="zx", seed=3)
    ref = engine.energy(spec, 5, seed=3)
    i, j = cm.pairs(L)
    nn = np.flatnonzero(j == i + 1)
    assert nn.size == L - 1
    for what, a, b in (("z", got["z"], ref["z"]), ("zz", got["zz"][..., nn], ref["zz"]),
                       ("x", got["x"], ref["x"])):
        dev = float(np.max(np.abs(a - b)))
        print(f"L={L} {what}: largest deviation from engine.energy {dev:.3e}")
        assert dev <= cm.EPS, what
    # single-basis calls return the same rows
    z = engine.correlations(spec, 5, bases="z", seed=3)
    x = engine.correlations(spec, 5, bases="x", seed=3)
    assert set(z) == {"z", "zz"} and set(x) == {"x", "xx"}
    for k in KEYS:
        assert np.array_equal((z if k in z else x)[k], got[k]), k


def test_correlation_sums(pkg, engine):
    rng = np.random.default_rng(77)
    L, n = 13, 10
    hs, phis = random_disorder(rng, L, 3)
    spec = pkg.SweepSpec(L=L, T=4, hs=hs, phis=phis, g=0.95, noise_prob=0.05,
                         initial_state="neel")
    rows = engine.correlations(spec, n, bases="zx", seed=6)
    for batch in (0, 8):  # one batch; batches that cut through the instances
        sums = engine.correlation_sums(spec, n, bases="zx", seed=6, batch=batch)
        assert set(sums) == set(KEYS)
        for k in KEYS:
            assert sums[k].shape == rows[k].shape[:1] + rows[k].shape[2:]
            dev = float(np.max(np.abs(sums[k] - rows[k].sum(axis=1))))
            print(f"batch {batch} {k}: largest deviation {dev:.3e}")
            assert dev <= cm.EPS * n, (batch, k)
    res = pkg.correlations.get_instances_correlations(spec, n, bases="zx", seed=6, engine=engine)
    assert res["zz"].shape == (3, 4, L, L) and res["chi_sg_z"].shape == (3, 4)
    want = pkg.correlations.pair_matrix(rows["zz"].mean(axis=1), L)
    assert np.max(np.abs(res["zz"] - want)) <= cm.EPS
    assert np.max(np.abs(res["chi_sg_x"] - pkg.correlations.spin_glass_order(
        pkg.correlations.pair_matrix(rows["xx"].mean(axis=1), L)))) <= cm.EPS


def test_correlations_t_offset_and_t_first(pkg, engine):
    rng = np.random.default_rng(31)
    L = 13
    hs, phis = random_disorder(rng, L)
    plain = pkg.SweepSpec(L=L, T=5, hs=hs, phis=phis, g=0.95, noise_prob=0.05)
    shifted = pkg.SweepSpec(L=L, T=4, hs=hs, phis=phis, g=0.95, noise_prob=0.05, t_offset=1)
    a = engine.correlations(plain, 3, bases="zx", seed=9)
    b = engine.correlations(shifted, 3, bases="zx", seed=9)
    late = engine.correlations(plain, 3, bases="zx", seed=9, t_first=2)
    for k in KEYS:
        assert np.any(b[k] != 0.0), k
        assert np.array_equal(b[k], a[k][:, :, 1:]), k
        assert not late[k][:, :, :2].any(), k
        assert np.array_equal(late[k][:, :, 2:], a[k][:, :, 2:]), k
    _check_traj(b, shifted, 0, 1, 9)


@pytest.mark.parametrize("L,state", [(5, "neel"), (13, "vacuum"), (13, "neel")])
def test_correlations_noiseless_initial_row(pkg, engine, L, state):
    rng = np.random.default_rng(55 + L)
    hs, phis = random_disorder(rng, L)
    spec = pkg.energy.energy_spec(L, 3, hs, phis, 0.95, state, noise_prob=0.0, use_noise=0)
    got = engine.correlations(spec, 2, bases="zx", seed=3)
    m = spec.init_mask
    s = np.array([1.0 - 2.0 * ((m >> i) & 1) for i in range(L)])
    i, j = cm.pairs(L)
    assert np.all(got["z"][:, :, 0] == s)
    assert np.all(got["zz"][:, :, 0] == s[i] * s[j])
    assert not got["x"][:, :, 0].any() and not got["xx"][:, :, 0].any()
    sums = engine.correlation_sums(spec, 2, bases="zx", seed=3)
    assert np.all(sums["zz"][:, 0] == 2.0 * s[i] * s[j])
    C = pkg.correlations.pair_matrix(got["zz"][0, 0, 0], L)
    assert pkg.correlations.spin_glass_order(C) == pytest.approx(1.0, abs=1e-15)


def test_correlations_profiling_books_reduce(pkg):
    """The correlator launches are booked under the reduce kind: two per measured
    state and basis, the chunk kernel with 16 B per amplitude."""
    rng = np.random.default_rng(12)
    L, T, n = 13, 4, 2
    hs, phis = random_disorder(rng, L)
    spec = pkg.SweepSpec(L=L, T=T, hs=hs, phis=phis, g=0.95, noise_prob=0.05)
    n_col = L + L * (L - 1) // 2
    with pkg.DtcEngine(0) as eng:
        eng.set_profiling(True)
        eng.correlations(spec, n, bases="zx", seed=1)
        st = eng.kernel_stats()[pkg._capi.KERNEL_REDUCE]
        eng.reset_stats()
        eng.correlations(spec, n, bases="z", seed=1)
        st_z = eng.kernel_stats()[pkg._capi.KERNEL_REDUCE]
    assert st["launches"] == 2 * 2 * (T - 1) and st_z["launches"] == 2 * (T - 1)
    per = 16.0 * (1 << L) * n + 8.0 * n * (2 * 79 + n_col)
    assert st["bytes"] == pytest.approx(2 * (T - 1) * per)
    assert st_z["bytes"] == pytest.approx((T - 1) * per)


def test_correlation_cli(pkg, tmp_path):
    import pandas as pd

    dis = tmp_path / "dis"
    dis.mkdir()
    rng = np.random.default_rng(6)
    L, T = 5, 6
    hs, phis = random_disorder(rng, L)
    pd.DataFrame(hs).to_csv(dis / "hs_L5.csv", index=False)
    pd.DataFrame(phis).to_csv(dis / "phis_L5.csv", index=False)
    out = tmp_path / "out"
    assert pkg.correlation_cli.main([
        "--L", "5", "--tf", str(T), "--trajectories", "32", "--disorder_folder", str(dis),
        "--out_dir", str(out), "--bases", "zx", "--initial_state", "neel"]) == 0
    folder = out / "correlation-data_L5"
    files = sorted(os.listdir(folder))
    assert len(files) == 3
    csv = [f for f in files if f.endswith(".csv")]
    assert len(csv) == 1 and csv[0].startswith("correlation_data_neel_g0.97_L5_inst1_tf6_")
    df = pd.read_csv(folder / csv[0])
    assert list(df.columns) == ["time", "chi_sg_z", "chi_sg_z_connected", "chi_sg_x"]
    assert len(df) == T and np.all(np.isfinite(df.values))
    # t = 0: a basis state up to the preparation's noise (32 trajectories of the
    # neel state at p = 0.05: chi_SG of the mean matrix stays near 1; exactly 1
    # without noise, test_correlations_noiseless_initial_row)
    assert 0.5 < df["chi_sg_z"][0] <= 1.0 + 1e-12
    assert df["chi_sg_x"][0] == 0.0
    for b in "zx":
        name = [f for f in files if f.startswith(f"correlation_matrix_{b}_")]
        assert len(name) == 1
        m = np.load(folder / name[0])
        assert m.shape == (T, L, L)
        assert np.array_equal(m, np.swapaxes(m, 1, 2))
    # without noise one trajectory runs and chi_SG(0) is 1
    out0 = tmp_path / "out0"
    assert pkg.correlation_cli.main([
        "--L", "5", "--tf", "3", "--use_noise", "0", "--disorder_folder", str(dis),
        "--out_dir", str(out0)]) == 0
    f0 = [f for f in os.listdir(out0 / "correlation-data_L5") if f.endswith(".csv")]
    d0 = pd.read_csv(out0 / "correlation-data_L5" / f0[0])
    assert list(d0.columns) == ["time", "chi_sg_z", "chi_sg_z_connected"]
    assert d0["chi_sg_z"][0] == pytest.approx(1.0, abs=1e-15)
    assert d0["chi_sg_z_connected"][0] == pytest.approx(0.0, abs=1e-15)
