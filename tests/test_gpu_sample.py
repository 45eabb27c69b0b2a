"""dtc_sample (HIP): Z- and X-basis bitstrings of every trajectory's state at
every time point of the forward sweep.

Per sample against the gate-by-gate oracle (tests/sample_model.py): with the
trajectory's state psi from the oracle and the shot's uniform u from
sample_draws, every returned x satisfies S(x - 1) - eps <= u W <= S(x) + eps on
psi (Z) or H^L psi (X), eps = 1e-10, the project's standing figure for engine
against oracle; rows are bit-identical under batching, trajectory splits and
both batch layouts; the sampled means agree with dtc_energy's trajectories.
"""
import os

import numpy as np
import pytest

from tests import sample_model as sm
from tests.helpers import implied_launch_counts, random_disorder

pytestmark = pytest.mark.gpu


def _check_traj(pkg, got, spec, inst, tid, seed, n_shots, row=None, t_first=0):
    """Row ``row`` (default ``tid``) of ``got`` is trajectory id ``tid``: all its
    samples, both bases, every t >= t_first; earlier rows are 0."""
    r = tid if row is None else row
    worst = 0.0
    for t, psi in sm.trajectory_states(spec, inst, tid, seed):
        if t < t_first:
            assert not got["z"][inst, r, t].any() and not got["x"][inst, r, t].any()
            continue
        p = t + spec.t_offset
        uz = pkg.engine.sample_draws(seed, tid, p, 0, n_shots)
        ux = pkg.engine.sample_draws(seed, tid, p, 1, n_shots)
        worst = max(worst, sm.check_outcomes(got["z"][inst, r, t], psi, uz, ("z", inst, tid, t)))
        if p == 0:
            # a basis state: X is floor(u 2^L), exactly
            want = np.floor(ux * 2.0 ** spec.L).astype(np.uint64)
            assert np.array_equal(got["x"][inst, r, t], want), (inst, tid, t)
        else:
            worst = max(worst, sm.check_outcomes(got["x"][inst, r, t], sm.hadamard_all(psi, spec.L),
                                                 ux, ("x", inst, tid, t)))
    print(f"L={spec.L} inst {inst} traj {tid}: largest excess over a boundary {worst:.3e}")


@pytest.mark.parametrize("L,T,p,pol,state", [
    (5, 6, 0.05, "x", "neel"),               # one group, seven padding sites
    (7, 5, 0.1, "circular_left", "vacuum"),  # general kicks, n_sub = 2
    (13, 5, 0.05, "xy", "neel"),             # two groups, the second a small one
    (14, 4, 0.05, "y", "vacuum"),            # two groups
])
def test_sample_matches_oracle(pkg, engine, L, T, p, pol, state):
    rng = np.random.default_rng(L + 500)
    hs, phis = random_disorder(rng, L, 2)
    spec = pkg.energy.energy_spec(L, T, hs, phis, 0.94, state, noise_prob=p, polarization=pol)
    got = engine.sample(spec, 3, n_shots=3, seed=21)
    assert set(got) == {"z", "x"}
    for b in "zx":
        assert got[b].shape == (2, 3, T, 3) and got[b].dtype == np.uint64
    for inst in range(2):
        for tr in range(3):
            _check_traj(pkg, got, spec, inst, tr, 21, 3)


def test_sample_L20_both_layouts(pkg, engine):
    """L = 20, RX: eight trajectories run in the octet layout, three contiguous;
    the shared trajectories' rows are bit-identical, and the oracle's."""
    rng = np.random.default_rng(2120)
    hs, phis = random_disorder(rng, 20, 1)
    spec = pkg.SweepSpec(L=20, T=4, hs=hs, phis=phis, g=0.97, noise_prob=0.05, polarization="x")
    a8 = engine.sample(spec, 8, n_shots=3, seed=33)
    a3 = engine.sample(spec, 3, n_shots=3, seed=33)
    for b in "zx":
        assert np.array_equal(a8[b][:, :3], a3[b]), b
    for tr in range(3):
        _check_traj(pkg, a3, spec, 0, tr, 33, 3)
    _check_traj(pkg, a8, spec, 0, 7, 33, 3)


@pytest.mark.parametrize("L,pol,state", [(9, "circular_left", "neel"), (14, "y", "vacuum")])
def test_sample_octet_layout(pkg, engine, L, pol, state):
    """One tile per state (L = 9) and 10 + 4 sites (L = 14): nine trajectories in
    one batch run in the octet layout (a full octet and a partial one), in
    batches of three contiguous; the rows are bit-identical, and trajectory 8
    (the partial octet's) is the oracle's."""
    rng = np.random.default_rng(L + 540)
    hs, phis = random_disorder(rng, L)
    spec = pkg.energy.energy_spec(L, 4, hs, phis, 0.94, state, noise_prob=0.1, polarization=pol)
    a9 = engine.sample(spec, 9, n_shots=3, seed=35, batch=0)
    a3 = engine.sample(spec, 9, n_shots=3, seed=35, batch=3)
    for b in "zx":
        assert np.array_equal(a9[b], a3[b]), b
    _check_traj(pkg, a9, spec, 0, 8, 35, 3)


@pytest.mark.parametrize("L,pol,state,T", [(21, "x", "neel", 4), (24, "y", "vacuum", 3)])
def test_sample_two_and_three_groups(pkg, engine, L, pol, state, T):
    """A further group split (21) and three groups (24): their basis-change passes."""
    rng = np.random.default_rng(L + 17)
    hs, phis = random_disorder(rng, L)
    spec = pkg.energy.energy_spec(L, T, hs, phis, 0.93, state, noise_prob=0.05, polarization=pol)
    got = engine.sample(spec, 1, n_shots=3, seed=5)
    _check_traj(pkg, got, spec, 0, 0, 5, 3)


def test_sample_t_offset_and_t_first(pkg, engine):
    rng = np.random.default_rng(31)
    L = 13
    hs, phis = random_disorder(rng, L)
    spec = pkg.SweepSpec(L=L, T=4, hs=hs, phis=phis, g=0.95, noise_prob=0.05, t_offset=1)
    got = engine.sample(spec, 3, n_shots=3, seed=9)
    for tr in range(3):
        _check_traj(pkg, got, spec, 0, tr, 9, 3)
    late = engine.sample(spec, 3, n_shots=3, seed=9, t_first=2)
    for b in "zx":
        assert not late[b][:, :, :2].any()
        assert np.array_equal(late[b][:, :, 2:], got[b][:, :, 2:])
    plain = pkg.SweepSpec(L=L, T=4, hs=hs, phis=phis, g=0.95, noise_prob=0.05)
    late = engine.sample(plain, 2, n_shots=3, seed=9, t_first=1, traj_offset=5)
    for tr in range(2):
        _check_traj(pkg, late, plain, 0, 5 + tr, 9, 3, row=tr, t_first=1)


def test_sample_single_basis(pkg, engine):
    rng = np.random.default_rng(32)
    hs, phis = random_disorder(rng, 7)
    spec = pkg.SweepSpec(L=7, T=4, hs=hs, phis=phis, g=0.95, noise_prob=0.05)
    both = engine.sample(spec, 4, n_shots=2, seed=4)
    z = engine.sample(spec, 4, n_shots=2, seed=4, bases="z")
    x = engine.sample(spec, 4, n_shots=2, seed=4, bases="x")
    assert set(z) == {"z"} and set(x) == {"x"}
    assert np.array_equal(z["z"], both["z"]) and np.array_equal(x["x"], both["x"])


@pytest.mark.parametrize("L,state", [(5, "neel"), (13, "vacuum"), (20, "vacuum")])
def test_sample_noiseless_initial_row(pkg, engine, L, state):
    rng = np.random.default_rng(55 + L)
    hs, phis = random_disorder(rng, L)
    spec = pkg.energy.energy_spec(L, 3, hs, phis, 0.95, state, noise_prob=0.0, use_noise=0)
    got = engine.sample(spec, 2, n_shots=4, seed=3)
    assert np.all(got["z"][:, :, 0] == np.uint64(spec.init_mask))
    for tr in range(2):
        ux = pkg.engine.sample_draws(3, tr, 0, 1, 4)
        assert np.array_equal(got["x"][0, tr, 0], np.floor(ux * 2.0 ** L).astype(np.uint64))


def test_sample_invariance(pkg, engine):
    rng = np.random.default_rng(41)
    L, n = 14, 24
    hs, phis = random_disorder(rng, L, 2)
    spec = pkg.SweepSpec(L=L, T=5, hs=hs, phis=phis, g=0.95, noise_prob=0.05)
    a = engine.sample(spec, n, n_shots=3, seed=8, batch=24)
    b = engine.sample(spec, n, n_shots=3, seed=8, batch=8)
    lo = engine.sample(spec, 12, n_shots=3, seed=8, traj_offset=0)
    hi = engine.sample(spec, 12, n_shots=3, seed=8, traj_offset=12)
    for key in "zx":
        assert np.array_equal(a[key], b[key]), key
        assert np.array_equal(a[key][:, :12], lo[key]), key
        assert np.array_equal(a[key][:, 12:], hi[key]), key


def test_sample_same_trajectories_as_energy(pkg, engine):
    """4096 trajectories, one shot each, fixed seed: the sampled means lie within
    5 standard errors sqrt((1 - m^2) / n) of dtc_energy's trajectory means m."""
    rng = np.random.default_rng(8)
    L, T, p, n = 4, 6, 0.1, 4096
    hs, phis = random_disorder(rng, L)
    spec = pkg.SweepSpec(L=L, T=T, hs=hs, phis=phis, g=0.97, noise_prob=p)
    bits = engine.sample(spec, n, n_shots=1, seed=3)
    obs = pkg.energy.observables_from_samples(bits["z"], bits["x"], L)
    ref = engine.energy(spec, n, seed=3)
    for key in ("z", "zz", "x"):
        m = ref[key][0].mean(axis=0)
        se = np.sqrt(np.clip(1.0 - m * m, 0.0, None) / n)
        dev = np.abs(obs[key][0] - m)
        print(f"{key}: max deviation {np.max(dev / (se + 1e-300)):.2f} standard errors")
        assert np.all(dev <= 5.0 * se + 1e-12), key


def test_sample_histogram(pkg, engine):
    """65536 shots of one noiseless L = 4 state, both bases: Pearson's chi^2
    against the oracle's |psi|^2 over the 16 outcomes (the seed meets the bound
    with dtc_sample_state on the host: tests/test_sample_cpu.py)."""
    h = sm.HIST
    spec, psi = sm.hist_state(pkg)
    got = engine.sample(spec, 1, n_shots=h["n_shots"], seed=h["seed"], t_first=h["t"])
    for basis, key in enumerate("zx"):
        ref = sm.hadamard_all(psi, h["L"]) if basis else psi
        prob = np.abs(ref) ** 2
        chi2 = sm.pearson_chi2(got[key][0, 0, h["t"]], prob / prob.sum())
        print(f"{key}: chi2 = {chi2:.2f}, bound {sm.chi2_bound(15):.2f}")
        assert chi2 <= sm.chi2_bound(15), key
        u = pkg.engine.sample_draws(h["seed"], 0, h["t"], basis, h["n_shots"])
        sm.check_outcomes(got[key][0, 0, h["t"]], ref, u, key)


def test_sample_profiling_books_reduce(pkg):
    """The sampling launches are booked under the reduce kind: two per sampled
    state and basis, the weights with 16 B per amplitude."""
    rng = np.random.default_rng(12)
    L, T, n = 13, 4, 2
    hs, phis = random_disorder(rng, L)
    spec = pkg.SweepSpec(L=L, T=T, hs=hs, phis=phis, g=0.95, noise_prob=0.05)
    with pkg.DtcEngine(0) as eng:
        eng.set_profiling(True)
        eng.sample(spec, n, n_shots=2, seed=1)
        st = eng.kernel_stats()[pkg._capi.KERNEL_REDUCE]
    assert st["launches"] == 2 * 2 * (T - 1)
    pick = n * 2 * (8.0 * 2 + 16.0 * 4096)
    assert st["bytes"] == pytest.approx(2 * (T - 1) * (16.0 * (1 << L) * n + pick))


def test_sample_launches_match_schedule_dump(pkg, tmp_path):
    """The engine streams exactly the launches that the schedule header builds
    (tools/schedule_check.cpp mode=sample, the same case on the CPU): passes by
    kind, and under the reduce kind the two sampling launches per (time, basis);
    three trajectories in one batch, both bases, four shots.  L = 14: two site
    groups."""
    rng = np.random.default_rng(62)
    L, T = 14, 3
    hs, phis = random_disorder(rng, L)
    spec = pkg.SweepSpec(L=L, T=T, hs=hs, phis=phis, g=0.95, noise_prob=0.05)
    want, n_times = implied_launch_counts(pkg, tmp_path, ["mode=sample", "L=%d" % L, "T=%d" % T],
                                          n_groups=2, x_basis=True, measured_x=False)
    assert n_times == T - 1
    want[pkg._capi.KERNEL_REDUCE] += 2 * 2 * n_times
    with pkg.DtcEngine(0) as eng:
        eng.set_profiling(True)
        eng.sample(spec, 3, n_shots=4, seed=1)
        st = eng.kernel_stats()
    assert {k: st[k]["launches"] for k in want} == want


def test_sample_cli(pkg, tmp_path):
    import pandas as pd

    dis = tmp_path / "dis"
    dis.mkdir()
    rng = np.random.default_rng(6)
    L, n = 5, 64
    hs, phis = random_disorder(rng, L)
    pd.DataFrame(hs).to_csv(dis / "hs_L5.csv", index=False)
    pd.DataFrame(phis).to_csv(dis / "phis_L5.csv", index=False)
    common = ["--L", "5", "--tf", "6", "--trajectories", str(n), "--disorder_folder", str(dis)]

    def run(out, extra):
        assert pkg.energy_cli.main(common + ["--out_dir", str(out)] + extra) == 0
        files = [os.path.join(r, f) for r, _, fs in os.walk(out) for f in fs]
        assert len(files) == 1
        return files[0]

    sampled = run(tmp_path / "sampled", ["--sampled", "1"])
    plain = run(tmp_path / "plain", [])
    zero = run(tmp_path / "zero", ["--sampled", "0"])
    assert os.path.basename(sampled) == os.path.basename(plain)[:-4] + "_sampled.csv"
    assert os.path.basename(os.path.dirname(sampled)) == os.path.basename(os.path.dirname(plain))
    with open(zero, "rb") as f0, open(plain, "rb") as f1:
        assert f0.read() == f1.read()
    ds, dp = pd.read_csv(sampled), pd.read_csv(plain)
    assert list(ds.columns) == list(dp.columns) and len(ds) == 6
    # t = 0 without noise: the vacuum's Z outcomes are exact (the plain run's Z
    # and ZZ part; its X part is 0), the X outcomes are floor(u 2^L)
    seed = pkg.energy_cli.build_parser().parse_args([]).seed
    xs = np.zeros(L)
    for tr in range(n):
        x = int(np.floor(pkg.engine.sample_draws(seed, tr, 0, 1, 1)[0] * 2.0 ** L))
        xs += [1.0 - 2.0 * ((x >> i) & 1) for i in range(L)]
    _, _, cx = pkg.energy.hamiltonian_coefficients(L, 0.97, hs[0], phis[0])
    want = dp["energy_p_0"][0] + float(xs / n @ cx) / L
    assert abs(ds["energy_p_0"][0] - want) < 1e-12
    assert np.all(np.isfinite(ds.values))
