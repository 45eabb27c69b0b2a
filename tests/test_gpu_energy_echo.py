"""dtc_energy_echo (HIP): <Z_i>, <Z_i Z_i+1>, <X_i> of every echo chain's final
state -- the forward state after p = t + t_offset periods taken through p
inverse periods, the state dtc_autocorr measures its echo on.

Per trajectory against the gate-by-gate oracle (tests/energy_echo_model.py) at
1e-10, the project's standing figure for engine against oracle; schedule
variants against each other at 1e-12; the trajectory mean against the exact
channel within 5 standard errors.
"""
import os

import numpy as np
import pytest

from tests import energy_echo_model as model
from tests.helpers import harsh_device, random_disorder

pytestmark = pytest.mark.gpu
TOL = 1e-10
KEYS = ("z", "zz", "x")


def _check(got, spec, inst, tr, seed, row=None, traj=None, t_first=0):
    """Row ``row`` of ``got`` (default ``tr``) is trajectory id ``traj`` (default ``tr``)."""
    ref = model.trajectory_energy_echo(spec, inst, tr if traj is None else traj, seed=seed,
                                       t_first=t_first)
    r = tr if row is None else row
    for key, want in zip(KEYS, ref):
        err = float(np.abs(got[key][inst, r] - want).max())
        print(f"L={spec.L} inst {inst} traj {tr if traj is None else traj} {key}: {err:.3e}")
        assert err < TOL, (key, inst, r, err)


@pytest.mark.parametrize("L,T,p,pol,state", [
    (5, 6, 0.05, "x", "neel"),              # one group; the chain is D-K finals
    (7, 5, 0.1, "circular_left", "vacuum"),  # general kicks, n_sub = 2
    (13, 5, 0.05, "xy", "neel"),            # two groups, the second a small one
    (14, 5, 0.05, "y", "vacuum"),           # RY, two groups
])
def test_energy_echo_matches_oracle(pkg, engine, L, T, p, pol, state):
    rng = np.random.default_rng(L + 300)
    hs, phis = random_disorder(rng, L, 2)
    spec = pkg.energy.energy_spec(L, T, hs, phis, 0.94, state, noise_prob=p, polarization=pol)
    got = engine.energy_echo(spec, 3, seed=21)
    for inst in range(2):
        for tr in range(3):
            _check(got, spec, inst, tr, 21)


@pytest.mark.parametrize("L,pol,state,T,n", [(21, "x", "neel", 4, 2), (24, "y", "vacuum", 3, 1)])
def test_energy_echo_two_and_three_groups(pkg, engine, L, pol, state, T, n):
    rng = np.random.default_rng(L + 17)
    hs, phis = random_disorder(rng, L)
    spec = pkg.energy.energy_spec(L, T, hs, phis, 0.93, state, noise_prob=0.05, polarization=pol)
    got = engine.energy_echo(spec, n, seed=5)
    for tr in range(n):
        _check(got, spec, 0, tr, 5)


def test_energy_echo_octet_layout_matches_oracle(pkg, engine):
    """L = 17 (9 + 8 sites, RY), nine trajectories: one batch runs the octet
    layout (a full octet and a partial one), batches of one contiguous states;
    the rows are the same bits, and the oracle's for the trajectories 7 and 8
    on either side of the octet's edge."""
    rng = np.random.default_rng(317)
    L = 17
    hs, phis = random_disorder(rng, L)
    spec = pkg.energy.energy_spec(L, 4, hs, phis, 0.94, "neel", noise_prob=0.1, polarization="y")
    got = engine.energy_echo(spec, 9, seed=27, batch=0)
    one = engine.energy_echo(spec, 9, seed=27, batch=1)
    for key in KEYS:
        assert np.array_equal(got[key], one[key]), (key, float(np.abs(got[key] - one[key]).max()))
    for tr in (7, 8):
        _check(got, spec, 0, tr, 27)


def _fresh(pkg, monkeypatch, spec, n, env=None, **kw):
    """One energy_echo call on a fresh engine opened with ``env`` set."""
    with monkeypatch.context() as m:
        for k in ("DTC_WAVEFRONT", "DTC_NO_WAVEFRONT", "DTC_NO_DUAL", "DTC_NO_LIGHTCONE"):
            m.delenv(k, raising=False)
        if env:
            m.setenv(env, "1")
        with pkg.DtcEngine(0) as eng:
            eng.set_profiling(True)
            out = eng.energy_echo(spec, n, **kw)
            info = {"stats": eng.kernel_stats(), "wf": eng.wavefront_count(),
                    "sched": eng.schedule_counts(), "lc": eng.lightcone_counts()}
            eng.release_buffers()
    return out, info


@pytest.mark.parametrize("n,off,ids", [(8, 0, (0, 7)), (16, 1016, (1023, 1024))])
def test_energy_echo_c2_shape(pkg, monkeypatch, n, off, ids):
    """L = 20, RX, p = 0.05, the octet layout: the dual-pass start and the
    wavefront interior run, every chain ends in one measure-only pass, and the
    plain schedules give the same rows."""
    rng = np.random.default_rng(2020)
    hs, phis = random_disorder(rng, 20, 1)
    T, t_first = 8, 6
    spec = pkg.SweepSpec(L=20, T=T, hs=hs, phis=phis, g=0.97, noise_prob=0.05)
    kw = dict(seed=91, traj_offset=off, t_first=t_first)
    got, info = _fresh(pkg, monkeypatch, spec, n, **kw)
    for tid in ids:
        _check(got, spec, 0, tid, 91, row=tid - off, traj=tid, t_first=t_first)
    for key in KEYS:
        assert not got[key][:, :, :t_first].any()
    assert info["wf"] > 0
    assert info["sched"]["folded"] > 0
    assert not any(info["lc"].values())
    final = info["stats"][pkg._capi.KERNEL_FINAL_PASS]
    chains = T - t_first
    assert final["launches"] == chains
    assert final["bytes"] == pytest.approx(chains * 16.0 * (1 << 20) * n)
    for env in ("DTC_NO_WAVEFRONT", "DTC_NO_DUAL"):
        other, oinfo = _fresh(pkg, monkeypatch, spec, n, env=env, **kw)
        for key in KEYS:
            err = float(np.abs(other[key] - got[key]).max())
            print(f"{env} {key}: {err:.3e}")
            assert err < 1e-12, (env, key, err)
        if env == "DTC_NO_WAVEFRONT":
            assert oinfo["wf"] == 0
        else:
            assert oinfo["sched"]["folded"] == 0


def _c2_wavefront_and_plain(pkg, monkeypatch, spec, n, t_first, seed, states):
    """An L = 20 call in the octet layout whose chains run the wavefront interior:
    the oracle's rows for ``states`` ((inst, trajectory) pairs), nothing before
    ``t_first``, one measure-only end per chain, and the plain interior's rows
    (DTC_NO_WAVEFRONT=1) within 1e-12.  Returns the rows."""
    kw = dict(seed=seed, t_first=t_first)
    got, info = _fresh(pkg, monkeypatch, spec, n, **kw)
    for inst, tr in states:
        _check(got, spec, inst, tr, seed, t_first=t_first)
    for key in KEYS:
        assert got[key].shape[:3] == (spec.n_inst, n, spec.T)
        assert not got[key][:, :, :t_first].any()
        assert got[key][:, :, t_first:].any()
    assert info["wf"] > 0
    assert not any(info["lc"].values())
    assert info["stats"][pkg._capi.KERNEL_FINAL_PASS]["launches"] == spec.T - t_first
    other, oinfo = _fresh(pkg, monkeypatch, spec, n, env="DTC_NO_WAVEFRONT", **kw)
    assert oinfo["wf"] == 0
    for key in KEYS:
        err = float(np.abs(other[key] - got[key]).max())
        print(f"DTC_NO_WAVEFRONT {key}: {err:.3e}")
        assert err < 1e-12, (key, err)
    return got


def test_energy_echo_c2_shape_two_instances(pkg, monkeypatch):
    """test_energy_echo_c2_shape's sweep with two disorder instances of six
    trajectories: twelve states, an octet that holds instance 0 and the first two
    states of instance 1, and a partial octet.  The wavefront pass reads its
    diagonal tables per instance ((batch_start + b) / n_traj): the oracle's rows
    for (instance 0, trajectory 5) and (instance 1, trajectory 0), the states on
    either side of the instance edge, which share an octet."""
    rng = np.random.default_rng(2021)
    hs, phis = random_disorder(rng, 20, 2)
    spec = pkg.SweepSpec(L=20, T=8, hs=hs, phis=phis, g=0.97, noise_prob=0.05)
    got = _c2_wavefront_and_plain(pkg, monkeypatch, spec, 6, 6, 92, [(0, 5), (1, 0)])
    # the same trajectory ids under the two instances' angles: other rows
    for key in KEYS:
        assert np.abs(got[key][0, :, 6:] - got[key][1, :, 6:]).max() > 1e-3, key


def test_energy_echo_c2_shape_ry_neel(pkg, monkeypatch):
    """The RY twin of test_energy_echo_c2_shape's one-octet case: RY kicks from
    the Neel state (the wavefront pass's real kicks, tile 1's trailing kick-less
    diagonal among its passes); the oracle's rows for the trajectories 0 and 7."""
    rng = np.random.default_rng(2022)
    hs, phis = random_disorder(rng, 20, 1)
    spec = pkg.SweepSpec(L=20, T=8, hs=hs, phis=phis, g=0.93, noise_prob=0.05,
                         polarization="y", initial_state="neel")
    _c2_wavefront_and_plain(pkg, monkeypatch, spec, 8, 6, 93, [(0, 0), (0, 7)])


@pytest.mark.parametrize("L,n", [(20, 3), (21, 8)])
def test_energy_echo_fallback(pkg, monkeypatch, L, n):
    """No octet layout (3 states) or L = 21: the plain interior, the oracle's rows."""
    rng = np.random.default_rng(2030 + L)
    hs, phis = random_disorder(rng, L, 1)
    T, t_first = 7, 5
    spec = pkg.SweepSpec(L=L, T=T, hs=hs, phis=phis, g=0.97, noise_prob=0.05)
    got, info = _fresh(pkg, monkeypatch, spec, n, seed=94, t_first=t_first)
    assert info["wf"] == 0
    for tr in (0, n - 1):
        _check(got, spec, 0, tr, 94, t_first=t_first)


@pytest.mark.parametrize("L", [14, 20])
def test_energy_echo_against_autocorr_echo(pkg, engine, L):
    """The existing echo autocorrelator is (1 - p)^6 z_j(init) <Z_j> of the same state."""
    rng = np.random.default_rng(77 + L)
    hs, phis = random_disorder(rng, L, 2 if L == 14 else 1)
    p, T, n = 0.05, 6, 8
    spec = pkg.SweepSpec(L=L, T=T, hs=hs, phis=phis, g=0.96, noise_prob=p, initial_state="neel")
    ee = engine.energy_echo(spec, n, seed=12)
    ac = engine.autocorr(spec, n, seed=12, want_fwd=False)["echo"]
    j = L // 2
    zinit = np.sign(ee["z"][:, :, 0, j])
    want = (1 - p) ** 6 * zinit[:, :, None] * ee["z"][:, :, :, j]
    err = float(np.abs(ac - want).max())
    print(f"L={L}: {err:.3e}")
    assert err < 1e-12


@pytest.mark.parametrize("L", [5, 13, 20])
def test_energy_echo_noiseless_is_initial_state(pkg, engine, L):
    rng = np.random.default_rng(55 + L)
    hs, phis = random_disorder(rng, L)
    state = "neel" if L % 2 else "vacuum"
    spec = pkg.energy.energy_spec(L, 6, hs, phis, 0.95, state, noise_prob=0.0, use_noise=0)
    got = engine.energy_echo(spec, 1, seed=3)
    m = spec.init_mask
    z0 = np.array([-1.0 if (m >> i) & 1 else 1.0 for i in range(L)])
    assert np.array_equal(got["z"][0, 0, 0], z0)
    for t in range(6):
        assert np.abs(got["z"][0, 0, t] - z0).max() < 1e-12
        assert np.abs(got["zz"][0, 0, t] - z0[:-1] * z0[1:]).max() < 1e-12
        assert np.abs(got["x"][0, 0, t]).max() < 1e-12


def test_energy_echo_t_offset(pkg, engine):
    """t_offset = 1: the echo streams are 1 + t, so the rows are not a shift of
    the t_offset = 0 run's: compared through the oracle."""
    rng = np.random.default_rng(31)
    L = 13
    hs, phis = random_disorder(rng, L)
    spec = pkg.SweepSpec(L=L, T=4, hs=hs, phis=phis, g=0.95, noise_prob=0.05, t_offset=1)
    got = engine.energy_echo(spec, 3, seed=9)
    for tr in range(3):
        _check(got, spec, 0, tr, 9)


def test_energy_echo_invariance(pkg, engine):
    rng = np.random.default_rng(41)
    L, n = 14, 24
    hs, phis = random_disorder(rng, L, 2)
    spec = pkg.SweepSpec(L=L, T=5, hs=hs, phis=phis, g=0.95, noise_prob=0.05)
    a = engine.energy_echo(spec, n, seed=8, batch=24)
    b = engine.energy_echo(spec, n, seed=8, batch=8)
    lo = engine.energy_echo(spec, 12, seed=8, traj_offset=0)
    hi = engine.energy_echo(spec, 12, seed=8, traj_offset=12)
    sums = engine.energy_echo_sums(spec, n, seed=8, batch=8)
    for key in KEYS:
        assert np.array_equal(a[key], b[key]), key
        assert np.array_equal(a[key][:, :12], lo[key]), key
        assert np.array_equal(a[key][:, 12:], hi[key]), key
        assert sums[key].shape == a[key].sum(axis=1).shape
        np.testing.assert_allclose(sums[key], a[key].sum(axis=1), rtol=1e-12, atol=1e-12 * n)


def test_energy_echo_mean_vs_exact_channel(pkg, engine):
    """4096 trajectories, fixed seed: every mean within 5 standard errors of the
    exact channel's value (the density-matrix oracle's periods and inverses)."""
    rng = np.random.default_rng(8)
    L, T, p, n = 4, 6, 0.1, 4096
    hs, phis = random_disorder(rng, L)
    spec = pkg.SweepSpec(L=L, T=T, hs=hs, phis=phis, g=0.97, noise_prob=p)
    got = engine.energy_echo(spec, n, seed=3)
    exact = model.exact_energy_echo(L, T, hs[0], phis[0], spec.kick, p)
    for k, key in enumerate(KEYS):
        v = got[key][0]
        mean, sd = v.mean(axis=0), v.std(axis=0) / np.sqrt(n) + 1e-12
        dev = np.abs(mean - exact[k]) / sd
        print(f"{key}: max deviation {dev.max():.2f} standard errors")
        assert np.all(dev < 5), key


def test_energy_echo_refusals(pkg, engine):
    rng = np.random.default_rng(5)
    L = 5
    hs, phis = random_disorder(rng, L)
    dev = pkg.SweepSpec(L=L, T=4, hs=hs, phis=phis, device=harsh_device(pkg, L))
    bond = pkg.SweepSpec(L=L, T=4, hs=hs, phis=phis, bond_noise=0.02)
    for spec, word in ((dev, "device-like noise"), (bond, "bond noise")):
        for call in (lambda s: engine.energy_echo(s, 2), lambda s: engine.energy_echo_sums(s, 2),
                     lambda s: pkg.energy.get_instances_energy(s, 2, engine=engine, echo=True)):
            with pytest.raises(NotImplementedError, match=word):
                call(spec)


def test_energy_echo_cli(pkg, tmp_path):
    import pandas as pd

    dis = tmp_path / "dis"
    dis.mkdir()
    rng = np.random.default_rng(6)
    hs, phis = random_disorder(rng, 5)
    pd.DataFrame(hs).to_csv(dis / "hs_L5.csv", index=False)
    pd.DataFrame(phis).to_csv(dis / "phis_L5.csv", index=False)
    common = ["--L", "5", "--tf", "6", "--trajectories", "64", "--disorder_folder", str(dis)]

    def run(out, extra):
        assert pkg.energy_cli.main(common + ["--out_dir", str(out)] + extra) == 0
        files = [os.path.join(r, f) for r, _, fs in os.walk(out) for f in fs]
        assert len(files) == 1
        return files[0]

    echo = run(tmp_path / "echo", ["--echo", "1"])
    plain = run(tmp_path / "plain", [])
    zero = run(tmp_path / "zero", ["--echo", "0"])
    assert echo.endswith("_echo.csv") and not plain.endswith("_echo.csv")
    assert os.path.basename(echo) == os.path.basename(plain)[:-4] + "_echo.csv"
    assert os.path.basename(os.path.dirname(echo)) == os.path.basename(os.path.dirname(plain))
    assert os.path.basename(zero) == os.path.basename(plain)
    with open(zero, "rb") as f0, open(plain, "rb") as f1:
        assert f0.read() == f1.read()
    de, dp = pd.read_csv(echo), pd.read_csv(plain)
    assert list(de.columns) == list(dp.columns) and len(de) == 6
    # without noise the echo is the initial state's energy at every t
    assert np.abs(de["energy_p_0"] - de["energy_p_0"][0]).max() < 1e-12
    assert abs(de["energy_p_0"][0] - dp["energy_p_0"][0]) < 1e-12
    for extra in (["--use_fakebackend", "1"], ["--bond_noise_prob", "0.01"]):
        with pytest.raises(SystemExit, match="does not support"):
            pkg.energy_cli.main(common + ["--out_dir", str(tmp_path / "no"), "--echo", "1"] + extra)
