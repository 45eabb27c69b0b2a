"""Bond noise with device-like kick noise (dtc_autocorr_bond with dv) and in the
energy path (dtc_energy_bond, dtc_energy_sums_bond) on the MI355X:
per-trajectory parity with the literal gate-by-gate model of
tests/bond_device_model.py (validated against the C oracle on the CPU by
tests/test_bond_device_cpu.py), the unchanged kick draws, the on-device sums,
the trajectory means against the exact channel, batch / split invariance, the
facade and the command lines.
"""
import ctypes
import os

import numpy as np
import pytest

from tests import bond_device_model as bdm
from tests import bond_model as bm
from tests.helpers import random_disorder
from tests.test_bond_device_cpu import EXACT, exact_spec, harsh_device

pytestmark = pytest.mark.gpu
P_BOND = 0.4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _draws(pkg, spec, seed, traj, p_bond=P_BOND):
    return bdm.Draws(pkg, spec.L, spec.n_sub, seed, traj, p=spec.p, device=spec.device,
                     p_bond=p_bond)


def _autocorr_ref(pkg, spec, n_traj, seed, p_bond=P_BOND):
    dev = spec.device
    fac = dev.anc_factor if dev is not None else (1.0 - spec.p) ** pkg.N_ANCILLA_NOISY_GATES
    ro = ((1.0 - dev.readout_p01 - dev.readout_p10, dev.readout_p10 - dev.readout_p01)
          if dev is not None else (1.0, 0.0))
    ref = {"fwd": np.zeros((spec.n_inst, n_traj, spec.T)),
           "echo": np.zeros((spec.n_inst, n_traj, spec.T)),
           "zsite": np.zeros((spec.n_inst, n_traj, spec.T, spec.L))}
    for i in range(spec.n_inst):
        for r in range(n_traj):
            f, e, z = bdm.literal_autocorr(spec.L, spec.T, spec.hs[i], spec.phis[i], spec.kick,
                                           spec.init_mask, spec.probe_site,
                                           _draws(pkg, spec, seed, r, p_bond), fac, ro)
            ref["fwd"][i, r], ref["echo"][i, r], ref["zsite"][i, r] = f, e, z
    return ref


def _autocorr_coverage(pkg, spec, n_traj, seed):
    """Which rules the seed's draws exercise (dtc_kick_draws, dtc_bond_draws)."""
    L, T = spec.L, spec.T
    got = dict(jump=False, probe_x=False, odd_fwd=False, even_inv=False)
    for r in range(n_traj):
        d = _draws(pkg, spec, seed, r)
        for t in range(1, T):
            codes = d.bond(0, t)
            got["jump"] |= bool(d.kick(0, t)[1].any())
            got["probe_x"] |= bool(bm.outgoing_x(L, codes)[spec.probe_site] == 1)
            got["odd_fwd"] |= bool(np.any(bm.flip_signs(L, codes, False)[1][1::2] < 0))
            for k in range(1, t + 1):
                got["jump"] |= bool(d.kick(1 + t, k)[1].any())
                got["even_inv"] |= bool(
                    np.any(bm.flip_signs(L, d.bond(1 + t, k), True)[1][0::2] < 0))
    return got


# (L, T, n_inst, n_traj, batch, polarization, seed); the seeds were checked on
# the CPU to exercise every rule (asserted below)
AUTOCORR_CASES = [
    pytest.param(5, 4, 1, 9, 0, "x", 11, id="L5-padded-tile"),
    pytest.param(14, 4, 2, 9, 8, "x", 11, id="L14-two-groups-octets"),
    pytest.param(14, 4, 2, 9, 8, "xy", 11, id="L14-xy-general-kicks"),
    pytest.param(20, 3, 1, 2, 0, "x", 11, id="L20-12+8"),
]


@pytest.mark.parametrize("L,T,n_inst,n_traj,batch,pol,seed", AUTOCORR_CASES)
def test_autocorr_device_bond_matches_literal_model(pkg, engine, L, T, n_inst, n_traj, batch, pol,
                                                    seed):
    rng = np.random.default_rng(2000 + L)
    hs, phis = random_disorder(rng, L, n_inst)
    spec = pkg.SweepSpec(L=L, T=T, hs=hs, phis=phis, g=0.94, polarization=pol,
                         initial_state="neel", device=harsh_device(pkg, L), bond_noise=P_BOND)
    cov = _autocorr_coverage(pkg, spec, n_traj, seed)
    assert all(cov.values()), cov
    before = engine.schedule_counts()
    got = engine.autocorr(spec, n_traj, seed=seed, want_zsite=True, batch=batch)
    after = engine.schedule_counts()
    assert after["device_kd"] > before["device_kd"]
    assert after["folded"] == before["folded"]
    assert after["device_runahead"] == before["device_runahead"]
    ref = _autocorr_ref(pkg, spec, n_traj, seed)
    for k in ("fwd", "echo", "zsite"):
        err = float(np.abs(got[k] - ref[k]).max())
        print(f"{k}: max |engine - literal| = {err:.3e}")
        assert err < 1e-10, (k, err)


def test_device_kick_draws_unchanged(pkg, engine):
    L, T, n_traj, seed = 14, 4, 9, 5
    rng = np.random.default_rng(7)
    hs, phis = random_disorder(rng, L, 2)
    base = dict(L=L, T=T, hs=hs, phis=phis, g=0.97, initial_state="neel",
                device=harsh_device(pkg, L))
    spec = pkg.SweepSpec(**base)
    plain = engine.autocorr(spec, n_traj, seed=seed, want_zsite=True, batch=8)
    # a non-null p_bond of zeros, with dv, through dtc_autocorr_bond itself
    pr = engine._problem(spec, True, True, 8, 0)
    dv = pkg._capi.device_struct(spec.device)
    bd = pkg.engine.bond_struct(np.zeros(L - 1))
    out = {k: np.zeros_like(v) for k, v in plain.items()}
    pkg._capi.check(engine._lib.dtc_autocorr_bond(
        engine._ctx, ctypes.byref(pr), None, ctypes.byref(dv), ctypes.byref(bd),
        ctypes.c_uint64(seed), ctypes.c_int64(0), ctypes.c_int32(n_traj),
        pkg._capi.as_dptr(out["fwd"]), pkg._capi.as_dptr(out["echo"]),
        pkg._capi.as_dptr(out["zsite"])))
    for k in plain:
        assert np.abs(out[k] - plain[k]).max() <= 1e-13, k
    # one noisy bond: a trajectory whose bond draws are all II is the plain device row
    pb = np.zeros(L - 1)
    pb[3] = 0.1
    noisy = engine.autocorr(pkg.SweepSpec(**base, bond_noise=pb), n_traj, seed=seed,
                            want_zsite=True, batch=8)
    layers = [(0, t) for t in range(1, T)] + [(1 + t, k) for t in range(1, T)
                                              for k in range(1, t + 1)]
    quiet = [r for r in range(n_traj)
             if not any(pkg.engine.bond_draws(pb, L, seed, r, s, c).any() for s, c in layers)]
    assert 3 <= len(quiet) < n_traj
    for k in plain:
        assert np.abs(noisy[k][:, quiet] - plain[k][:, quiet]).max() <= 1e-13, k
    assert np.abs(noisy["echo"] - plain["echo"]).max() > 1e-6


# ---- energy ---------------------------------------------------------------------------
def _energy_spec(pkg, L, T, pol, device, n_inst=1, toff=0, bond=P_BOND, seed=0):
    rng = np.random.default_rng(3000 + L + seed)
    hs, phis = random_disorder(rng, L, n_inst)
    kw = dict(device=harsh_device(pkg, L)) if device else dict(noise_prob=0.05)
    return pkg.SweepSpec(L=L, T=T, hs=hs, phis=phis, g=0.93, polarization=pol,
                         initial_state="neel", t_offset=toff, bond_noise=bond, **kw)


def _energy_coverage(pkg, spec, n_traj, seed):
    """A site whose outgoing Pauli is Z only and one where it is Y: the X rule
    and the Z rule then act apart and together."""
    got = dict(z_only=False, y=False)
    for r in range(n_traj):
        d = _draws(pkg, spec, seed, r)
        for s in range(1, spec.T + spec.t_offset):
            codes = d.bond(0, s)
            ox, oz = bm.outgoing_x(spec.L, codes), bdm.outgoing_z(spec.L, codes)
            got["z_only"] |= bool(np.any((oz == 1) & (ox == 0)))
            got["y"] |= bool(np.any((oz == 1) & (ox == 1)))
    return got


ENERGY_CASES = [
    pytest.param(5, 4, 3, "x", False, 0, 11, id="depol-L5"),
    pytest.param(14, 3, 3, "xy", False, 0, 11, id="depol-L14-xy"),
    pytest.param(20, 3, 2, "x", False, 0, 11, id="depol-L20"),
    pytest.param(5, 4, 3, "x", True, 1, 11, id="device-L5-toffset1"),
    pytest.param(13, 3, 3, "x", True, 0, 11, id="device-L13"),
    pytest.param(20, 3, 2, "x", True, 0, 11, id="device-L20"),
]


@pytest.mark.parametrize("L,T,n_traj,pol,device,toff,seed", ENERGY_CASES)
def test_energy_bond_matches_literal_model(pkg, engine, L, T, n_traj, pol, device, toff, seed):
    spec = _energy_spec(pkg, L, T, pol, device, toff=toff)
    cov = _energy_coverage(pkg, spec, n_traj, seed)
    assert all(cov.values()), cov
    got = engine.energy_bond(spec, n_traj, seed=seed)
    worst = 0.0
    for r in range(n_traj):
        ref = bdm.literal_energy(L, T, spec.hs[0], spec.phis[0], spec.kick, spec.init_mask,
                                 _draws(pkg, spec, seed, r), t_offset=toff)
        for key, v in zip(("z", "zz", "x"), ref):
            err = float(np.abs(got[key][0, r] - v).max())
            worst = max(worst, err)
            assert err < 1e-10, (key, r, err)
    print(f"max |engine - literal| = {worst:.3e}")
    # the signs matter: the rows differ from those of the run without bond noise
    plain = engine.energy(_energy_spec(pkg, L, T, pol, device, toff=toff, bond=None), n_traj,
                          seed=seed)
    assert max(np.abs(got[k] - plain[k]).max() for k in ("z", "zz", "x")) > 1e-3
    # and no bond noise in the spec gives exactly the plain rows
    same = engine.energy_bond(_energy_spec(pkg, L, T, pol, device, toff=toff, bond=None), n_traj,
                              seed=seed)
    for k in ("z", "zz", "x"):
        assert np.array_equal(same[k], plain[k]), k


@pytest.mark.parametrize("device", [False, True], ids=["depol", "device"])
@pytest.mark.parametrize("L,T,n_inst,n_traj,batch", [
    (14, 3, 3, 5, 4),     # batches that split instances
    (20, 3, 1, 24, 16),   # octet layout
])
def test_energy_sums_bond_match_rows(pkg, engine, L, T, n_inst, n_traj, batch, device):
    spec = _energy_spec(pkg, L, T, "x", device, n_inst=n_inst)
    rows = engine.energy_bond(spec, n_traj, seed=44, traj_offset=3)
    sums = engine.energy_sums_bond(spec, n_traj, seed=44, traj_offset=3, batch=batch)
    for key in ("z", "zz", "x"):
        ref = rows[key].sum(axis=1)
        assert sums[key].shape == ref.shape
        err = float(np.abs(sums[key] - ref).max())
        assert err < 1e-12 * n_traj, (key, err)
    e = pkg.energy.get_instances_energy(spec, n_traj, seed=44, engine=engine, traj_offset=3)
    means = {k: v.mean(axis=1) for k, v in rows.items()}
    ref_e = np.stack([pkg.energy.energy_from_observables({k: v[i] for k, v in means.items()}, L,
                                                         0.93, spec.hs[i], spec.phis[i], "full")
                      for i in range(n_inst)])
    assert np.abs(e["full"] - ref_e).max() < 1e-11


# ---- trajectory means against the exact channel ---------------------------------------
def _check_means(rows, exact, exact_without, what):
    """|mean - exact| / standard error < 4.5 per point, and the exact curve
    without bond noise further than twice the largest standard error away."""
    n = rows.shape[0]
    se = rows.std(axis=0, ddof=1) / np.sqrt(n) + 1e-12
    z = (rows.mean(axis=0) - exact) / se
    print(f"{what}: max |z| = {np.abs(z).max():.2f}, max se = {se.max():.2e}, "
          f"bond shift = {np.abs(exact - exact_without).max():.2e}")
    assert np.abs(z).max() < 4.5, (what, z)
    assert np.abs(exact - exact_without).max() > 2 * se.max(), what


def test_autocorr_device_bond_means_match_exact_channel(pkg, engine):
    spec = exact_spec(pkg, "device")
    N, pb = 8192, EXACT["p_bond"]
    args = (spec.L, spec.T, spec.hs[0], spec.phis[0], spec.kick)
    kw = dict(device=spec.device, init_mask=spec.init_mask, probe=spec.probe_site)
    f1, e1 = bdm.exact_autocorr(*args, pb, **kw)
    f0, e0 = bdm.exact_autocorr(*args, 0.0, **kw)
    got = engine.autocorr(spec, N, seed=EXACT["seed"])
    _check_means(got["fwd"][0], f1, f0, "fwd")
    _check_means(got["echo"][0], e1, e0, "echo")


@pytest.mark.parametrize("noise", ["depol", "device"])
def test_energy_bond_means_match_exact_channel(pkg, engine, noise):
    spec = exact_spec(pkg, noise, energy=True)
    N, pb = 8192, EXACT["p_bond"]
    args = (spec.L, spec.T, spec.hs[0], spec.phis[0], spec.kick)
    kw = dict(p=spec.p, device=spec.device, init_mask=spec.init_mask)
    ex1 = bdm.exact_energy(*args, pb, **kw)
    ex0 = bdm.exact_energy(*args, 0.0, **kw)
    got = engine.energy_bond(spec, N, seed=EXACT["seed"])
    rows = np.concatenate([got[k][0] for k in ("z", "zz", "x")], axis=2)
    _check_means(rows, np.concatenate(ex1, axis=1), np.concatenate(ex0, axis=1), "z | zz | x")
    sums = engine.energy_sums_bond(spec, N, seed=EXACT["seed"])
    for k in ("z", "zz", "x"):
        assert np.abs(sums[k][0] / N - got[k][0].mean(axis=0)).max() < 1e-12


# ---- rows independent of batching and splits -------------------------------------------
def test_rows_invariant_under_batch_and_split(pkg, engine):
    L, T = 14, 4
    rng = np.random.default_rng(9)
    hs, phis = random_disorder(rng, L, 2)
    spec = pkg.SweepSpec(L=L, T=T, hs=hs, phis=phis, g=0.97, initial_state="neel",
                         device=harsh_device(pkg, L), bond_noise=0.2)
    kw = dict(seed=77, want_zsite=True)
    a = engine.autocorr(spec, 16, batch=0, **kw)
    b = engine.autocorr(spec, 16, batch=8, **kw)
    lo = engine.autocorr(spec, 8, traj_offset=0, batch=0, **kw)
    hi = engine.autocorr(spec, 8, traj_offset=8, batch=0, **kw)
    for k in ("fwd", "echo", "zsite"):
        assert np.array_equal(a[k], b[k]), k
        assert np.array_equal(a[k], np.concatenate([lo[k], hi[k]], axis=1)), k
    for device in (False, True):
        es = _energy_spec(pkg, L, T, "x", device, n_inst=2, bond=0.2)
        a = engine.energy_bond(es, 16, seed=77, batch=0)
        b = engine.energy_bond(es, 16, seed=77, batch=8)
        lo = engine.energy_bond(es, 8, seed=77, traj_offset=0)
        hi = engine.energy_bond(es, 8, seed=77, traj_offset=8)
        for k in ("z", "zz", "x"):
            assert np.array_equal(a[k], b[k]), (device, k)
            assert np.array_equal(a[k], np.concatenate([lo[k], hi[k]], axis=1)), (device, k)


# ---- facade and command lines ----------------------------------------------------------
CAL = os.path.join(ROOT, "data", "device_standin_L20.json")


def test_facade_calibration_with_rzz_error(pkg, engine):
    aer = pkg.aer
    L, n_fwd, pb, shots, seed = 4, 3, 0.1, 512, 4242
    rng = np.random.default_rng(33)
    hs, phis = random_disorder(rng, L)
    backend = aer.FakeDevice(CAL)
    nm = pkg.NoiseModel.from_backend(backend)
    nm.add_all_qubit_quantum_error(aer.depolarizing_error(pb, 2), ["rzz"])
    spec = pkg.SweepSpec(L=L, T=n_fwd + 1, hs=hs, phis=phis, g=0.97,
                         device=backend.calibration.device_noise(L), bond_noise=pb)
    plain = pkg.SweepSpec(L=L, T=n_fwd + 1, hs=hs, phis=phis, g=0.97,
                          device=backend.calibration.device_noise(L))
    for echo in (False, True):
        circ = pkg.circuit.dtc_circuit(
            L, n_fwd, spec.hs[0], spec.phis[0],
            lambda step: pkg.kicks.period_gate_specs("x", 0.97, step), echo=echo)
        res = aer.DtcSimulator(noise_model=nm).run(circ, shots=shots, seed_simulator=seed).result()
        key = "echo" if echo else "fwd"
        out = engine.autocorr(spec, shots, seed=seed, want_fwd=not echo, want_echo=echo,
                              t_first=n_fwd)
        want = float(out[key][0, :, n_fwd].mean())
        assert abs(res.expectations[0] - want) < 1e-12, (echo, res.expectations[0], want)
        base = engine.autocorr(plain, shots, seed=seed, want_fwd=not echo, want_echo=echo,
                               t_first=n_fwd)
        assert abs(want - float(base[key][0, :, n_fwd].mean())) > 1e-3


def _disorder_dir(golden, tmp_path):
    import pandas as pd

    d = golden["disorder"]["L4"]
    dis = tmp_path / "dis"
    dis.mkdir()
    pd.DataFrame(d["hs"]).to_csv(dis / "hs_L4.csv", index=False)
    pd.DataFrame(d["phis"]).to_csv(dis / "phis_L4.csv", index=False)
    return dis


def _files(root):
    return sorted(os.path.relpath(os.path.join(r, f), root)
                  for r, _, fs in os.walk(root) for f in fs)


def test_cli_fakebackend_bond(pkg, golden, tmp_path):
    import pandas as pd

    dis = _disorder_dir(golden, tmp_path)
    common = ["--L", "4", "--tf", "5", "--use_fakebackend", "1", "--shots", "0",
              "--trajectories", "64", "--disorder_folder", str(dis)]
    outs = {}
    for tag, extra in (("none", []), ("zero", ["--fakebackend_bond", "0"]),
                       ("bond", ["--fakebackend_bond", "1"])):
        out = tmp_path / tag
        assert pkg.cli.main(common + extra + ["--out_dir", str(out)]) == 0
        outs[tag] = out
    # the flag at 0: the same files, byte for byte
    assert _files(outs["none"]) == _files(outs["zero"]) and len(_files(outs["none"])) == 1
    for f in _files(outs["none"]):
        assert open(outs["none"] / f, "rb").read() == open(outs["zero"] / f, "rb").read()
    (plain,) = _files(outs["none"])
    (bond,) = _files(outs["bond"])
    assert bond == plain[:-4] + "_bondcal.csv"
    a, b = pd.read_csv(outs["none"] / plain), pd.read_csv(outs["bond"] / bond)
    assert list(a.columns) == list(b.columns) and len(b) == 5
    assert a["av_autocorr"][0] == b["av_autocorr"][0]       # t = 0: no RZZ yet
    assert np.abs(a["av_autocorr_echo"] - b["av_autocorr_echo"]).max() > 1e-4
    # --bond_noise_prob now combines with the device-like noise
    out = tmp_path / "prob"
    assert pkg.cli.main(common + ["--bond_noise_prob", "0.05", "--out_dir", str(out)]) == 0
    assert _files(out) == [plain[:-4] + "_bond0.05.csv"]


def test_energy_cli_fakebackend_bond(pkg, golden, tmp_path):
    import pandas as pd

    dis = _disorder_dir(golden, tmp_path)
    common = ["--mode", "fakebrisbane", "--L", "4", "--tf", "5", "--trajectories", "64",
              "--disorder_folder", str(dis)]
    outs = {}
    for tag, extra in (("none", []), ("zero", ["--fakebackend_bond", "0"]),
                       ("bond", ["--fakebackend_bond", "1"])):
        out = tmp_path / tag
        assert pkg.energy_cli.main(common + extra + ["--out_dir", str(out)]) == 0
        outs[tag] = out
    assert _files(outs["none"]) == _files(outs["zero"]) and len(_files(outs["none"])) == 1
    for f in _files(outs["none"]):
        assert open(outs["none"] / f, "rb").read() == open(outs["zero"] / f, "rb").read()
    (plain,) = _files(outs["none"])
    (bond,) = _files(outs["bond"])
    assert bond == plain[:-4] + "_bondcal.csv"
    a, b = pd.read_csv(outs["none"] / plain), pd.read_csv(outs["bond"] / bond)
    assert list(a.columns) == list(b.columns) == ["time", "energy_p_fakebrisbane"]
    assert a["energy_p_fakebrisbane"][0] == b["energy_p_fakebrisbane"][0]
    assert np.abs(a["energy_p_fakebrisbane"] - b["energy_p_fakebrisbane"]).max() > 1e-5
    # --bond_noise_prob with the depolarizing kick model
    out = tmp_path / "prob"
    assert pkg.energy_cli.main(["--mode", "full", "--L", "4", "--tf", "4", "--trajectories", "32",
                                "--bond_noise_prob", "0.05", "--disorder_folder", str(dis),
                                "--out_dir", str(out)]) == 0
    (name,) = _files(out)
    assert name.endswith("_bond0.05.csv")
