"""Bond noise on the MI355X (dtc_autocorr_bond, include/dtc.h): per-trajectory
parity of the HIP engine with the literal numpy model of tests/bond_model.py
(every gate of autocorr-delta-a-single-qiskit-fast.py:111-121 / 140-143 one by
one, the drawn Pauli pair after each RZZ / RZZ^+), the unchanged kick draws,
the trajectory mean against the exact channel, batch / split invariance and
the facade.
"""
import numpy as np
import pytest

from tests import bond_model as bm
from tests.helpers import random_disorder

pytestmark = pytest.mark.gpu
P_BOND = 0.4


def _draw(pkg, p_bond, L, seed, traj):
    return lambda s, c: pkg.engine.bond_draws(p_bond, L, seed, traj, s, c)


def _coverage(pkg, L, T, n_traj, seed, probe):
    """Which sign rules the seed's draws exercise (from dtc_bond_draws)."""
    got = dict(probe_x=False, odd_fwd=False, even_inv=False, z_only=False)
    for r in range(n_traj):
        d = _draw(pkg, P_BOND, L, seed, r)
        for t in range(1, T):
            codes = d(0, t)
            # an X or Y on the probe from a bond touching it, not cancelled by the other
            got["probe_x"] |= bool(bm.outgoing_x(L, codes)[probe] == 1)
            got["odd_fwd"] |= bool(np.any(bm.flip_signs(L, codes, False)[1][1::2] < 0))
            layers = [codes] + [d(1 + t, k) for k in range(1, t + 1)]
            for k in range(1, t + 1):
                got["even_inv"] |= bool(np.any(bm.flip_signs(L, layers[k], True)[1][0::2] < 0))
            for cs in layers:
                got["z_only"] |= any(c in (3, 12, 15) for c in cs)
    return got


# (L, T, n_inst, n_traj, batch, polarization, seed); the seeds were picked on
# the CPU so that every sign rule is exercised (asserted below)
CASES = [
    pytest.param(5, 4, 1, 9, 0, "x", 11, id="L5-padded-tile"),
    pytest.param(14, 4, 2, 9, 8, "x", 11, id="L14-10+4-octets"),
    pytest.param(14, 4, 2, 9, 8, "xy", 11, id="L14-xy-general-kicks"),
    pytest.param(20, 3, 1, 2, 0, "x", 11, id="L20-12+8"),
]


@pytest.mark.parametrize("L,T,n_inst,n_traj,batch,pol,seed", CASES)
def test_per_trajectory_parity_with_literal_model(pkg, engine, L, T, n_inst, n_traj, batch, pol,
                                                  seed):
    rng = np.random.default_rng(1000 + L)
    hs, phis = random_disorder(rng, L, n_inst)
    spec = pkg.SweepSpec(L=L, T=T, hs=hs, phis=phis, g=0.94, polarization=pol, noise_prob=0.0,
                         use_noise=0, initial_state="neel", bond_noise=P_BOND)
    assert spec.n_sub == (2 if pol == "xy" else 1)
    cov = _coverage(pkg, L, T, n_traj, seed, spec.probe_site)
    assert all(cov.values()), cov
    got = engine.autocorr(spec, n_traj, seed=seed, want_zsite=True, batch=batch)
    ref = {k: np.zeros_like(got[k]) for k in ("fwd", "echo", "zsite")}
    for i in range(n_inst):
        for r in range(n_traj):
            f, e, z = bm.literal_trajectory(L, T, spec.hs[i], spec.phis[i], spec.kick,
                                            spec.init_mask, spec.probe_site,
                                            _draw(pkg, P_BOND, L, seed, r))
            ref["fwd"][i, r], ref["echo"][i, r], ref["zsite"][i, r] = f, e, z
    for k in ("fwd", "echo", "zsite"):
        err = float(np.abs(got[k] - ref[k]).max())
        print(f"{k}: max |engine - literal| = {err:.3e}")
        assert err < 1e-10, (k, err)
    # the noise is visible: the noiseless sweep differs
    clean = engine.autocorr(pkg.SweepSpec(L=L, T=T, hs=hs, phis=phis, g=0.94, polarization=pol,
                                          noise_prob=0.0, use_noise=0, initial_state="neel"),
                            1, seed=seed)
    assert np.abs(clean["echo"] - 1.0).max() < 1e-10
    assert np.abs(got["echo"] - 1.0).max() > 1e-3


def test_kick_draws_unchanged(pkg, engine):
    L, T = 14, 4
    rng = np.random.default_rng(7)
    hs, phis = random_disorder(rng, L, 2)
    base = dict(L=L, T=T, hs=hs, phis=phis, g=0.97, noise_prob=0.05, initial_state="neel")
    plain = engine.autocorr(pkg.SweepSpec(**base), 9, seed=5, want_zsite=True, batch=8)
    # a non-null p_bond of zeros through dtc_autocorr_bond itself
    import ctypes

    spec = pkg.SweepSpec(**base)
    pr = engine._problem(spec, True, True, 8, 0)
    nz = engine._noise(spec)
    zeros = np.zeros(L - 1)
    bd = pkg.engine.bond_struct(zeros)
    out = {k: np.zeros_like(v) for k, v in plain.items()}
    pkg._capi.check(engine._lib.dtc_autocorr_bond(
        engine._ctx, ctypes.byref(pr), ctypes.byref(nz), None, ctypes.byref(bd),
        ctypes.c_uint64(5), ctypes.c_int64(0), ctypes.c_int32(9), pkg._capi.as_dptr(out["fwd"]),
        pkg._capi.as_dptr(out["echo"]), pkg._capi.as_dptr(out["zsite"])))
    for k in plain:
        assert np.abs(out[k] - plain[k]).max() <= 1e-13, k
    # and with one bond noisy, the kick draws are still those of the plain run:
    # a trajectory whose bond draws are all II equals the plain one
    pb = np.zeros(L - 1)
    pb[3] = 0.02
    noisy = engine.autocorr(pkg.SweepSpec(**base, bond_noise=pb), 9, seed=5, want_zsite=True,
                            batch=8)
    quiet = [r for r in range(9)
             if not any(pkg.engine.bond_draws(pb, L, 5, r, s, c).any()
                        for s, c in [(0, t) for t in range(1, T)]
                        + [(1 + t, k) for t in range(1, T) for k in range(1, t + 1)])]
    assert len(quiet) >= 3
    for k in plain:
        assert np.abs(noisy[k][:, quiet] - plain[k][:, quiet]).max() <= 1e-13, k


def test_mixed_noise_against_exact_channel(pkg, engine):
    L, T, p, pb, N = 4, 6, 0.05, 0.1, 16384
    rng = np.random.default_rng(21)
    hs, phis = random_disorder(rng, L)
    spec = pkg.SweepSpec(L=L, T=T, hs=hs, phis=phis, g=0.97, noise_prob=p, initial_state="neel",
                         bond_noise=pb)
    got = engine.autocorr(spec, N, seed=0xD1CE)
    ref_f, ref_e = bm.exact_sweep(L, T, spec.hs[0], spec.phis[0], spec.kick, pb, p,
                                  spec.init_mask, spec.probe_site)
    bound = 5.0 / np.sqrt(N)
    for k, ref in (("fwd", ref_f), ("echo", ref_e)):
        err = float(np.abs(got[k][0].mean(axis=0) - ref).max())
        print(f"{k}: max |mean - exact| = {err:.3e} (bound {bound:.3e})")
        assert err <= bound, (k, err)
    # the bond channel is resolved at this N: the exact curve without it is further away
    no_f, no_e = bm.exact_sweep(L, T, spec.hs[0], spec.phis[0], spec.kick, 0.0, p,
                                spec.init_mask, spec.probe_site)
    assert np.abs(no_e - ref_e).max() > 2 * bound


def test_rows_invariant_under_batch_and_split(pkg, engine):
    L, T = 14, 4
    rng = np.random.default_rng(9)
    hs, phis = random_disorder(rng, L, 2)
    spec = pkg.SweepSpec(L=L, T=T, hs=hs, phis=phis, g=0.97, noise_prob=0.05,
                         initial_state="neel", bond_noise=0.2)
    kw = dict(seed=77, want_zsite=True)
    a = engine.autocorr(spec, 16, batch=0, **kw)
    b = engine.autocorr(spec, 16, batch=8, **kw)
    lo = engine.autocorr(spec, 8, traj_offset=0, batch=0, **kw)
    hi = engine.autocorr(spec, 8, traj_offset=8, batch=0, **kw)
    for k in ("fwd", "echo", "zsite"):
        assert np.array_equal(a[k], b[k]), k
        assert np.array_equal(a[k], np.concatenate([lo[k], hi[k]], axis=1)), k


def test_facade_end_to_end(pkg, engine):
    aer = pkg.aer
    L, n_fwd, p, pb, shots, seed = 4, 3, 0.05, 0.1, 512, 4242
    rng = np.random.default_rng(33)
    hs, phis = random_disorder(rng, L)
    nm = aer.NoiseModel()
    nm.add_all_qubit_quantum_error(aer.depolarizing_error(p, 1), ["u1", "u2", "u3"])
    nm.add_all_qubit_quantum_error(aer.depolarizing_error(pb, 2), ["rzz"])
    spec = pkg.SweepSpec(L=L, T=n_fwd + 1, hs=hs, phis=phis, g=0.97, noise_prob=p, bond_noise=pb)
    for echo in (False, True):
        circ = pkg.circuit.dtc_circuit(
            L, n_fwd, spec.hs[0], spec.phis[0],
            lambda step: pkg.kicks.period_gate_specs("x", 0.97, step), echo=echo)
        res = aer.DtcSimulator(noise_model=nm).run(circ, shots=shots, seed_simulator=seed).result()
        out = engine.autocorr(spec, shots, seed=seed, want_fwd=not echo, want_echo=echo,
                              t_first=n_fwd)
        want = float(out["echo" if echo else "fwd"][0, :, n_fwd].mean())
        assert abs(res.expectations[0] - want) < 1e-12, (echo, res.expectations[0], want)
        assert sum(res.get_counts().values()) == shots
