"""The oracle side of the measurement-sampling tests (test infrastructure only):
the states of one noisy trajectory from the C oracle's gate-by-gate periods, as
oracle/energy_oracle.trajectory_energy follows them, and the sampling rule of
include/dtc.h (dtc_sample) evaluated on them in extended precision."""
import dataclasses

import numpy as np

from oracle import c_oracle, energy_oracle

EPS = 1e-10  # the project's standing figure for engine against oracle

# the histogram test (tests/test_gpu_sample.py; its host twin in test_sample_cpu.py)
HIST = dict(L=4, T=4, t=3, n_shots=65536, seed=2024)


def trajectory_states(spec, inst, traj, seed):
    """(t, psi) for t = 0..T-1: the state after t + t_offset periods."""
    one = dataclasses.replace(spec, hs=spec.hs[inst:inst + 1], phis=spec.phis[inst:inst + 1])
    psi = np.zeros(1 << spec.L, dtype=np.complex128)
    psi[energy_oracle.prep_mask(spec, seed, traj)] = 1.0
    for s in range(spec.T - 1 + spec.t_offset + 1):
        if s > 0:
            psi, _ = c_oracle.apply_periods(one, psi, s, 1, inst=0, traj=traj, stream=0, seed=seed)
        if s - spec.t_offset >= 0:
            yield s - spec.t_offset, psi


def hadamard_all(psi, L):
    """H on every site (in place on a copy, one butterfly stage per site)."""
    a = np.array(psi, dtype=np.complex128)
    for q in range(L):
        v = a.reshape(-1, 2, 1 << q)
        lo = v[:, 0, :].copy()
        v[:, 0, :] += v[:, 1, :]
        v[:, 1, :] = lo - v[:, 1, :]
    a *= 2.0 ** (-0.5 * L)
    return a


def check_outcomes(bits, psi, u, what=""):
    """Every outcome x of the uniforms u on psi satisfies
    S(x - 1) - EPS <= u W <= S(x) + EPS, has non-zero weight and lies below 2^L."""
    w = psi.real * psi.real + psi.imag * psi.imag
    cs = np.cumsum(w, dtype=np.longdouble)
    x = np.asarray(bits).astype(np.int64)
    assert x.shape == np.shape(u), what
    assert np.all(x >= 0) and np.all(x < w.size), (what, x)
    tgt = np.asarray(u, dtype=np.longdouble) * cs[-1]
    lo = np.where(x > 0, cs[np.maximum(x - 1, 0)], np.longdouble(0))
    hi = cs[x]
    slack = float(max(np.max(lo - tgt), np.max(tgt - hi)))
    assert np.all(lo - EPS <= tgt) and np.all(tgt <= hi + EPS), (what, x, slack)
    assert np.all(w[x] > 0.0), (what, x)
    return slack


def pearson_chi2(bits, prob):
    """Pearson's chi^2 of the outcomes against the distribution prob."""
    n = np.size(bits)
    obs = np.bincount(np.asarray(bits).astype(np.int64).reshape(-1), minlength=prob.size)
    exp = n * prob
    return float(((obs - exp) ** 2 / exp).sum())


def chi2_bound(dof):
    return dof + 5.0 * np.sqrt(2.0 * dof)


def hist_spec(pkg):
    from tests.helpers import random_disorder

    hs, phis = random_disorder(np.random.default_rng(404), HIST["L"])
    return pkg.SweepSpec(L=HIST["L"], T=HIST["T"], hs=hs, phis=phis, g=0.9, noise_prob=0.0,
                         use_noise=0)


def hist_state(pkg):
    spec = hist_spec(pkg)
    for t, psi in trajectory_states(spec, 0, 0, HIST["seed"]):
        if t == HIST["t"]:
            return spec, psi
    raise AssertionError("no state at the histogram's time")
