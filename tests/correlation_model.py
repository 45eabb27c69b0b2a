"""The oracle side of the all-pair correlator tests (test infrastructure only):
correlators of a state by direct numpy sums, the rows of one noisy trajectory
from the C oracle's states (tests/sample_model.trajectory_states), and the
depolarizing channel's exact values from a density matrix (oracle.dm_oracle)."""
import numpy as np

from oracle import dm_oracle
from tests import sample_model as sm

EPS = sm.EPS  # the project's standing figure for engine against oracle

# the trajectory-mean test (tests/test_correlations_cpu.py): every summand lies
# in [-1, 1], so a mean of n has standard deviation <= 1 / sqrt(n): bound 5 / sqrt(n)
CHANNEL = dict(L=4, T=4, p=0.05, n=4096, seed=77)


def pairs(L):
    """(i, j) arrays in the C ABI's order, written out independently of the package."""
    ij = [(i, j) for i in range(L) for j in range(i + 1, L)]
    return (np.array([a for a, _ in ij], dtype=np.int64),
            np.array([b for _, b in ij], dtype=np.int64))


def signs(L):
    x = np.arange(1 << L)
    return 1.0 - 2.0 * ((x[None, :] >> np.arange(L)[:, None]) & 1)


DIRECT_MAX_L = 14  # direct sums up to here; larger states by the Walsh-Hadamard transform


def weights_correlators_direct(w, L):
    """z [L], zz [L(L-1)/2] of the probability vector w by direct sums."""
    s = signs(L)
    i, j = pairs(L)
    z = s @ w
    zz = np.array([np.dot(s[a] * s[b], w) for a, b in zip(i, j)]) if L > 1 else np.zeros(0)
    return z, zz


def weights_correlators_wht(w, L):
    """The same numbers as the entries at masks of weight 1 and 2 of w's
    Walsh-Hadamard transform (one numpy butterfly stage per site): for the
    states whose direct sums would take seconds each.  Agrees with the direct
    sums to rounding (tests/test_correlations_cpu.py)."""
    a = np.array(w, dtype=np.float64)
    for q in range(L):
        v = a.reshape(-1, 2, 1 << q)
        lo = v[:, 0, :].copy()
        v[:, 0, :] += v[:, 1, :]
        v[:, 1, :] = lo - v[:, 1, :]
    i, j = pairs(L)
    return a[1 << np.arange(L)], a[(1 << i) | (1 << j)]


def weights_correlators(w, L):
    return (weights_correlators_direct if L <= DIRECT_MAX_L else weights_correlators_wht)(w, L)


def state_correlators(psi, L, basis=0):
    a = sm.hadamard_all(psi, L) if basis else np.asarray(psi)
    return weights_correlators(a.real * a.real + a.imag * a.imag, L)


def trajectory_rows(spec, inst, traj, seed, bases="zx"):
    """{"z": [T][L], "zz": [T][L(L-1)/2], "x": ..., "xx": ...} of one trajectory;
    the row of p = 0 in the X basis is 0 (the contract's basis-state rule)."""
    L, T = spec.L, spec.T
    n_pair = L * (L - 1) // 2
    out = {}
    for b in bases:
        out[b] = np.zeros((T, L))
        out[2 * b] = np.zeros((T, n_pair))
    for t, psi in sm.trajectory_states(spec, inst, traj, seed):
        for k, b in enumerate("zx"):
            if b not in bases or (b == "x" and t + spec.t_offset == 0):
                continue
            out[b][t], out[2 * b][t] = state_correlators(psi, L, k)
    return out


def exact_channel(spec, inst=0):
    """The same rows of the exact depolarizing channel: the density matrix of
    oracle.dm_oracle.energy_sweep's preparation (vacuum) stepped period by period."""
    L, T = spec.L, spec.T
    assert spec.init_mask == 0 and spec.t_offset == 0
    rho0 = np.zeros((1 << L, 1 << L), dtype=np.complex128)
    rho0[0, 0] = 1.0
    rho = dm_oracle.DM(L, rho0)
    n_pair = L * (L - 1) // 2
    out = {k: np.zeros((T, L if len(k) == 1 else n_pair)) for k in ("z", "zz", "x", "xx")}
    for t in range(T):
        if t > 0:
            dm_oracle._period(rho, 0, L, dm_oracle.kick_gates_from_table(spec.kick[t - 1]),
                              spec.hs[inst], spec.phis[inst], spec.p)
        out["z"][t], out["zz"][t] = weights_correlators(np.real(np.diag(rho.matrix())), L)
        if t == 0:
            continue
        r = rho.copy()
        for q in range(L):
            r.u1(q, dm_oracle.H)
        out["x"][t], out["xx"][t] = weights_correlators(np.real(np.diag(r.matrix())), L)
    return out
