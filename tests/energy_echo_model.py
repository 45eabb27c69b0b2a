"""Reference models of the energy echo (dtc_energy_echo), composed from the
oracles: one trajectory gate by gate with the C oracle's periods, and the exact
channel with the density-matrix oracle's.

Row t is the forward state after p = t + t_offset periods (stream 0, counter =
period) taken through p inverse periods (stream 1 + t, counter = step k, step k
undoing period p - k + 1) -- the state orc_autocorr measures its echo on.
"""
import dataclasses

import numpy as np

from oracle import c_oracle, dm_oracle, energy_oracle


def trajectory_energy_echo(spec, inst, traj, seed=0x5EED0001, t_first=0):
    """z [T][L], zz [T][L-1], x [T][L] of one trajectory's echo states; rows
    before ``t_first`` stay 0 (as the engine leaves them)."""
    one = dataclasses.replace(spec, hs=spec.hs[inst:inst + 1], phis=spec.phis[inst:inst + 1])
    L, T = spec.L, spec.T
    psi = np.zeros(1 << L, dtype=np.complex128)
    psi[energy_oracle.prep_mask(spec, seed, traj)] = 1.0
    z = np.zeros((T, L))
    zz = np.zeros((T, max(L - 1, 0)))
    xs = np.zeros((T, L))
    for s in range(T - 1 + spec.t_offset + 1):
        if s > 0:
            psi, _ = c_oracle.apply_periods(one, psi, s, 1, inst=0, traj=traj, stream=0,
                                            seed=seed)
        t = s - spec.t_offset
        if t < 0 or t < t_first:
            continue
        if s == 0:
            # the prepared basis state: its signs, no sum over 2^L amplitudes
            m = int(np.flatnonzero(psi)[0])
            z[t] = [-1.0 if (m >> i) & 1 else 1.0 for i in range(L)]
            zz[t] = z[t, :-1] * z[t, 1:]
            continue
        e, _ = c_oracle.apply_periods(one, psi, s, s, inverse=True, inst=0, traj=traj,
                                      stream=1 + t, seed=seed)
        z[t], zz[t], xs[t] = energy_oracle.observables(e, L)
    return z, zz, xs


def exact_energy_echo(L, T, hs, phis, kick, p, init_mask=0):
    """Exact <Z_i>, <Z_i Z_i+1>, <X_i> of the echo states under the depolarizing
    channel after every kick gate (forward and inverse) and after the prep X of
    every site in ``init_mask``: t forward periods, then their inverses."""
    N = 1 << L
    x = np.arange(N)
    w = np.ones(N)
    for i in range(L):
        pf = (1 - p / 2) if (init_mask >> i) & 1 else 0.0
        w = w * np.where(((x >> i) & 1) == 1, pf, 1 - pf)
    rho = dm_oracle.DM(L, np.diag(w).astype(np.complex128))
    gates = [dm_oracle.kick_gates_from_table(kick[s]) for s in range(T - 1)]
    zbits = 1 - 2 * ((x[None, :] >> np.arange(L)[:, None]) & 1)
    z = np.zeros((T, L))
    zz = np.zeros((T, max(L - 1, 0)))
    xs = np.zeros((T, L))
    for t in range(T):
        if t > 0:
            dm_oracle._period(rho, 0, L, gates[t - 1], hs, phis, p)
        e = rho.copy()
        for s in range(t, 0, -1):
            dm_oracle._period(e, 0, L, gates[s - 1], hs, phis, p, inverse=True)
        m = e.matrix()
        d = np.real(np.diag(m))
        z[t] = zbits @ d
        for i in range(L - 1):
            zz[t, i] = (zbits[i] * zbits[i + 1]) @ d
        for i in range(L):
            lo = x[((x >> i) & 1) == 0]
            xs[t, i] = 2.0 * np.real(m[lo ^ (1 << i), lo]).sum()
    return z, zz, xs
