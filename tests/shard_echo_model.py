"""Numpy model of the sharded echo steps (test infrastructure, no test in it):
``NumpyShardStepper`` plus the four echo methods the drivers of sharded.py
call, written from the definition in include/dtc.h (dtc_shard_echo_step):

* layer k >= 1 of chain t is the inverse kick of period p - k + 1 (p = t +
  t_offset): per site ``P_n G_1^+ ... P_1 G_n^+`` with the q-th Pauli drawn as
  ``sample_pauli(p_noise, seed, traj, 1 + t, k, site, q)`` -- q counts the
  gates in the order applied (kKickInverse, the C oracle's inverse period);
* layer 0 is the dagger of the forward kick of period p + 1 (same draws);
* the diagonal is the conjugate of the forward step's.
"""
from __future__ import annotations

import numpy as np

from oracle import c_oracle
from oracle.shard_oracle import PAULI, NumpyShardStepper, _row_matrix


class NumpyEchoStepper(NumpyShardStepper):
    @classmethod
    def _layer(cls, spec, t, k, site, seed, traj):
        p = t + spec.t_offset
        if k == 0:
            return cls._kick(spec, p + 1, site, seed, traj).conj().T
        period = p - k + 1
        M = np.eye(2, dtype=complex)
        for q in range(spec.n_sub):
            M = _row_matrix(spec.kick[period - 1, site, spec.n_sub - 1 - q]).conj().T @ M
            if spec.p > 0:
                M = PAULI[c_oracle.sample_pauli(spec.p, seed, traj, 1 + t, k, site, q)] @ M
        return M

    def step_echo(self, spec, layout, seed, traj, inst, t, k, pre, diag, post, src, dst,
                  want_obs):
        nl = layout.n_local
        if k < 0 or k > t + spec.t_offset or (post and k == t + spec.t_offset):
            raise ValueError("layer outside the chain")
        psi = src.numpy().reshape(layout.n_shards, -1).copy()
        for q in range(nl):
            if (pre >> q) & 1:
                self._apply(psi, nl, q, self._layer(spec, t, k, layout.site_of[q], seed, traj))
        obs = np.zeros((layout.n_shards, 1 + nl)) if want_obs else None
        h, ph = spec.hs[inst], spec.phis[inst]
        for b in range(layout.n_shards):
            z = self._logical_z(layout, layout.first_rank + b)
            if diag:
                ang = (h[:, None] * z).sum(axis=0)
                if spec.L > 1:
                    ang += (ph[:, None] * z[:-1] * z[1:]).sum(axis=0)
                psi[b] *= np.exp(+0.5j * ang)
            if want_obs:
                pr = np.abs(psi[b]) ** 2
                obs[b, 0] = pr.sum()
                x = np.arange(1 << nl)
                for q in range(nl):
                    obs[b, 1 + q] = ((1.0 - 2.0 * ((x >> q) & 1)) * pr).sum()
        for q in range(nl):
            if (post >> q) & 1:
                self._apply(psi, nl, q,
                            self._layer(spec, t, k + 1, layout.site_of[q], seed, traj))
        if dst is not None:
            dst.numpy().reshape(layout.n_shards, -1)[:] = psi
        elif diag or post or not want_obs:
            raise ValueError("dst None is the measured kick-only end")
        return obs

    def step_echo_async(self, spec, layout, seed, traj, inst, t, k, pre, diag, post, src, dst,
                        obs_out):
        obs = self.step_echo(spec, layout, seed, traj, inst, t, k, pre, diag, post, src, dst,
                             obs_out is not None)
        if obs_out is not None:
            obs_out.numpy()[...] = obs

    def kick_slice_echo(self, spec, layout, seed, traj, t, k, pre, chunk_bits, slice_bits,
                        slice_, buf):
        nl = layout.n_local
        nsub = nl - chunk_bits - slice_bits
        if pre >> nsub:
            raise ValueError("slice kick mask reaches the chunk/slice bits")
        psi = buf.numpy().reshape(layout.n_shards << chunk_bits, 1 << slice_bits, 1 << nsub)
        sub = psi[:, slice_, :].copy()
        for q in range(nsub):
            if (pre >> q) & 1:
                self._apply(sub, nsub, q, self._layer(spec, t, k, layout.site_of[q], seed, traj))
        psi[:, slice_, :] = sub

    def kick_exchange_slice_echo(self, spec, layout, seed, traj, t, k, pre, slice_bits, slice_,
                                 buf):
        self.kick_slice_echo(spec, layout, seed, traj, t, k, pre, layout.n_global, slice_bits,
                             slice_, buf)
        self.exchange_slice(layout, slice_bits, slice_, buf)
