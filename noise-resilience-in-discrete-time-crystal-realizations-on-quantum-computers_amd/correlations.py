"""All-pair correlators and the spin-glass (Edwards-Anderson) order parameter.

The reference scripts measure a probe site's autocorrelator and the terms of H;
neither shows spatial order.  The standard diagnostic of the MBL discrete time
crystal is the two-point matrix ``C_ij(t) = <Z_i Z_j>`` and

    chi_SG(t) = 1 / (L (L - 1)) * sum_{i != j} C_ij(t)^2,

which stays finite in the DTC while the disorder-averaged ``<Z_i>`` vanishes.
``DtcEngine.correlations`` / ``correlation_sums`` (dtc_correlations, include/dtc.h)
give the exact ``<Z_i Z_j>`` (and ``<X_i X_j>``) of every trajectory's state at
every time; ``C_ij`` is linear in the density matrix, so the trajectory mean is
an unbiased estimate of the depolarizing channel's exact value.  The names here
have no counterpart in the reference.
"""
from __future__ import annotations

import numpy as np

from .engine import SweepSpec, refuse_correlations
from .energy import ESTIMATOR_SHOTS, _engine


def pair_index(L: int):
    """The sites ``(i, j)`` (two int arrays of length L(L-1)/2) of the pair
    entries in the C ABI's order: row-major (0,1), (0,2), ..., (L-2,L-1)."""
    i, j = np.triu_indices(int(L), k=1)
    return i, j


def pair_matrix(zz, L: int) -> np.ndarray:
    """``zz [..., L(L-1)/2]`` as the symmetric matrix ``[..., L, L]`` with unit
    diagonal (Z_i^2 = 1)."""
    zz = np.asarray(zz, dtype=np.float64)
    i, j = pair_index(L)
    if zz.shape[-1] != i.size:
        raise ValueError(f"last axis must hold L(L-1)/2 = {i.size} pairs, got {zz.shape[-1]}")
    C = np.zeros(zz.shape[:-1] + (L, L))
    C[..., i, j] = zz
    C[..., j, i] = zz
    d = np.arange(L)
    C[..., d, d] = 1.0
    return C


def pair_vector(C) -> np.ndarray:
    """The inverse of ``pair_matrix``: the upper triangle in the ABI's order."""
    C = np.asarray(C)
    i, j = pair_index(C.shape[-1])
    return C[..., i, j]


def connected(zz_mean, z_mean) -> np.ndarray:
    """``C_ij - <Z_i><Z_j>`` per pair from mean pair entries ``[..., L(L-1)/2]`` and
    mean sites ``[..., L]``."""
    z = np.asarray(z_mean, dtype=np.float64)
    i, j = pair_index(z.shape[-1])
    return np.asarray(zz_mean, dtype=np.float64) - z[..., i] * z[..., j]


_connected = connected  # (get_instances_correlations has a flag of that name)


def spin_glass_order(C) -> np.ndarray:
    """``chi_SG = 1 / (L (L - 1)) sum_{i != j} C_ij^2`` of matrices ``[..., L, L]``
    (the diagonal is ignored).  For a noisy sweep ``C`` is the trajectory mean of
    one disorder instance; average chi_SG over the instances afterwards.

    Squaring an n-trajectory mean is biased upwards by ``Var(c_ij) / n`` per pair
    (the mean's own variance); ``spin_glass_order_unbiased`` removes that."""
    C = np.asarray(C, dtype=np.float64)
    L = C.shape[-1]
    if L < 2:
        return np.zeros(C.shape[:-2])
    sq = C * C
    d = np.arange(L)
    return (sq.sum(axis=(-2, -1)) - sq[..., d, d].sum(axis=-1)) / (L * (L - 1))


def spin_glass_order_unbiased(rows, axis: int = 0) -> np.ndarray:
    """chi_SG from per-trajectory pair rows ``c_r`` (``axis`` numbers the n >= 2
    trajectories, the last axis the L(L-1)/2 pairs) with the U-statistic
    ``(S^2 - sum_r c_r^2) / (n (n - 1))``, ``S = sum_r c_r``, per pair: the mean of
    ``c_r c_r'`` over r != r', whose expectation is ``E[c]^2`` exactly -- no
    ``Var / n`` bias -- averaged over the pairs."""
    rows = np.asarray(rows, dtype=np.float64)
    n = rows.shape[axis]
    if n < 2:
        raise ValueError("the unbiased estimator needs at least two trajectories")
    s = rows.sum(axis=axis)
    s2 = (rows * rows).sum(axis=axis)
    return ((s * s - s2) / (n * (n - 1))).mean(axis=-1)


def get_instances_correlations(spec: SweepSpec, n_traj: int = ESTIMATOR_SHOTS, bases: str = "z",
                               connected: bool = False, seed: int = 0x5EED0001, engine=None,
                               traj_offset: int = 0) -> dict:
    """Per-instance trajectory means and chi_SG(t) from the engine's on-device
    trajectory sums (``DtcEngine.correlation_sums``).  For every basis b of
    ``bases``: ``b`` ``[n_inst][T][L]`` the mean sites, ``bb`` ``[n_inst][T][L][L]`` the
    mean matrices (``connected=True``: minus ``<Z_i><Z_j>``, diagonal kept 1),
    ``chi_sg_b`` ``[n_inst][T]``.  chi_SG is the square of the n_traj-trajectory
    mean (biased by ``Var / n_traj``, see ``spin_glass_order``)."""
    refuse_correlations(spec, "get_instances_correlations")
    sums = _engine(engine).correlation_sums(spec, n_traj, bases=bases, seed=seed,
                                            traj_offset=traj_offset)
    out = {}
    for b in "zx":
        if b not in sums:
            continue
        m1, m2 = sums[b] / n_traj, sums[2 * b] / n_traj
        if connected:
            m2 = _connected(m2, m1)
        out[b] = m1
        out[2 * b] = pair_matrix(m2, spec.L)
        out["chi_sg_" + b] = spin_glass_order(out[2 * b])
    return out
