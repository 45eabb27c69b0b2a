"""Reduced density matrices of site windows: entropy, purity, mutual information
and every k-local Pauli expectation.

``DtcEngine.rdm`` / ``rdm_sums`` (dtc_rdm, include/dtc.h) give the reduced state
``rho_A(t)`` of a window A of up to four sites for every trajectory and time.
``rho_A`` is linear in ``|psi><psi|``, so its trajectory mean is an unbiased
estimate of the depolarizing channel's exact reduced state.  Entropy, purity and
mutual information are *not* linear in rho: take them of the trajectory mean
(``get_instances_rdm``), never average them per trajectory.  The names here have
no counterpart in the reference.

Index convention (the C ABI's): for a window of sites ``s_0 < ... < s_{k-1}`` bit
m of a row index is the bit of ``s_m``; an operator on the window is
``kron(O_{s_{k-1}}, ..., O_{s_0})``.
"""
from __future__ import annotations

import numpy as np

from .engine import SweepSpec, refuse_rdm, window_array
from .energy import ESTIMATOR_SHOTS, _engine

PAULI = np.array([[[1, 0], [0, 1]], [[0, 1], [1, 0]], [[0, -1j], [1j, 0]], [[1, 0], [0, -1]]],
                 dtype=np.complex128)
PAULI_LETTERS = "IXYZ"


def _n_sites(rho) -> int:
    d = rho.shape[-1]
    k = int(d).bit_length() - 1
    if rho.ndim < 2 or rho.shape[-2] != d or d != 1 << k or k < 1:
        raise ValueError(f"rho must be [..., d, d] with d a power of two >= 2, got {rho.shape}")
    return k


def von_neumann_entropy(rho) -> np.ndarray:
    """``S = -Tr rho ln rho`` (natural log) of Hermitian matrices ``[..., d, d]``;
    eigenvalues are clipped at 0 (``0 ln 0 = 0``).  rho is taken as it is, not
    renormalised."""
    rho = np.asarray(rho, dtype=np.complex128)
    _n_sites(rho)
    lam = np.clip(np.linalg.eigvalsh(rho), 0.0, None)
    safe = np.where(lam > 0.0, lam, 1.0)
    return -(lam * np.log(safe)).sum(axis=-1)


def purity(rho) -> np.ndarray:
    """``Tr rho^2 = sum |rho_ab|^2`` of Hermitian matrices ``[..., d, d]``."""
    rho = np.asarray(rho, dtype=np.complex128)
    _n_sites(rho)
    return (rho.real ** 2 + rho.imag ** 2).sum(axis=(-2, -1))


def renyi2(rho) -> np.ndarray:
    """The second Renyi entropy ``-ln Tr rho^2``."""
    return -np.log(purity(rho))


def partial_trace(rho, keep) -> np.ndarray:
    """The reduced matrix ``[..., 2^n, 2^n]`` of the window positions ``keep``
    (ascending indices m into the window's sites, n = len(keep)) of
    ``rho [..., 2^k, 2^k]``; the kept sites keep their order."""
    rho = np.asarray(rho, dtype=np.complex128)
    k = _n_sites(rho)
    keep = [int(m) for m in keep]
    if not keep or any(m < 0 or m >= k for m in keep) or any(
            b <= a for a, b in zip(keep, keep[1:])):
        raise ValueError(f"keep must be ascending positions in [0, {k}), got {keep}")
    lead = rho.shape[:-2]
    for m in sorted(set(range(k)) - set(keep), reverse=True):
        # bit m of the row and column index, between `hi` higher and `lo` lower values
        d = rho.shape[-1]
        lo, hi = 1 << m, d >> (m + 1)
        r = rho.reshape(lead + (hi, 2, lo, hi, 2, lo))
        rho = (r[..., :, 0, :, :, 0, :] + r[..., :, 1, :, :, 1, :]).reshape(
            lead + (hi * lo, hi * lo))
    return rho


def mutual_information(rho_ij) -> np.ndarray:
    """``I(i:j) = S_i + S_j - S_ij`` of two-site matrices ``[..., 4, 4]``."""
    rho_ij = np.asarray(rho_ij, dtype=np.complex128)
    if _n_sites(rho_ij) != 2:
        raise ValueError("mutual_information takes two-site matrices [..., 4, 4]")
    return (von_neumann_entropy(partial_trace(rho_ij, [0]))
            + von_neumann_entropy(partial_trace(rho_ij, [1]))
            - von_neumann_entropy(rho_ij))


def pauli_strings(k: int) -> list:
    """The 4^k Pauli strings in the order of ``pauli_expectations``: entry q has
    letter ``IXYZ[(q >> 2 m) & 3]`` on the window's m-th site; the string is
    written site 0 first, e.g. k = 2, q = 7 is "ZX" = Z on s_0, X on s_1."""
    return ["".join(PAULI_LETTERS[(q >> (2 * m)) & 3] for m in range(k)) for q in range(4 ** k)]


def pauli_operator(q: int, k: int) -> np.ndarray:
    """``kron(P_{k-1}, ..., P_0)`` with ``P_m = PAULI[(q >> 2 m) & 3]``."""
    op = np.ones((1, 1), dtype=np.complex128)
    for m in range(k):
        op = np.kron(PAULI[(q >> (2 * m)) & 3], op)
    return op


def pauli_expectations(rho) -> np.ndarray:
    """``Tr(rho P_q)`` for all 4^k Pauli strings of ``rho [..., 2^k, 2^k]``, real
    ``[..., 4^k]`` in the order of ``pauli_strings`` (entry 0 is Tr rho)."""
    rho = np.asarray(rho, dtype=np.complex128)
    k = _n_sites(rho)
    ops = np.stack([pauli_operator(q, k) for q in range(4 ** k)])
    # Tr(rho P) = sum_ab rho_ab P_ba
    return np.einsum("...ab,qba->...q", rho, ops).real


def get_instances_rdm(spec: SweepSpec, n_traj: int = ESTIMATOR_SHOTS, windows=((0,),),
                      seed: int = 0x5EED0001, engine=None, traj_offset: int = 0) -> dict:
    """The noise-averaged reduced state per instance and time from the engine's
    on-device trajectory sums (``DtcEngine.rdm_sums``): ``rho``
    ``[n_inst][T][n_win][d][d]`` the trajectory mean, ``entropy`` and ``purity``
    ``[n_inst][T][n_win]`` of that mean, ``windows`` the int32 ``[n_win][k]`` sites."""
    refuse_rdm(spec, "get_instances_rdm")
    win = window_array(windows)
    rho = _engine(engine).rdm_sums(spec, n_traj, win, seed=seed, traj_offset=traj_offset) / n_traj
    return {"rho": rho, "entropy": von_neumann_entropy(rho), "purity": purity(rho),
            "windows": win}
