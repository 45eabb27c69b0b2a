"""Reduced density matrices of site windows: entropy, purity, mutual information
and every k-local Pauli expectation.

``DtcEngine.rdm`` / ``rdm_sums`` (dtc_rdm, include/dtc.h) give the reduced state
``rho_A(t)`` of a window A of up to four sites for every trajectory and time.
``rho_A`` is linear in ``|psi><psi|``, so its trajectory mean is an unbiased
estimate of the depolarizing channel's exact reduced state.  Entropy, purity and
mutual information are *not* linear in rho: take them of the trajectory mean
(``get_instances_rdm``), never average them per trajectory.  The names here have
no counterpart in the reference.

Blocks of 5..10 contiguous sites -- the half chain up to L = 20 -- come from
``DtcEngine.rdm_block_sums`` (dtc_rdm_block_sums): the trajectory mean of rho_A
as above (``get_instances_block``), and the purity ``Tr rho_A^2`` of every
trajectory's own pure state, whose ``-ln`` is the trajectory-resolved second
Renyi *entanglement* entropy: that one is averaged per trajectory
(``renyi2_traj``), and in a noiseless run equals the Renyi-2 entropy of the mean.
``entanglement_profile`` takes every cut of the chain.

Index convention (the C ABI's): for a window of sites ``s_0 < ... < s_{k-1}`` bit
m of a row index is the bit of ``s_m``; an operator on the window is
``kron(O_{s_{k-1}}, ..., O_{s_0})``.
"""
from __future__ import annotations

import numpy as np

from .engine import SweepSpec, block_array, refuse_rdm, window_array
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


MAX_BLOCK = 10   # dtc_rdm_block_sums' largest block; dtc_rdm's is 4


def get_instances_block(spec: SweepSpec, n_traj: int = ESTIMATOR_SHOTS, blocks=((0, 5),),
                        seed: int = 0x5EED0001, engine=None, traj_offset: int = 0,
                        batch: int = 0) -> dict:
    """Blocks of 5..10 contiguous sites, ``blocks`` = ``(start, k)`` pairs of one
    size (``DtcEngine.rdm_block_sums``): ``rho`` ``[n_inst][T][n_blk][d][d]`` the
    trajectory mean, ``entropy`` and ``purity`` ``[n_inst][T][n_blk]`` of that
    mean, ``renyi2_traj`` ``[n_inst][T][n_blk]`` the trajectory mean of
    ``-ln Tr rho_A^2`` of each trajectory's own state, ``blocks`` int32
    ``[n_blk][2]``."""
    refuse_rdm(spec, "get_instances_block")
    res = _engine(engine).rdm_block_sums(spec, n_traj, block_array(blocks), seed=seed,
                                         traj_offset=traj_offset, batch=batch)
    rho = res["rho_sum"] / n_traj
    return {"rho": rho, "entropy": von_neumann_entropy(rho), "purity": purity(rho),
            "renyi2_traj": -np.log(res["purity"]).mean(axis=1), "blocks": res["blocks"]}


def profile_blocks(L: int) -> list:
    """The block ``(start, k)`` of every cut l = 1 .. L-1 of the chain (between
    sites l-1 and l): the smaller side, the left one ``[0, l)`` on a tie.  A pure
    state's two sides have the same spectrum, so either gives the cut's entropy.
    Refuses an L with a cut whose smaller side exceeds ``MAX_BLOCK`` sites."""
    if L < 2:
        raise ValueError("a cut needs L >= 2")
    if L // 2 > MAX_BLOCK:
        raise ValueError(f"L = {L}: the middle cuts' smaller side has {L // 2} sites, "
                         f"more than the {MAX_BLOCK} a block can have")
    return [(0, l) if l <= L - l else (l, L - l) for l in range(1, L)]


def entanglement_profile(spec: SweepSpec, n_traj: int = ESTIMATOR_SHOTS,
                         seed: int = 0x5EED0001, engine=None, traj_offset: int = 0) -> dict:
    """The entanglement across every cut of the chain: ``renyi2_traj``
    ``[n_inst][T][L-1]``, the trajectory mean of ``-ln Tr rho_A^2`` of each
    trajectory's own state, A the smaller side of cut l (``profile_blocks``); for
    a noiseless spec also ``entropy`` ``[n_inst][T][L-1]``, the von Neumann
    entanglement entropy of the (single) state.  Sides of up to four sites go
    through ``DtcEngine.rdm`` with the purity of each trajectory's matrix taken
    here, sides of 5..10 through ``rdm_block_sums``.  ``blocks``: int32
    ``[L-1][2]``."""
    refuse_rdm(spec, "entanglement_profile")
    L, T = spec.L, spec.T
    blocks = profile_blocks(L)
    eng = _engine(engine)
    noiseless = not spec.p > 0
    r2 = np.zeros((spec.n_inst, T, L - 1))
    ent = np.zeros((spec.n_inst, T, L - 1)) if noiseless else None
    for k in sorted({k for _, k in blocks}):
        cuts = [c for c, (_, kk) in enumerate(blocks) if kk == k]
        if k <= 4:
            rho = eng.rdm(spec, n_traj, [list(range(blocks[c][0], blocks[c][0] + k)) for c in cuts],
                          seed=seed, traj_offset=traj_offset)
            pur, mean = purity(rho), rho.mean(axis=1)
        else:
            res = eng.rdm_block_sums(spec, n_traj, [blocks[c] for c in cuts], seed=seed,
                                     traj_offset=traj_offset)
            pur, mean = res["purity"], res["rho_sum"] / n_traj
        r2[:, :, cuts] = -np.log(pur).mean(axis=1)
        if noiseless:
            ent[:, :, cuts] = von_neumann_entropy(mean)
    out = {"renyi2_traj": r2, "blocks": np.asarray(blocks, dtype=np.int32)}
    if noiseless:
        out["entropy"] = ent
    return out
