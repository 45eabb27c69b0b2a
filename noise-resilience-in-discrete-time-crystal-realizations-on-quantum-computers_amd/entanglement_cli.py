"""Command line for the reduced density matrices of site windows
(``entanglement.py``; ``DtcEngine.rdm_sums``).  The reference has no such script:
the flags are those of the autocorrelator and energy drivers (disorder files, g,
L, tf, noise, initial state, polarization), the outputs are ours.

Windows: ``--window_sites 0,1 4,5`` names them (all of one size, at most 4 sites,
each ascending); otherwise ``--window_size k`` slides a block of k adjacent sites
from ``--window_start`` in steps of ``--window_stride`` to the end of the chain.

Written under ``--out_dir`` into ``entanglement-data_L{L}/``:

    entanglement_data_{state}_g{g}_L{L}_inst{inst}_tf{tf}_randomphi{..}_delta{..}
        _amplitude{..}_noise{p}_usenoise{0|1}.csv
            columns time, then entropy_s{sites} and purity_s{sites} per window
            (sites joined by "-"): von Neumann entropy (natural log) and purity
            of each instance's trajectory-mean rho_A(t), averaged over instances
    entanglement_rho_....npy
            the instance-averaged mean matrices, complex ``[T][n_win][d][d]``

Blocks of 5..10 contiguous sites (``entanglement.get_instances_block``):
``--block_size k`` with one ``--block_start a`` per block (default 0) writes,
instead of the windows' files,

    entanglement_block_data_....csv
            columns time, then entropy_b{a}-{a+k-1}, purity_b.. (of the
            trajectory-mean rho_A) and renyi2_traj_b.. (the trajectory mean of
            -ln Tr rho_A^2 of each trajectory's own state) per block
    entanglement_block_rho_....npy
            the instance-averaged mean matrices, complex ``[T][n_blk][d][d]``

and ``--profile 1`` (``entanglement.entanglement_profile``) writes

    entanglement_profile_....csv
            columns time, then renyi2_traj_cut{l} for every cut l = 1 .. L-1
            and, without noise, entropy_cut{l}

The sites' initial state is the autocorrelator's (``neel`` = X on sites 1, 3,
...).  Depolarizing or noiseless kicks only.
"""
from __future__ import annotations

import argparse
import os

import numpy as np

from . import entanglement as en
from .disorder import load_disorder
from .engine import SweepSpec
from .kicks import POLARIZATIONS


def build_parser():
    p = argparse.ArgumentParser(
        description="DTC reduced density matrices, entropy and purity on MI355X (HIP engine)")
    p.add_argument("--L", type=int, default=4)
    p.add_argument("--device_name", type=int, default=0)
    p.add_argument("--inst", type=int, default=1)
    p.add_argument("--randomphi", type=int, default=1, help="Prethermal=0 or DTC=1 (file name)")
    p.add_argument("--phi_delta", type=float, default=0.0)
    p.add_argument("--phi_amplitude", type=float, default=1.0)
    p.add_argument("--tf", type=int, default=20)
    p.add_argument("--g", type=float, default=0.97)
    p.add_argument("--noise_prob", type=float, default=0.05)
    p.add_argument("--use_noise", type=int, default=1)
    p.add_argument("--initial_state", type=str, default="vacuum", choices=["vacuum", "neel"])
    p.add_argument("--polarization", type=str, default="x", choices=list(POLARIZATIONS))
    p.add_argument("--circular_frequency", type=float, default=1.0)
    p.add_argument("--window_sites", type=str, nargs="+", default=None,
                   help="windows as comma-separated ascending sites, e.g. 0,1 2,3")
    p.add_argument("--window_size", type=int, default=1, choices=[1, 2, 3, 4],
                   help="sliding block of adjacent sites (without --window_sites)")
    p.add_argument("--window_start", type=int, default=0)
    p.add_argument("--window_stride", type=int, default=1)
    p.add_argument("--block_size", type=int, default=None, choices=[5, 6, 7, 8, 9, 10],
                   help="blocks of this many contiguous sites (instead of windows)")
    p.add_argument("--block_start", type=int, action="append", default=None,
                   help="first site of a block (repeatable; default 0)")
    p.add_argument("--profile", type=int, default=0, choices=[0, 1],
                   help="1: the Renyi-2 entanglement across every cut of the chain")
    p.add_argument("--trajectories", type=int, default=1024,
                   help="noisy trajectories per instance (1 is used without noise)")
    p.add_argument("--seed", type=int, default=0x5EED0001)
    p.add_argument("--disorder_folder", type=str, default=".")
    p.add_argument("--out_dir", type=str, default=".")
    return p


def windows_from_args(args) -> np.ndarray:
    """The int32 ``[n_win][k]`` windows the flags name."""
    L = args.L
    if args.window_sites:
        wins = [[int(s) for s in w.split(",")] for w in args.window_sites]
        if len({len(w) for w in wins}) != 1:
            raise ValueError("all --window_sites windows must have the same size")
    else:
        k = args.window_size
        if args.window_stride < 1 or args.window_start < 0:
            raise ValueError("--window_stride >= 1 and --window_start >= 0")
        wins = [list(range(s, s + k)) for s in range(args.window_start, L - k + 1,
                                                       args.window_stride)]
        if not wins:
            raise ValueError(f"no window of {k} sites from site {args.window_start} fits L = {L}")
    for w in wins:
        if not 1 <= len(w) <= 4 or any(s < 0 or s >= L for s in w) or any(
                b <= a for a, b in zip(w, w[1:])):
            raise ValueError(f"window {w}: 1 to 4 strictly ascending sites in [0, {L})")
    return np.asarray(wins, dtype=np.int32)


def blocks_from_args(args):
    """The int32 ``[n_blk][2]`` ``(start, k)`` blocks the flags name, or None
    without ``--block_size``."""
    k = args.block_size
    if k is None:
        if args.block_start is not None:
            raise ValueError("--block_start needs --block_size")
        return None
    starts = args.block_start if args.block_start is not None else [0]
    if 2 * k > args.L:
        raise ValueError(f"--block_size {k}: a block has at most L / 2 = {args.L // 2} sites")
    for a in starts:
        if a < 0 or a + k > args.L:
            raise ValueError(f"block of {k} sites from site {a} does not fit L = {args.L}")
    return np.asarray([[a, k] for a in starts], dtype=np.int32)


def block_label(block) -> str:
    a, k = int(block[0]), int(block[1])
    return f"b{a}-{a + k - 1}"


def window_label(sites) -> str:
    return "s" + "-".join(str(int(s)) for s in sites)


def entanglement_folder(L: int) -> str:
    return f"entanglement-data_L{L}"


def entanglement_file_name(prefix, ext, state, g, L, inst, tf, randomphi, delta, amplitude, noise,
                           use_noise) -> str:
    return (f"{prefix}_{state}_g{g}_L{L}_inst{inst}_tf{tf}_randomphi{randomphi}_delta{delta}"
            f"_amplitude{amplitude}_noise{noise}_usenoise{use_noise}.{ext}")


def main(argv=None):
    import pandas as pd

    args = build_parser().parse_args(argv)
    L, T = args.L, args.tf
    blocks = blocks_from_args(args)
    wins = windows_from_args(args) if blocks is None and not args.profile else None
    hs, phis = load_disorder(L, args.inst, args.disorder_folder)
    spec = SweepSpec(L=L, T=T, hs=hs, phis=phis, g=args.g, polarization=args.polarization,
                     circular_frequency=args.circular_frequency,
                     initial_state=args.initial_state, noise_prob=args.noise_prob,
                     use_noise=args.use_noise)
    n_traj = args.trajectories if spec.p > 0 else 1
    name_args = (args.initial_state, args.g, L, args.inst, T, args.randomphi, args.phi_delta,
                 args.phi_amplitude, args.noise_prob, args.use_noise)
    folder = os.path.join(args.out_dir, entanglement_folder(L))
    if args.profile:
        os.makedirs(folder, exist_ok=True)
        prof = en.entanglement_profile(spec, n_traj, seed=args.seed)
        cols = {"time": np.arange(0, T)}
        for key in ("renyi2_traj", "entropy"):
            if key in prof:
                for c in range(L - 1):
                    cols[f"{key}_cut{c + 1}"] = prof[key][:, :, c].mean(axis=0)
        path = os.path.join(folder, entanglement_file_name("entanglement_profile", "csv",
                                                           *name_args))
        pd.DataFrame(cols).to_csv(path, index=False)
        print(f"Entanglement profile saved to {path}")
        if blocks is None:
            return 0
    if blocks is not None:
        os.makedirs(folder, exist_ok=True)
        res = en.get_instances_block(spec, n_traj, blocks, seed=args.seed)
        cols = {"time": np.arange(0, T)}
        for key in ("entropy", "purity", "renyi2_traj"):
            for w, blk in enumerate(blocks):
                cols[f"{key}_{block_label(blk)}"] = res[key][:, :, w].mean(axis=0)
        path = os.path.join(folder, entanglement_file_name("entanglement_block_data", "csv",
                                                           *name_args))
        pd.DataFrame(cols).to_csv(path, index=False)
        print(f"Block entanglement data saved to {path}")
        mpath = os.path.join(folder, entanglement_file_name("entanglement_block_rho", "npy",
                                                            *name_args))
        np.save(mpath, res["rho"].mean(axis=0))
        print(f"Mean block density matrices saved to {mpath}")
        return 0
    res = en.get_instances_rdm(spec, n_traj, wins, seed=args.seed)
    cols = {"time": np.arange(0, T)}
    for w, sites in enumerate(wins):
        cols["entropy_" + window_label(sites)] = res["entropy"][:, :, w].mean(axis=0)
    for w, sites in enumerate(wins):
        cols["purity_" + window_label(sites)] = res["purity"][:, :, w].mean(axis=0)
    os.makedirs(folder, exist_ok=True)
    path = os.path.join(folder, entanglement_file_name("entanglement_data", "csv", *name_args))
    pd.DataFrame(cols).to_csv(path, index=False)
    print(f"Entanglement data saved to {path}")
    mpath = os.path.join(folder, entanglement_file_name("entanglement_rho", "npy", *name_args))
    np.save(mpath, res["rho"].mean(axis=0))
    print(f"Mean reduced density matrices saved to {mpath}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
