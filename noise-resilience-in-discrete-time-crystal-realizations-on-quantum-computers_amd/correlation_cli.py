"""Command line for the all-pair correlators and the spin-glass order parameter
(``correlations.py``; ``DtcEngine.correlation_sums``).  The reference has no such
script: the flags are those of the autocorrelator and energy drivers (disorder
files, g, L, tf, noise, initial state, polarization), the outputs are ours.

Written under ``--out_dir`` into ``correlation-data_L{L}/``:

    correlation_data_{state}_g{g}_L{L}_inst{inst}_tf{tf}_randomphi{..}_delta{..}
        _amplitude{..}_noise{p}_usenoise{0|1}.csv
            columns time, chi_sg_z, chi_sg_z_connected[, chi_sg_x]: chi_SG(t) of
            each instance's trajectory-mean matrix, averaged over the instances
            (``_connected``: of C_ij - <Z_i><Z_j>); chi_sg_x with ``--bases zx``
    correlation_matrix_z_....npy (and _x_ with ``--bases zx``)
            the instance-averaged mean matrices <Z_i Z_j>(t), ``[T][L][L]``, unit
            diagonal

The sites' initial state is the autocorrelator's (``neel`` = X on sites 1, 3,
...).  Depolarizing or noiseless kicks only.
"""
from __future__ import annotations

import argparse
import os

import numpy as np

from . import correlations as co
from .disorder import load_disorder
from .engine import SweepSpec
from .kicks import POLARIZATIONS


def build_parser():
    p = argparse.ArgumentParser(
        description="DTC all-pair correlators and spin-glass order on MI355X (HIP engine)")
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
    p.add_argument("--bases", type=str, default="z", choices=["z", "zx"],
                   help="zx = also <X_i X_j> (one basis-change pass per site group and time)")
    p.add_argument("--trajectories", type=int, default=1024,
                   help="noisy trajectories per instance (1 is used without noise)")
    p.add_argument("--seed", type=int, default=0x5EED0001)
    p.add_argument("--disorder_folder", type=str, default=".")
    p.add_argument("--out_dir", type=str, default=".")
    return p


def correlation_folder(L: int) -> str:
    return f"correlation-data_L{L}"


def correlation_file_name(prefix, ext, state, g, L, inst, tf, randomphi, delta, amplitude, noise,
                          use_noise) -> str:
    return (f"{prefix}_{state}_g{g}_L{L}_inst{inst}_tf{tf}_randomphi{randomphi}_delta{delta}"
            f"_amplitude{amplitude}_noise{noise}_usenoise{use_noise}.{ext}")


def main(argv=None):
    import pandas as pd

    args = build_parser().parse_args(argv)
    L, T = args.L, args.tf
    hs, phis = load_disorder(L, args.inst, args.disorder_folder)
    spec = SweepSpec(L=L, T=T, hs=hs, phis=phis, g=args.g, polarization=args.polarization,
                     circular_frequency=args.circular_frequency,
                     initial_state=args.initial_state, noise_prob=args.noise_prob,
                     use_noise=args.use_noise)
    n_traj = args.trajectories if spec.p > 0 else 1
    plain = co.get_instances_correlations(spec, n_traj, bases=args.bases, seed=args.seed)
    conn = co.pair_matrix(co.connected(co.pair_vector(plain["zz"]), plain["z"]), L)
    cols = {"time": np.arange(0, T),
            "chi_sg_z": plain["chi_sg_z"].mean(axis=0),
            "chi_sg_z_connected": co.spin_glass_order(conn).mean(axis=0)}
    if "x" in args.bases:
        cols["chi_sg_x"] = plain["chi_sg_x"].mean(axis=0)
    name_args = (args.initial_state, args.g, L, args.inst, T, args.randomphi, args.phi_delta,
                 args.phi_amplitude, args.noise_prob, args.use_noise)
    folder = os.path.join(args.out_dir, correlation_folder(L))
    os.makedirs(folder, exist_ok=True)
    path = os.path.join(folder, correlation_file_name("correlation_data", "csv", *name_args))
    pd.DataFrame(cols).to_csv(path, index=False)
    print(f"Correlation data saved to {path}")
    for b in args.bases:
        mpath = os.path.join(folder, correlation_file_name(f"correlation_matrix_{b}", "npy",
                                                           *name_args))
        np.save(mpath, plain[2 * b].mean(axis=0))
        print(f"<{b.upper()}_i {b.upper()}_j> matrices saved to {mpath}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
