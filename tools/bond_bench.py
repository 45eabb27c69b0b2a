#!/usr/bin/env python3
"""Throughput of the bond-noise sweep (dtc_autocorr_bond) against the plain
schedule of dtc_autocorr, at the C2 shape (L=20, tf=30, p=0.05, vacuum,
tests/golden/disorder.json row 0).

    python tools/bond_bench.py [--traj 1024] [--steps 3] [--warmup 1] [--p_bond 0.01] [--out F]

Two engines, one after the other on device 0:
  plain  dtc_autocorr with DTC_NO_LIGHTCONE=1 DTC_NO_DUAL=1 (the schedule the
         bond runs are built from: no light-cone end, no dual pass),
  bond   dtc_autocorr_bond with p_bond on every bond.
Prints one JSON object: periods*instances/s of both (bench.py's unit), the
launch counts and times per kernel kind from kernel_stats, and the bond table
builder's share (time and bytes) of the diagonal pass it feeds.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def run(pkg, spec, B, steps, warmup):
    import torch

    eng = pkg.DtcEngine(0)
    try:
        for i in range(warmup):
            eng.autocorr(spec, B, seed=0x5EED0001, traj_offset=i * B, batch=B)
        eng.reset_stats()
        eng.set_profiling(True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(steps):
            out = eng.autocorr(spec, B, seed=0x5EED0001, traj_offset=(warmup + i) * B, batch=B)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        eng.set_profiling(False)
        stats = eng.kernel_stats()
        counts = eng.lightcone_counts(), eng.schedule_counts()
    finally:
        eng.close()
    T = spec.T
    per_traj = (T - 1) + sum(range(T))
    return {
        "value": steps * B * per_traj / dt, "unit": "periods*instances/s",
        "ms_per_step": dt / steps * 1e3,
        "echo_mean_last_t": float(out["echo"][0, :, -1].mean()),
        "kernel_stats": {pkg._capi.KERNEL_NAMES[k].split()[0]: v for k, v in stats.items()
                         if v["launches"]},
        "stats_by_kind": {str(k): v for k, v in stats.items()},
        "lightcone_counts": counts[0], "schedule_counts": counts[1],
    }


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--L", type=int, default=20)
    ap.add_argument("--tf", type=int, default=30)
    ap.add_argument("--traj", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--p_bond", type=float, default=0.01)
    ap.add_argument("--out", type=str, default="")
    args = ap.parse_args(argv)

    from __graft_entry__ import load_package

    pkg = load_package()
    with open(os.path.join(ROOT, "tests", "golden", "disorder.json")) as f:
        d = json.load(f)[f"L{args.L}"]
    base = dict(L=args.L, T=args.tf, hs=np.array(d["hs"][:1]), phis=np.array(d["phis"][:1]),
                g=0.97, noise_prob=0.05, use_noise=1, initial_state="vacuum")
    res = {"L": args.L, "tf": args.tf, "trajectories": args.traj, "steps": args.steps,
           "warmup": args.warmup, "p_bond": args.p_bond}
    # the switches are read when an engine opens
    os.environ["DTC_NO_LIGHTCONE"] = "1"
    os.environ["DTC_NO_DUAL"] = "1"
    res["plain"] = run(pkg, pkg.SweepSpec(**base), args.traj, args.steps, args.warmup)
    del os.environ["DTC_NO_LIGHTCONE"], os.environ["DTC_NO_DUAL"]
    res["bond"] = run(pkg, pkg.SweepSpec(**base, bond_noise=args.p_bond), args.traj, args.steps,
                      args.warmup)
    sb = res["bond"]["stats_by_kind"]
    build, lo = sb[str(pkg._capi.KERNEL_INIT)], sb[str(pkg._capi.KERNEL_LO_PASS)]
    fin = sb[str(pkg._capi.KERNEL_FINAL_PASS)]
    if build["launches"] and lo["launches"]:
        res["builder"] = {
            "launches": build["launches"],
            "ms_per_launch": build["total_ms"] / build["launches"],
            "diag_pass_ms_per_launch": lo["total_ms"] / lo["launches"],
            "time_share_of_a_diag_pass": (build["total_ms"] / build["launches"])
            / (lo["total_ms"] / lo["launches"]),
            "bytes_share_of_a_diag_pass": (build["bytes"] / build["launches"])
            / (lo["bytes"] / lo["launches"]),
            "measure_only_pass_launches": fin["launches"],
        }
    res["bond_over_plain"] = res["bond"]["value"] / res["plain"]["value"]
    txt = json.dumps(res, indent=1)
    print(txt)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(txt + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
