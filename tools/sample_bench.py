#!/usr/bin/env python3
"""Throughput of measurement sampling (dtc_sample, both bases, one shot per
trajectory) against the trajectory sums of exact expectations
(dtc_energy_sums), the fastest path to the same means, at the C2 shape (L=20,
tf=30, p=0.05, vacuum, tests/golden/disorder.json row 0, 1024 trajectories per
step).

    python tools/sample_bench.py [--steps 20] [--warmup 5] [--traj 1024] [--rounds 2]
                                 [--out profiles/sample_bench.json]

Two engines alternate on device 0, A B A B (--rounds pairs):
  A  sums     dtc_energy_sums: one K-D-K pass per site group and period, every
              pass measuring in flight;
  B  sample   dtc_sample: the forward in K-D passes (the state at t in memory
              exactly), the Z-basis weights and picks, one basis-change pass per
              site group, the X-basis weights and picks -- several passes per
              period by construction.
Both run tf - 1 forward periods per trajectory: the rate is
periods*trajectories/s.  Prints one JSON object: the rate and ms/step of every
run, launches and kernel time per step by profiling kind, and the sampling
launches' achieved rate.  The sampling launches are the only ones B books under
the reduce kind, weights and picks together, so
  sample_reduce_TBps   the reduce kind's booked bytes over its time, and
  weights_TBps_floor   the weights' 16 B per amplitude alone over that time (a
                       floor for dtc_sample_weights: the picks' time is in it).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def run(pkg, spec, B, steps, warmup, sample):
    import torch

    eng = pkg.DtcEngine(0)
    try:
        if sample:
            def call(off):
                return eng.sample(spec, B, n_shots=1, bases="zx", seed=0x5EED0001,
                                  traj_offset=off, batch=B)
        else:
            def call(off):
                return eng.energy_sums(spec, B, seed=0x5EED0001, traj_offset=off, batch=B)
        for i in range(warmup):
            call(i * B)
        eng.reset_stats()
        eng.set_profiling(True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(steps):
            out = call((warmup + i) * B)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        eng.set_profiling(False)
        stats = eng.kernel_stats()
    finally:
        eng.close()
    T, L = spec.T, spec.L
    j = spec.probe_site
    if sample:
        zj = 1.0 - 2.0 * ((out["z"][0, :, -1, 0] >> np.uint64(j)) & np.uint64(1)).astype(float)
        check = {"z_probe_mean_last_t": float(zj.mean())}
    else:
        check = {"z_probe_mean_last_t": float(out["z"][0, -1, j]) / B}
    res = {
        "value": steps * B * (T - 1) / dt,
        "unit": "periods*trajectories/s",
        "ms_per_step": dt / steps * 1e3,
        **check,
        "launches_per_step": {str(k): v["launches"] / steps for k, v in stats.items()},
        "kernel_ms_per_step": {str(k): v["total_ms"] / steps for k, v in stats.items()},
        "kernel_TBps": {str(k): v["bytes"] / max(v["total_ms"], 1e-9) * 1e-9 for k, v in stats.items()},
    }
    if sample:
        red = stats[pkg._capi.KERNEL_REDUCE]
        weights_bytes = 2.0 * (T - 1) * steps * 16.0 * (1 << max(L, 12)) * B
        res["sample_reduce_TBps"] = red["bytes"] / red["total_ms"] * 1e-9
        res["weights_TBps_floor"] = weights_bytes / red["total_ms"] * 1e-9
    return res


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--L", type=int, default=20)
    ap.add_argument("--tf", type=int, default=30)
    ap.add_argument("--traj", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2, help="A B pairs")
    ap.add_argument("--out", type=str, default="")
    args = ap.parse_args(argv)

    from __graft_entry__ import load_package

    pkg = load_package()
    with open(os.path.join(ROOT, "tests", "golden", "disorder.json")) as f:
        d = json.load(f)[f"L{args.L}"]
    spec = pkg.SweepSpec(L=args.L, T=args.tf, hs=np.array(d["hs"][:1]),
                         phis=np.array(d["phis"][:1]), g=0.97, noise_prob=0.05, use_noise=1,
                         initial_state="vacuum")
    res = {"L": args.L, "tf": args.tf, "trajectories": args.traj, "steps": args.steps,
           "warmup": args.warmup, "periods_per_trajectory": args.tf - 1,
           "kinds": {str(k): v.split()[0] for k, v in pkg._capi.KERNEL_NAMES.items()},
           "sums": [], "sample": []}
    for _ in range(args.rounds):
        res["sums"].append(run(pkg, spec, args.traj, args.steps, args.warmup, False))
        res["sample"].append(run(pkg, spec, args.traj, args.steps, args.warmup, True))

    def mean(runs, get):
        return float(np.mean([get(r) for r in runs]))

    a = mean(res["sums"], lambda r: r["value"])
    b = mean(res["sample"], lambda r: r["value"])
    res["summary"] = {
        "sums_rate": a, "sample_rate": b, "sample_over_sums": b / a,
        "sums_rate_spread": [min(r["value"] for r in res["sums"]),
                             max(r["value"] for r in res["sums"])],
        "sample_rate_spread": [min(r["value"] for r in res["sample"]),
                               max(r["value"] for r in res["sample"])],
        "sample_reduce_TBps": mean(res["sample"], lambda r: r["sample_reduce_TBps"]),
        "weights_TBps_floor": mean(res["sample"], lambda r: r["weights_TBps_floor"]),
    }
    txt = json.dumps(res, indent=1)
    print(txt)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(txt + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
