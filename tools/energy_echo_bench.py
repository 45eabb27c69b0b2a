#!/usr/bin/env python3
"""Throughput of the energy echo (dtc_energy_echo_sums) against the same echo
chains read for the probe only, at the C2 shape (L=20, tf=30, p=0.05, vacuum,
tests/golden/disorder.json row 0, 1024 trajectories per step).

    python tools/energy_echo_bench.py [--steps 20] [--warmup 5] [--traj 1024] [--rounds 2]
                                      [--out profiles/energy_echo_bench.json]

Two engines alternate on device 0, A B A B (--rounds pairs):
  A  probe   dtc_autocorr, echo only (want_fwd = 0), opened with
             DTC_NO_LIGHTCONE=1: the same chains -- dual-pass start, wavefront
             interior -- each ending in its last K-D-K (measure-only, the
             probe), the trailing kick-only pass dropped;
  B  energy  dtc_energy_echo_sums: every chain's last K-D-K stored and
             measuring X of its group, then the trailing kick-only pass
             (measure-only: X of its group, norm, Z, ZZ of all sites).
Both run 29 forward and 435 inverse periods per trajectory: the rate is
periods*trajectories/s over 464 periods.  Prints one JSON object: the rate and
ms/step of every run, launches per step by profiling kind, the wavefront and
folded counts, the average time and bytes of the measure-only passes, and the
per-step gap B - A (kernel time, HIP events) split into
  trailing   B's 29 measure-only kick passes,
  ends       B's 29 stored, X-measuring K-D-K ends against A's 29 measure-only
             probe K-D-K ends (the difference of the stored-pass totals, which
             are otherwise the same launches, less A's measure-only total),
  reduce     B's 58 reductions of 3 L / L columns against A's 29 of 2,
and what is left of the wall-clock gap beside them (launch gaps, B's
per-instance trajectory sum, the read-back).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def run(pkg, spec, B, steps, warmup, energy):
    import torch

    eng = pkg.DtcEngine(0)
    try:
        if energy:
            def call(off):
                return eng.energy_echo_sums(spec, B, seed=0x5EED0001, traj_offset=off, batch=B)
        else:
            def call(off):
                return eng.autocorr(spec, B, seed=0x5EED0001, traj_offset=off, batch=B,
                                    want_fwd=False)
        for i in range(warmup):
            call(i * B)
        eng.reset_stats()
        wf0, folded0 = eng.wavefront_count(), eng.schedule_counts()["folded"]
        eng.set_profiling(True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(steps):
            out = call((warmup + i) * B)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        eng.set_profiling(False)
        stats = eng.kernel_stats()
        wf = eng.wavefront_count() - wf0
        folded = eng.schedule_counts()["folded"] - folded0
        lc = eng.lightcone_counts()
    finally:
        eng.close()
    T = spec.T
    per_traj = (T - 1) + sum(range(T))
    fin = stats[pkg._capi.KERNEL_FINAL_PASS]
    check = ({"z_probe_mean_last_t": float(out["z"][0, -1, spec.probe_site]) / B} if energy
             else {"echo_mean_last_t": float(out["echo"][0, :, -1].mean())})
    return {
        "value": steps * B * per_traj / dt,
        "unit": "periods*trajectories/s",
        "ms_per_step": dt / steps * 1e3,
        **check,
        "launches_per_step": {str(k): v["launches"] / steps for k, v in stats.items()},
        "kernel_ms_per_step": {str(k): v["total_ms"] / steps for k, v in stats.items()},
        "wavefront_per_step": wf / steps,
        "folded_per_step": folded / steps,
        "lightcone_counts": lc,
        "measure_only_pass": {
            "launches_per_step": fin["launches"] / steps,
            "ms_per_launch": fin["total_ms"] / max(fin["launches"], 1),
            "bytes_per_launch": fin["bytes"] / max(fin["launches"], 1),
        },
    }


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
           "warmup": args.warmup, "periods_per_trajectory": (args.tf - 1) + sum(range(args.tf)),
           "kinds": {str(k): v.split()[0] for k, v in pkg._capi.KERNEL_NAMES.items()},
           "probe": [], "energy": []}
    for _ in range(args.rounds):
        # the switch is read when an engine opens
        os.environ["DTC_NO_LIGHTCONE"] = "1"
        res["probe"].append(run(pkg, spec, args.traj, args.steps, args.warmup, False))
        del os.environ["DTC_NO_LIGHTCONE"]
        res["energy"].append(run(pkg, spec, args.traj, args.steps, args.warmup, True))

    def mean(runs, get):
        return float(np.mean([get(r) for r in runs]))

    a = mean(res["probe"], lambda r: r["value"])
    b = mean(res["energy"], lambda r: r["value"])
    K = pkg._capi
    kms = {side: {k: mean(res[side], lambda r, k=k: r["kernel_ms_per_step"][str(k)])
                  for k in range(K.KERNEL_KINDS)} for side in ("probe", "energy")}
    stored = lambda s: kms[s][K.KERNEL_LO_PASS] + kms[s][K.KERNEL_HI_PASS]  # noqa: E731
    gap_wall = (mean(res["energy"], lambda r: r["ms_per_step"])
                - mean(res["probe"], lambda r: r["ms_per_step"]))
    split = {
        "trailing": kms["energy"][K.KERNEL_FINAL_PASS],
        "ends": stored("energy") - stored("probe") - kms["probe"][K.KERNEL_FINAL_PASS],
        "reduce": kms["energy"][K.KERNEL_REDUCE] - kms["probe"][K.KERNEL_REDUCE],
    }
    res["summary"] = {
        "probe_rate": a, "energy_rate": b, "energy_over_probe": b / a,
        "probe_rate_spread": [min(r["value"] for r in res["probe"]),
                              max(r["value"] for r in res["probe"])],
        "energy_rate_spread": [min(r["value"] for r in res["energy"]),
                               max(r["value"] for r in res["energy"])],
        "gap_ms_per_step_wall": gap_wall,
        "gap_split_ms_per_step": split,
        "gap_unexplained_ms_per_step": gap_wall - sum(split.values()),
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
