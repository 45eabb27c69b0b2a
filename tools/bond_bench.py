#!/usr/bin/env python3
"""Throughput of the bond-noise sweep (dtc_autocorr_bond) against the plain
schedule of dtc_autocorr, at the C2 shape (L=20, tf=30, p=0.05, vacuum,
tests/golden/disorder.json row 0).

    python tools/bond_bench.py [--config c2|c3|energy] [--traj 1024] [--steps 3] [--warmup 1]
                               [--p_bond 0.01] [--out F]

--config c2 (default): two engines, one after the other on device 0:
  plain  dtc_autocorr with DTC_NO_LIGHTCONE=1 DTC_NO_DUAL=1 (the schedule the
         bond runs are built from: no light-cone end, no dual pass),
  bond   dtc_autocorr_bond with p_bond on every bond.
Prints one JSON object: periods*instances/s of both (bench.py's unit), the
launch counts and times per kernel kind from kernel_stats, and the bond table
builder's share (time and bytes) of the diagonal pass it feeds.

--config c3: the C3 shape (device-like noise from data/device_standin_L20.json):
  plain  dtc_autocorr_device with DTC_NO_RUNAHEAD=1 (K-D forward passes, the
         schedule the device + bond runs are built from),
  bond   dtc_autocorr_bond with dv and the calibration's own two-qubit error
         (DeviceCalibration.bond_noise; --p_bond overrides it).
--config energy: bench.py's energy shape (L=20, tf=30, vacuum), for depolarizing
  (p=0.05) and device-like kicks: dtc_energy_sums against dtc_energy_sums_bond
  (p_bond as for c3), periods/s of both, and the sign kernel's time per launch
  -- it is counted with the reductions, so it is the difference of that kind's
  totals between the two runs over the launches added -- and as a share of a step.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def run(pkg, spec, B, steps, warmup, method="autocorr"):
    import torch

    eng = pkg.DtcEngine(0)
    try:
        call = getattr(eng, method)
        for i in range(warmup):
            call(spec, B, seed=0x5EED0001, traj_offset=i * B, batch=B)
        eng.reset_stats()
        eng.set_profiling(True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(steps):
            out = call(spec, B, seed=0x5EED0001, traj_offset=(warmup + i) * B, batch=B)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        eng.set_profiling(False)
        stats = eng.kernel_stats()
        counts = eng.lightcone_counts(), eng.schedule_counts()
    finally:
        eng.close()
    T = spec.T
    energy = method != "autocorr"
    per_traj = (T - 1) if energy else (T - 1) + sum(range(T))
    check = ({"x_sum_last_t": float(out["x"][0, -1].sum())} if energy
             else {"echo_mean_last_t": float(out["echo"][0, :, -1].mean())})
    return {
        "value": steps * B * per_traj / dt,
        "unit": "periods*trajectories/s" if energy else "periods*instances/s",
        "ms_per_step": dt / steps * 1e3,
        **check,
        "kernel_stats": {pkg._capi.KERNEL_NAMES[k].split()[0]: v for k, v in stats.items()
                         if v["launches"]},
        "stats_by_kind": {str(k): v for k, v in stats.items()},
        "lightcone_counts": counts[0], "schedule_counts": counts[1],
    }


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", choices=("c2", "c3", "energy"), default="c2")
    ap.add_argument("--L", type=int, default=20)
    ap.add_argument("--tf", type=int, default=30)
    ap.add_argument("--traj", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--p_bond", type=float, default=None,
                    help="default: 0.01 (c2), the calibration's bond noise (c3, energy)")
    ap.add_argument("--out", type=str, default="")
    args = ap.parse_args(argv)
    args.from_cal = args.p_bond is None and args.config != "c2"
    if args.p_bond is None:
        args.p_bond = 0.01

    from __graft_entry__ import load_package

    pkg = load_package()
    with open(os.path.join(ROOT, "tests", "golden", "disorder.json")) as f:
        d = json.load(f)[f"L{args.L}"]
    base = dict(L=args.L, T=args.tf, hs=np.array(d["hs"][:1]), phis=np.array(d["phis"][:1]),
                g=0.97, noise_prob=0.05, use_noise=1, initial_state="vacuum")
    res = {"config": args.config, "L": args.L, "tf": args.tf, "trajectories": args.traj,
           "steps": args.steps, "warmup": args.warmup, "p_bond": args.p_bond}
    if args.config != "c2":
        return finish(args, main_device(args, pkg, base, res))
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
    return finish(args, res)


def main_device(args, pkg, base, res):
    """--config c3 / energy (module docstring)."""
    cal = pkg.DeviceCalibration.from_json(os.path.join(ROOT, "data", "device_standin_L20.json"))
    dev = cal.device_noise(args.L)
    bond = cal.bond_noise(args.L) if args.from_cal else args.p_bond
    res["p_bond"] = float(np.max(bond))
    res["p_bond_source"] = "DeviceCalibration.bond_noise" if args.from_cal else "--p_bond"
    if args.config == "c3":
        os.environ["DTC_NO_RUNAHEAD"] = "1"
        res["plain"] = run(pkg, pkg.SweepSpec(**base, device=dev), args.traj, args.steps,
                           args.warmup)
        del os.environ["DTC_NO_RUNAHEAD"]
        res["bond"] = run(pkg, pkg.SweepSpec(**base, device=dev, bond_noise=bond), args.traj,
                          args.steps, args.warmup)
        res["bond_over_plain"] = res["bond"]["value"] / res["plain"]["value"]
        return res
    red = str(pkg._capi.KERNEL_REDUCE)
    for kicks, kw in (("depolarizing", {}), ("device", {"device": dev})):
        plain = run(pkg, pkg.SweepSpec(**base, **kw), args.traj, args.steps, args.warmup,
                    "energy_sums")
        with_b = run(pkg, pkg.SweepSpec(**base, **kw, bond_noise=bond), args.traj, args.steps,
                     args.warmup, "energy_sums_bond")
        a, b = plain["stats_by_kind"][red], with_b["stats_by_kind"][red]
        added = b["launches"] - a["launches"]
        sign_ms = (b["total_ms"] - a["total_ms"]) / added if added else float("nan")
        res[kicks] = {
            "plain": plain, "bond": with_b,
            "bond_over_plain": with_b["value"] / plain["value"],
            "sign_kernel": {"launches": added, "launches_per_step": added / args.steps,
                            "ms_per_launch": sign_ms,
                            "share_of_step": sign_ms * added / args.steps
                            / with_b["ms_per_step"]},
        }
    return res


def finish(args, res):
    txt = json.dumps(res, indent=1)
    print(txt)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(txt + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
