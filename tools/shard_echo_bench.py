#!/usr/bin/env python3
"""Forward and inverse period times of the sharded single-state sweep on one
GPU (virtual ranks, in place): sharded_autocorr_pipelined at L = 30, k = 3,
T = 6 by default, with (A, E) buffers and every echo chain, beside two runs of
sharded_forward_pipelined at the same shape (the forward yardstick and its
run-to-run spread).  An inverse period runs a forward period's passes and moves
the same bytes, so ``echo_period_ms`` is expected at ``period_ms``.

    python tools/shard_echo_bench.py --steps 3 --warmup 1 [--out profiles/x.json]

Prints one JSON line (medians over every period of every step, ms)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from __graft_entry__ import load_package  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--L", type=int, default=30)
    ap.add_argument("--k", type=int, default=3, help="rank bits (2^k virtual ranks)")
    ap.add_argument("--T", type=int, default=6)
    ap.add_argument("--noise_prob", type=float, default=0.05)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--fuse", type=int, default=1, help="fused kick+exchange (the default path)")
    ap.add_argument("--out", type=str, default="")
    args = ap.parse_args(argv)
    pkg = load_package()
    sh = pkg.sharded
    L, k, T = args.L, args.k, args.T
    hs, phis = pkg.load_disorder(34, 1, os.path.join(ROOT, "data"))
    spec = pkg.SweepSpec(L=L, T=T, hs=hs[:, :L], phis=phis[:, :L - 1], g=0.97,
                         noise_prob=args.noise_prob, use_noise=int(args.noise_prob > 0))
    eng = pkg.DtcEngine(0)
    stepper = sh.EngineStepper(eng)
    A, E = stepper.alloc(sh.initial_layout(L, k, 0, 1 << k), 2)
    kw = dict(inplace=True, fuse_kick_exchange=bool(args.fuse), seed=77)

    def forward(out):
        st = {}
        sh.sharded_forward_pipelined(stepper, spec, k, buffers=(A,), stats=st, **kw)
        out += st["period_ms"]

    def autocorr(fwd_out, echo_out):
        st = {}
        r = sh.sharded_autocorr_pipelined(stepper, spec, k, buffers=(A, E), stats=st, **kw)
        fwd_out += st["period_ms"]
        echo_out += st["echo_period_ms"]
        return r

    for _ in range(args.warmup):
        forward([])
        autocorr([], [])
    f1, f2, fa, ea = [], [], [], []
    r = None
    for _ in range(args.steps):
        forward(f1)
        r = autocorr(fa, ea)
        forward(f2)
    med = statistics.median
    # the first forward period also kicks the top group (one more whole pass):
    # the medians are over every period
    res = {
        "tool": "shard_echo_bench", "L": L, "k": k, "T": T, "noise_prob": args.noise_prob,
        "steps": args.steps, "fused_kick_exchange": bool(args.fuse),
        "forward_period_ms_run1": med(f1), "forward_period_ms_run2": med(f2),
        "forward_spread_ms": abs(med(f1) - med(f2)),
        "period_ms": med(fa), "echo_period_ms": med(ea),
        "echo_over_forward": med(ea) / med(fa),
        "n_forward_periods": len(fa), "n_inverse_periods": len(ea),
        "echo_last": float(r["echo"][-1]), "fwd_last": float(r["fwd"][-1]),
    }
    # L = 34 on one GPU holds one chain (t = T - 1, buffers (A,)): p forward and
    # p inverse periods; estimated from the measured rates by the state's size
    scale = float(1 << (34 - L))
    res["l34_estimate_unmeasured_s_per_period_pair"] = scale * (med(fa) + med(ea)) / 1e3
    eng.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
