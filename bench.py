#!/usr/bin/env python3
"""Benchmark: the DTC autocorrelator sweep at L=20 (BASELINE.json configs[1]).

Workload (one "step"): a batch of B noisy trajectories of disorder instance 0
(hs_L20.csv / phis_L20.csv row 0, g=0.97, depolarizing p=0.05, vacuum state,
probe site j=10) through the full forward + echo sweep over t = 0..29
(autocorr-delta-a-single-qiskit-fast.py with --L 20 --tf 30).  Each
trajectory applies 29 forward periods and sum_{t<30} t = 435 inverse periods
(echo branches), i.e. 464 Floquet-period applications to a 2^20 complex128
state.  The metric counts those period applications per second over all
ranks ("Floquet-periods x instances / s").

Multi-GPU: one process per GPU.  `--gpus N` spawns the N rank processes
itself when no launcher set WORLD_SIZE (torchrun works too; a WORLD_SIZE that
differs from --gpus is refused).  By default a step is 1024 trajectories split
evenly over the ranks (strong scaling, the north_star's 1 -> 8 GPU target;
--strong-total 0 --batch B gives weak scaling).  Trajectories are independent
units with counter-based RNG keyed by the global trajectory id, so there is no
data-path collective: the per-t sums are all-reduced once at the end over
RCCL.

Prints ONE JSON line on rank 0 (contract in the task statement), with
"roofline" for the K-D-K pass kernel (kick . RZZ/RZ diagonal . kick; HIP
events on the engine's stream over the timed region, all passes that apply
the diagonal; every rank's rate in per_rank_GBps).  A plain run does only
that: set up, warm up, time the steps, print the line.

`--full` adds the measurements that take runs of their own, after the timed
region (they never change the line's own numbers): "cpu_baseline" = the
period-fused CPU restatement (oracle/dtc_oracle.c orc_autocorr_fused) on this
host's usable cores for a bounded sample, with the CPU model, and at 8 ranks
"c5": the C5 configuration (one L=34 state over the 8 GPUs) measured by a
nested 8-rank job (run_child_ranks), or its error.

`--dump-outputs DIR` writes what the last timed step returned to its caller
(c2/c3: fwd and echo per trajectory) as DIR/<name>.npy, float64; the inputs
depend only on the arguments, so two builds can be compared array by array.
"""
from __future__ import annotations

import argparse
import glob
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
PKG = "noise-resilience-in-discrete-time-crystal-realizations-on-quantum-computers_amd"

import numpy as np  # noqa: E402

HBM_PEAK_GBS = 8000.0        # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec
HBM_MEASURED_GBS = 6290.0    # the guide's measured float4 copy (same table)
# The best read+write stream measured on this part (tools/hbm_ceiling2.hip,
# profiles/r3b_hbm_ceiling2.txt): an in-place sweep with ONE 16-B amplitude per
# lane and nontemporal loads/stores, 6.59 TB/s (copy 6.53).  The same sweep with
# 4 / 16 amplitudes per lane (16 / 64 KiB per workgroup, the pass kernels' tile)
# reaches 5.66 / 5.4 TB/s (r3b, r2d).
BEST_RW_STREAM_GBS = 6586.0
METRIC = "Floquet-periods×instances/sec at L=20; RZZ-kernel HBM GB/s vs peak"


def load_disorder_row(L):
    with open(os.path.join(ROOT, "tests", "golden", "disorder.json")) as f:
        d = json.load(f)[f"L{L}"]
    return np.array(d["hs"][:1]), np.array(d["phis"][:1])


def load_disorder_rows(pkg, L, lo, hi):
    """Rows [lo, hi) of data/hs_L{L}.csv (tools/make_large_disorder.py)."""
    hs, phis = pkg.load_disorder(L, hi, os.path.join(ROOT, "data"))
    return hs[lo:hi], phis[lo:hi]


def periods_per_traj(T, t_offset=0):
    P = T - 1 + t_offset
    echo = sum(t + t_offset for t in range(T))
    return P + echo


DUMP_MAX_BYTES = 60_000_000   # all files of one run together (64 MB less headers and slack)


def dump_outputs(path, arrays, rank=0, world=1):
    """--dump-outputs: the arrays the last timed step returned, as
    <path>/<name>.npy (rank r of a multi-rank run: <name>_rank<r>.npy), float64.
    All ranks' files together stay under DUMP_MAX_BYTES: when a rank's share
    would not, each array is cut to a fixed, seeded sample of its flattened
    elements (sorted indices, the same from run to run)."""
    if not path:
        return
    os.makedirs(path, exist_ok=True)
    arrays = {k: np.ascontiguousarray(v, dtype=np.float64) for k, v in arrays.items()}
    total = sum(a.nbytes for a in arrays.values())
    budget = DUMP_MAX_BYTES // world
    for name, a in sorted(arrays.items()):
        if total > budget:
            keep = max(1, int(a.size * (budget / total)))
            idx = np.sort(np.random.default_rng(0xD0C5).choice(a.size, keep, replace=False))
            a = a.reshape(-1)[idx]
        suffix = f"_rank{rank}" if world > 1 else ""
        np.save(os.path.join(path, f"{name}{suffix}.npy"), a)


def cpu_baseline(spec, n_traj, T_sample, threads=None, t_offset=0):
    """Time the period-fused CPU restatement (oracle/dtc_oracle.c:
    orc_autocorr_fused: the same trajectories as the engine, per-site noisy
    kicks composed once per period, cache-blocked low/high sweeps, split
    re/im arrays, OpenMP over trajectories) on this host's usable cores."""
    from oracle import c_oracle

    info = host_cpu_info()
    threads = threads or info["usable_cores"]
    pkg = importlib.import_module(PKG)
    s = pkg.SweepSpec(L=spec.L, T=T_sample, hs=spec.hs, phis=spec.phis, g=spec.g,
                      noise_prob=spec.noise_prob, use_noise=spec.use_noise, t_offset=t_offset)
    t0 = time.perf_counter()
    c_oracle.autocorr_fused(s, n_traj, seed=0xC0FFEE, n_threads=threads)
    dt = time.perf_counter() - t0
    work = n_traj * periods_per_traj(T_sample, t_offset)
    return {
        "value": work / dt,
        "unit": "periods*instances/s",
        "cores": threads,
        "cpu_model": info["cpu_model"],
        "host_cpus_in_affinity": info["affinity_cpus"],
        "cgroup_cpu_quota": info["cgroup_cpu_quota"],
        "kind": "port",
        "sample": (f"period-fused CPU restatement (oracle/dtc_oracle.c orc_autocorr_fused, "
                   f"OpenMP over trajectories, {threads} threads): L={spec.L}, g={spec.g}, "
                   f"p={spec.noise_prob}, {n_traj} trajectories x T={T_sample} fwd+echo = "
                   f"{work} period applications in {dt:.1f} s"),
    }


def read_traffic(bytes_per_launch, suffix="_pmc.json", batch=None):
    """HBM bytes per launch of the RZZ kernel from the latest committed PMC
    summary named *<suffix> (tools/pmc_summary.py output: rocprofv3 FETCH_SIZE
    and WRITE_SIZE passes of this same bench config), or (None, None).  With
    ``batch``, only a summary taken at that batch counts (no rescaling)."""
    import re

    def tag_order(path):
        # profile tags run r1a .. r1z, r2a .. r2z, r2aa, r2ab, ...: (round, length, letters)
        m = re.match(r"r(\d+)([a-z]+)_", os.path.basename(path))
        return (int(m.group(1)), len(m.group(2)), m.group(2)) if m else (-1, 0, path)

    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "*" + suffix)), key=tag_order)
    d = None
    for path in reversed(files):
        with open(path) as f:
            cand = json.load(f)
        if batch is None or cand.get("batch") == batch:
            d = cand
            files = [path]
            break
    if d is None:
        return None, None
    k = d.get("lo_pass")
    if not k or not k.get("hbm_bytes_per_launch"):
        return None, None
    # scale to this run's launch size
    scale = bytes_per_launch / k["algorithmic_bytes_per_launch"]
    return k["hbm_bytes_per_launch"] * scale, os.path.relpath(files[-1], ROOT)


def _free_port() -> int:
    import socket

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def spawn_ranks(n: int, argv) -> int:
    """``bench.py --gpus N`` without an external launcher: start N rank
    processes of this script (RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* set,
    rendezvous on 127.0.0.1) and wait for them.  Runs before anything touches
    the GPU (this process never initialises HIP; the ranks are children, not
    an exec).  Only rank 0 prints the JSON line.  If a rank fails, the others
    are terminated (they would wait forever at the next collective).  Returns
    the first non-zero exit code, or 0."""
    import subprocess

    port = _free_port()
    base = dict(os.environ)
    base.update({"MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port), "WORLD_SIZE": str(n),
                 "LOCAL_WORLD_SIZE": str(n), "GROUP_RANK": "0", "ROLE_RANK": "0"})
    base.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # dmabuf IPC for RCCL on this host
    procs = []
    for r in range(n):
        env = dict(base, RANK=str(r), LOCAL_RANK=str(r))
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + list(argv),
                                      env=env))
    rc = 0
    alive = list(procs)
    while alive:
        for p in list(alive):
            code = p.poll()
            if code is None:
                continue
            alive.remove(p)
            if code != 0 and rc == 0:
                rc = code if code > 0 else 128 - code
                for q in alive:
                    q.terminate()
        if alive:
            time.sleep(0.05)
    for p in procs:
        p.wait()
    return rc


def _child_env(port: int, rank: int, local_rank: int, world: int) -> dict:
    """Environment of a rank of a nested job: its own rendezvous on 127.0.0.1.
    torchrun's agent variables are dropped (TORCHELASTIC_USE_AGENT_STORE would
    make the child connect to the agent's store instead of hosting its own)."""
    env = {k: v for k, v in os.environ.items()
           if not k.startswith(("TORCHELASTIC_", "TORCH_ELASTIC_"))}
    env.update({"MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port), "WORLD_SIZE": str(world),
                "RANK": str(rank), "LOCAL_RANK": str(local_rank),
                "LOCAL_WORLD_SIZE": str(world), "GROUP_RANK": "0", "ROLE_RANK": str(rank)})
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    return env


def run_child_ranks(child_argv, dist, rank: int, local_rank: int, world: int,
                    timeout_s: float, coll_dev: str = "cpu"):
    """Run a second N-rank job of this script from inside a running one: every
    rank starts one child (a subprocess, never an exec), the children
    rendezvous on a port rank 0 picked and broadcast over ``dist``, and the
    parents wait for them at most ``timeout_s`` (a child still running then is
    killed with its process group).  A failure of the nested job can therefore
    not hang or end the outer one.  Returns rank 0's parsed JSON line, or
    {"error": ...}; other ranks return None."""
    import signal
    import subprocess

    import torch

    port = torch.tensor([_free_port() if rank == 0 else 0], dtype=torch.int64, device=coll_dev)
    if dist:
        dist.broadcast(port, 0)
    env = _child_env(int(port.item()), rank, local_rank, world)
    t0 = time.perf_counter()
    p = subprocess.Popen([sys.executable, os.path.abspath(__file__)] + list(child_argv), env=env,
                         stdout=subprocess.PIPE if rank == 0 else subprocess.DEVNULL,
                         text=True, start_new_session=True)
    status = "ok"
    try:
        out, _ = p.communicate(timeout=timeout_s)
    except subprocess.TimeoutExpired:
        os.killpg(p.pid, signal.SIGKILL)
        out, _ = p.communicate()
        status = f"timeout after {timeout_s:.0f} s"
    ok = torch.tensor([1.0 if (status == "ok" and p.returncode == 0) else 0.0],
                      dtype=torch.float64, device=coll_dev)
    if dist:
        dist.all_reduce(ok, op=dist.ReduceOp.MIN)
    if rank != 0:
        return None
    wall = time.perf_counter() - t0
    if status != "ok" or p.returncode != 0 or float(ok.item()) < 1.0:
        return {"error": status if status != "ok" else
                f"a rank of the nested job failed (rank 0 exit code {p.returncode})",
                "wall_s": wall}
    lines = [ln for ln in (out or "").splitlines() if ln.strip().startswith("{")]
    if not lines:
        return {"error": "no JSON line from the nested job", "wall_s": wall}
    d = json.loads(lines[-1])
    d["wall_s"] = wall
    return d


def spawn_selftest(args) -> int:
    """Rank-side half of the spawn check (tests/test_bench_spawn.py): every
    rank joins a gloo group, the world size and the ranks are all-reduced,
    rank 0 prints one JSON line shaped like the bench line.  No GPU work."""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    if os.environ.get("BENCH_SELFTEST_FAIL_RANK") == str(rank):
        return 3  # test hook: this rank dies before the rendezvous
    import torch
    import torch.distributed as dist

    if world > 1:
        dist.init_process_group("gloo")
    t = torch.tensor([1.0, float(rank)])
    if world > 1:
        dist.all_reduce(t)
        dist.barrier()
    nested = None
    if args.selftest_nested and world > 1:
        # the C5 sub-run's plumbing (run_child_ranks) with a selftest as the child
        local_rank = int(os.environ.get("LOCAL_RANK", "0"))
        fail = os.environ.get("BENCH_SELFTEST_NESTED_HANG_RANK")
        child = ["--gpus", str(world), "--spawn-selftest"]
        env_hang = fail is not None and fail == str(rank)
        if env_hang:
            os.environ["BENCH_SELFTEST_HANG"] = "1"
        nested = run_child_ranks(child, dist, rank, local_rank, world,
                                 timeout_s=args.nested_timeout)
        os.environ.pop("BENCH_SELFTEST_HANG", None)
    if os.environ.get("BENCH_SELFTEST_HANG") == "1":
        time.sleep(3600)  # test hook: a nested rank that never finishes
    if rank == 0:
        B = args.strong_total // world if args.strong_total else (args.batch or 256)
        d = {"metric": "spawn-selftest", "value": float(t[0]), "n_gpus": world,
             "rank_sum": float(t[1]), "scaling": "strong" if args.strong_total else "weak",
             "trajectories_per_step_per_gpu": B}
        if nested is not None:
            d["nested"] = nested
        print(json.dumps(d), flush=True)
    if world > 1:
        dist.destroy_process_group()
    return 0


def _device_and_backend(local_rank, world):
    """GPU of this rank and the process-group backend.  Normal runs: GPU
    local_rank, RCCL ("nccl").  BENCH_SHARE_DEVICE=1 (plumbing test on a 1-GPU
    box, tests/test_gpu_bench_spawn.py): every rank on GPU 0 with the backend
    BENCH_DIST_BACKEND (gloo: RCCL refuses two ranks on one GPU); the numbers
    of such a run say nothing about scaling."""
    share = os.environ.get("BENCH_SHARE_DEVICE") == "1"
    dev = 0 if (share or world == 1) else local_rank
    backend = os.environ.get("BENCH_DIST_BACKEND", "gloo" if share else "nccl")
    return dev, backend


def _coll_dev(backend):
    """Where the (few-KB) collective buffers live: the GPU for RCCL, host for gloo."""
    return "cuda" if backend == "nccl" else "cpu"


def host_cpu_info() -> dict:
    """CPU model and the cores this process may use: the affinity set, capped
    by a cgroup CPU quota when one is set (a GPU box's share of its host)."""
    model = "unknown"
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name"):
                    model = line.split(":", 1)[1].strip()
                    break
    except OSError:
        pass
    try:
        affinity = len(os.sched_getaffinity(0))
    except AttributeError:
        affinity = os.cpu_count() or 1
    quota = None
    try:
        with open("/sys/fs/cgroup/cpu.max") as f:
            q, per = f.read().split()[:2]
            if q != "max":
                quota = float(q) / float(per)
    except (OSError, ValueError):
        pass
    usable = affinity if quota is None else max(1, min(affinity, int(quota + 0.5)))
    return {"cpu_model": model, "affinity_cpus": affinity, "cgroup_cpu_quota": quota,
            "usable_cores": usable}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--batch", type=int, default=0,
                    help="trajectories per step per GPU when --strong-total is 0 (weak scaling); "
                         "0 = the config's default (c2: 256, c3 and energy: 1024)")
    ap.add_argument("--strong-total", type=int, default=1024,
                    help="c2/c3: trajectories per step over ALL ranks, split evenly (strong "
                         "scaling, the north_star's 1 -> 8 GPU target; default 1024); 0 = weak "
                         "scaling with --batch per GPU")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps also run what takes a run of its own: the CPU "
                         "baseline (c2, energy, ctrl; --no-cpu-baseline still drops it) and, at "
                         "8 GPUs, the C5 sub-run attached to the c2 line")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the arrays the last timed step returned as DIR/<name>.npy "
                         "(float64; ranks of a multi-GPU run add _rank<r>)")
    ap.add_argument("--spawn-selftest", action="store_true",
                    help="CPU-only check of the rank spawn path (gloo, no GPU work)")
    ap.add_argument("--selftest-nested", action="store_true",
                    help="with --spawn-selftest: also run a nested selftest job through "
                         "run_child_ranks (the C5 sub-run's plumbing)")
    ap.add_argument("--nested-timeout", type=float, default=240.0,
                    help="seconds a nested job (the C5 sub-run) may take before it is killed")
    ap.add_argument("--no-c5-subrun", action="store_true",
                    help="c2 at 8 GPUs with --full: skip the C5 (L=34 over 8 GPUs) sub-run that "
                         "is attached to the line as \"c5\"")
    ap.add_argument("--L", type=int, default=20)
    ap.add_argument("--tf", type=int, default=30)
    ap.add_argument("--no-cpu-baseline", action="store_true",
                    help="with --full: skip the CPU baseline (a plain run never takes it)")
    ap.add_argument("--cpu-traj", type=int, default=0,
                    help="0 = three per host thread at c2 (about 12 s on the GPU box's 16 "
                         "cores at T=30)")
    ap.add_argument("--cpu-tf", type=int, default=0,
                    help="time points of the CPU sample; 0 = the line's own tf (c2: T=30, "
                         "the headline config; ctrl: 20; energy: 6)")
    ap.add_argument("--config", choices=("c2", "c3", "c4", "c5", "energy", "ctrl"), default="c2",
                    help="c2: BASELINE configs[1] (default, the headline line); c3: L=20 "
                         "device-like noise (stand-in calibration, data/"
                         "device_standin_L20.json), 1024 trajectories per step; c4: L=28 "
                         "noiseless disorder sweep, instances sharded over ranks; c5: one "
                         "L=34 state sharded over the ranks (1 GPU: L=34 as 8 virtual ranks "
                         "with the in-place exchange; --L 31 or less: the two-buffer form); "
                         "energy: the energy observable path (§8(f)1); ctrl: the real-time "
                         "adaptive-g controller loop (§8(f)2)")
    ap.add_argument("--ctrl-tf", type=int, default=20, help="ctrl: time points of the loop")
    ap.add_argument("--ctrl-opt", action="store_true",
                    help="ctrl: the optimisation controller (g-optimization.py) instead of "
                         "the feedback rule; value = controller time points per second")
    ap.add_argument("--no-prefix-cache", action="store_true",
                    help="ctrl --ctrl-opt: a full t+1-period run per candidate evaluation")
    ap.add_argument("--shard-bits", type=int, default=3, help="c5: log2 of the shard count")
    ap.add_argument("--instances", type=int, default=32, help="c4: instances per step per GPU")
    args = ap.parse_args(argv)
    env_world = os.environ.get("WORLD_SIZE")
    if env_world is None and args.gpus > 1:
        # no launcher: this process spawns the ranks (before any GPU call)
        return spawn_ranks(args.gpus, sys.argv[1:] if argv is None else argv)
    if env_world is not None and int(env_world) != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={env_world}: refusing to report a "
                         "different GPU count than requested")
    if args.spawn_selftest:
        return spawn_selftest(args)
    if args.config == "c4":
        return main_c4(args)
    if args.config == "c5":
        return main_c5(args)
    if args.config == "energy":
        return main_energy(args)
    if args.config == "ctrl":
        return main_ctrl(args)

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))

    import torch

    dist = None
    dev, backend = _device_and_backend(local_rank, world)
    cdev = _coll_dev(backend)
    torch.cuda.set_device(dev)
    if world > 1:
        import torch.distributed as dist

        dist.init_process_group(backend)

    pkg = importlib.import_module(PKG)
    hs, phis = load_disorder_row(args.L)
    spec = pkg.SweepSpec(L=args.L, T=args.tf, hs=hs, phis=phis, g=0.97, noise_prob=0.05,
                         use_noise=1, initial_state="vacuum")
    c3 = args.config == "c3"
    if c3:  # device-like noise, throughput only (parity unpinned)
        cal = pkg.DeviceCalibration.from_json(os.path.join(ROOT, "data",
                                                           "device_standin_L20.json"))
        spec.device = cal.device_noise(args.L)
    if not args.batch:
        args.batch = 1024 if c3 else 256
    eng = pkg.DtcEngine(dev)
    B = args.batch
    if args.strong_total:
        # SURVEY.md §8(d) scaling report (north_star: >= 6x strong scaling 1 -> 8
        # GPUs): the same total trajectory count whatever the rank count
        if args.strong_total % world:
            raise SystemExit(f"--strong-total {args.strong_total} is not a multiple of {world} ranks")
        B = args.strong_total // world
    T = args.tf
    per_traj = periods_per_traj(T)
    sums = np.zeros((2, T))
    last = {}  # the latest step's outputs (--dump-outputs)

    def step(i):
        off = (rank * (args.warmup + args.steps) + i) * B
        out = eng.autocorr(spec, B, seed=0x5EED0001, traj_offset=off, batch=B)
        sums[0] += out["fwd"][0].sum(axis=0)
        sums[1] += out["echo"][0].sum(axis=0)
        last.update(out)

    for i in range(args.warmup):
        step(i)
    sums[:] = 0
    eng.reset_stats()
    eng.set_profiling(True)

    if dist:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(args.steps):
        step(args.warmup + i)
    acc = torch.from_numpy(sums).to(cdev)
    if dist:
        dist.all_reduce(acc)  # RCCL over xGMI: the only collective (final autocorr gather)
    torch.cuda.synchronize()
    if dist:
        dist.barrier()
    elapsed = time.perf_counter() - t0
    eng.set_profiling(False)
    stats = eng.kernel_stats()

    el = torch.tensor([elapsed], dtype=torch.float64, device=cdev)
    if dist:
        dist.all_reduce(el, op=dist.ReduceOp.MAX)
    elapsed = float(el.item())
    autocorr = (acc.cpu().numpy() / (world * args.steps * B))
    # every rank's K-D-K pass rate (the north_star's per-GPU roofline at N GPUs)
    my = torch.tensor([stats[0]["total_ms"], float(stats[0]["launches"]), elapsed],
                      dtype=torch.float64, device=cdev)
    per_rank = [my]
    if dist:
        per_rank = [torch.zeros_like(my) for _ in range(world)]
        dist.all_gather(per_rank, my)
    per_rank = [r.cpu().numpy() for r in per_rank]

    total_units = world * args.steps * B * per_traj
    value = total_units / elapsed
    lo = stats[0]
    hi = stats[1]
    # algorithmic bytes per launch as the engine booked them (32 B per amplitude
    # for a read+store pass; 16 B for the first pass, which forms the basis
    # states in registers and only stores, and for the measure-only passes)
    launch_bytes = lo["bytes"] / max(1, lo["launches"])
    hi_bytes = hi["bytes"] / max(1, hi["launches"])
    avg_lo = lo["total_ms"] / max(1, lo["launches"]) / 1e3
    avg_hi = hi["total_ms"] / max(1, hi["launches"]) / 1e3
    achieved = launch_bytes / avg_lo / 1e9 if lo["launches"] else 0.0
    traffic, traffic_src = read_traffic(launch_bytes, "_pmc_c3.json" if c3 else "_pmc.json",
                                        batch=B)
    # what the engine executed (the value credits whole period applications;
    # the schedule runs fewer, larger passes: K-D-K passes that each advance a
    # period, light-cone passes that replace the last 2-4 of an echo chain)
    n_launch = {k: stats[k]["launches"] / args.steps for k in (0, 1, 4)}
    state_passes = sum(stats[k]["launches"] for k in (0, 1, 4)) * B
    hbm_bytes_kernels = sum(stats[k]["bytes"] for k in (0, 1, 4, 5))

    dump_outputs(args.dump_outputs, last, rank, world)

    cpu = None
    if args.full and rank == 0 and world == 1 and not args.no_cpu_baseline and not c3:
        threads = host_cpu_info()["usable_cores"]
        cpu = cpu_baseline(spec, args.cpu_traj or 3 * threads, args.cpu_tf or spec.T, threads)

    info = eng.device_info()
    c5 = None
    force_c5 = os.environ.get("BENCH_C5_SUBRUN") == "1"  # plumbing check on a 1-GPU box
    if (args.full and (world == 8 or force_c5) and args.config == "c2"
            and not args.no_c5_subrun):
        # SURVEY.md §8(d) C5 (one L=34 state over the 8 GPUs) as a nested 8-rank
        # job after the timed C2 region, so the node's 8-GPU run also measures
        # it; its failure or hang cannot touch the C2 line (run_child_ranks).
        # Forced at other rank counts it runs the same driver as --config c5
        # there (1 GPU: 8 virtual shards of L=31)
        eng.close()
        torch.cuda.empty_cache()
        c5 = run_child_ranks(["--config", "c5", "--gpus", str(world), "--steps", "1",
                              "--warmup", "1"],
                             dist, rank, local_rank, world, args.nested_timeout, cdev)
    if rank != 0:
        if dist:
            dist.destroy_process_group()
        return
    res = {
        "metric": METRIC if not c3 else METRIC.replace("at L=20", "at L=20 (C3 device-like noise)"),
        "value": value,
        "unit": "periods*instances/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": elapsed / args.steps * 1e3,
        "higher_is_better": True,
        "scaling": "strong" if args.strong_total else "weak",
        "vs_baseline": None,
        "dtype": "f64",
        "data": "synthetic",
        "config": {
            "workload": (f"DTC autocorrelator sweep, L={args.L}, g=0.97, tf={T}, "
                         + ("device-like noise (T1/T2 relaxation + depolarizing + read-out, "
                            "stand-in calibration data/device_standin_L20.json)" if c3 else
                            "depolarizing p=0.05")
                         + f", 1 disorder instance (hs/phis_L{args.L}.csv row 0), "
                         + (f"{world * B} noisy trajectories per step split over {world} GPU(s) "
                            f"(strong scaling)" if args.strong_total else
                            f"{B} noisy trajectories per step per GPU (weak scaling)")
                         + ", forward+echo"),
            "L": args.L, "tf": T, "g": 0.97, "noise_prob": 0.05,
            "trajectories_per_step_per_gpu": B,
            "trajectories_per_step": world * B,
            "period_applications_per_trajectory": per_traj,
            "parallelism": f"traj-sharded x{world}",
        },
        "roofline": {
            "bound": "hbm",
            "kernel": ("dtc_kdk_pass / dtc_kdk_pass3 / dtc_kdk_dual (kick layer . fused RZZ+RZ "
                       "diagonal . kick layer; one launch advances every state by one Floquet "
                       "period; the dual form also stores the echo branch's first pass, 48 B "
                       "per amplitude, so the per-launch algorithmic bytes average above "
                       "32 * 2^L * B); launch-weighted over all of them"),
            "achieved": achieved,
            "peak": HBM_PEAK_GBS,
            "unit": "GB/s",
            "frac": achieved / HBM_PEAK_GBS,
            "frac_of_measured_copy": achieved / HBM_MEASURED_GBS,
            "frac_of_best_rw_stream": achieved / BEST_RW_STREAM_GBS,
            "traffic": traffic,
            "traffic_source": traffic_src,
            "algorithmic_bytes_per_launch": launch_bytes,
            "avg_launch_ms": avg_lo * 1e3,
            "launches": lo["launches"],
            "per_rank_GBps": [launch_bytes / (r[0] / max(1.0, r[1]) / 1e3) / 1e9
                              if r[1] else None for r in per_rank],
        },
        "kernels": {
            "kdk_pass": {"launches": lo["launches"], "avg_ms": avg_lo * 1e3,
                        "GBps": launch_bytes / avg_lo / 1e9 if lo["launches"] else None},
            "kick_pass": {"launches": hi["launches"], "avg_ms": avg_hi * 1e3,
                          "bytes_per_launch": hi_bytes,
                          "GBps": hi_bytes / avg_hi / 1e9 if hi["launches"] else None,
                          "note": "kick-only passes: the sweep's first (basis states formed "
                                  "in registers, store only, 16 B/amp) and, under device-like "
                                  "noise, the forward chain's kick passes (32 B/amp)"},
            "final_pass": {"launches": stats[4]["launches"], "avg_ms":
                           stats[4]["total_ms"] / max(1, stats[4]["launches"]),
                           "GBps": stats[4]["bytes"] / (stats[4]["total_ms"] / 1e3) / 1e9
                           if stats[4]["launches"] else None,
                           "note": "last pass of each echo chain: measure only, no store (16 B/amp)"},
            "reduce": {"launches": stats[2]["launches"], "total_ms": stats[2]["total_ms"]},
            "kernel_time_frac": sum(stats[k]["total_ms"] for k in stats) / (elapsed * 1e3),
        },
        "executed": {
            "note": ("value counts period applications of the full forward+echo sweep "
                     "(output-equivalent: the same per-trajectory results, oracle 1e-10); "
                     "the engine executes them as the passes below"),
            "launches_per_step": {"kdk_pass": n_launch[0], "kick_pass": n_launch[1],
                                  "lightcone_final_pass": n_launch[4]},
            "state_passes_per_step": state_passes / args.steps,
            "executed_state_passes_per_s": world * state_passes / elapsed,
            "period_applications_per_state_pass": (total_units / world) / max(1, state_passes),
            "algorithmic_hbm_bytes_per_step": hbm_bytes_kernels / args.steps,
            "algorithmic_hbm_GBps_over_timed_region": hbm_bytes_kernels / elapsed / 1e9,
        },
        "reference_equivalent": {
            "note": ("the reference runs one 1024-shot circuit per t (fwd and echo): "
                     "1024*3*T(T-1)/2 period applications per instance for the same per-t "
                     "statistics that 1024 trajectories give here"),
            "trajectories_per_s": world * args.steps * B / elapsed,
            "ref_period_applications_per_s": world * args.steps * B / elapsed
            * (3 * T * (T - 1) / 2),
        },
        "autocorr_t0_3": {"fwd": autocorr[0][:4].tolist(), "echo": autocorr[1][:4].tolist()},
        "device": info["name"],
    }
    if cpu:
        res["cpu_baseline"] = cpu
    if c5 is not None:
        res["c5"] = c5
    print(json.dumps(res), flush=True)
    if dist:
        dist.destroy_process_group()


def main_c4(args):
    """L=28, 256 disorder instances x 30 periods, noiseless
    forward + per-site <Z_i(t)>, j=14; instance-sharded (32 per GPU at N=8).
    One step = `--instances` instances per GPU, each a full T=30 forward sweep
    (29 period applications) with all 28 <Z_i(t)> measured every period."""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    import torch

    dist = None
    dev, backend = _device_and_backend(local_rank, world)
    cdev = _coll_dev(backend)
    torch.cuda.set_device(dev)
    if world > 1:
        import torch.distributed as dist

        dist.init_process_group(backend)
    pkg = importlib.import_module(PKG)
    L, T, n = 28, args.tf, args.instances
    eng = pkg.DtcEngine(dev)
    sums = np.zeros((T, L))
    last = {}  # the latest step's outputs (--dump-outputs)

    def step(i):
        lo = ((i * world + rank) * n) % 256
        hs, phis = load_disorder_rows(pkg, L, lo, lo + n)
        spec = pkg.SweepSpec(L=L, T=T, hs=hs, phis=phis, g=0.97, use_noise=0)
        out = eng.autocorr(spec, 1, want_echo=False, want_zsite=True)
        sums[:] += out["zsite"][:, 0].sum(axis=0)
        last.update(out)

    for i in range(args.warmup):
        step(i)
    sums[:] = 0
    eng.reset_stats()
    eng.set_profiling(True)
    if dist:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(args.steps):
        step(args.warmup + i)
    acc = torch.from_numpy(sums).to(cdev)
    if dist:
        dist.all_reduce(acc)  # the only collective: per-site <Z_i(t)> sums
    torch.cuda.synchronize()
    if dist:
        dist.barrier()
    elapsed = time.perf_counter() - t0
    eng.set_profiling(False)
    stats = eng.kernel_stats()
    el = torch.tensor([elapsed], dtype=torch.float64, device=cdev)
    if dist:
        dist.all_reduce(el, op=dist.ReduceOp.MAX)
    elapsed = float(el.item())
    dump_outputs(args.dump_outputs, last, rank, world)
    if rank != 0:
        if dist:
            dist.destroy_process_group()
        return
    per_inst = T - 1
    value = world * args.steps * n * per_inst / elapsed
    lo_s, hi_s = stats[0], stats[1]
    avg_lo = lo_s["total_ms"] / max(1, lo_s["launches"]) / 1e3
    avg_hi = hi_s["total_ms"] / max(1, hi_s["launches"]) / 1e3
    # algorithmic bytes per launch as the engine recorded them (32 B x 2^L x batch)
    launch_bytes = lo_s["bytes"] / max(1, lo_s["launches"])
    hi_bytes = hi_s["bytes"] / max(1, hi_s["launches"])
    achieved = launch_bytes / avg_lo / 1e9 if lo_s["launches"] else 0.0
    # PMC summary of this config (tools/pmc_traffic.sh with BENCH_ARGS="--config
    # c4", L=28): one launch holds the step's n instances' states
    traffic, traffic_src = read_traffic(launch_bytes, "_pmc_c4.json", batch=n)
    res = {
        "metric": "Floquet-periods×instances/sec at L=28 (C4); RZZ-kernel HBM GB/s vs peak",
        "value": value, "unit": "periods*instances/s", "n_gpus": world, "steps": args.steps,
        "warmup": args.warmup, "ms_per_step": elapsed / args.steps * 1e3,
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f64",
        "data": "synthetic (data/hs_L28.csv, seeded generate_disorder)",
        "config": {"workload": (f"C4: L=28 noiseless forward sweep, tf={T}, g=0.97, per-site "
                                f"<Z_i(t)> every period, {n} instances per step per GPU"),
                   "L": L, "tf": T, "instances_per_step_per_gpu": n,
                   "parallelism": f"instance-sharded x{world}"},
        "roofline": {"bound": "hbm", "kernel": "dtc_kdk_pass (+ dtc_kick_pass, 2 passes/period)",
                     "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                     "frac": achieved / HBM_PEAK_GBS,
                     "frac_of_best_rw_stream": achieved / BEST_RW_STREAM_GBS,
                     "traffic": traffic, "traffic_source": traffic_src,
                     "algorithmic_bytes_per_launch": launch_bytes,
                     "avg_launch_ms": avg_lo * 1e3, "launches": lo_s["launches"]},
        "kernels": {"kdk_pass": {"launches": lo_s["launches"], "avg_ms": avg_lo * 1e3},
                    "kick_pass": {"launches": hi_s["launches"], "avg_ms": avg_hi * 1e3,
                                  "GBps": hi_bytes / avg_hi / 1e9 if hi_s["launches"] else None},
                    "kernel_time_frac": (lo_s["total_ms"] + hi_s["total_ms"] + stats[2]["total_ms"])
                    / (elapsed * 1e3)},
        "z_mean_t1": float(acc[1].mean().item() / (world * args.steps * n)),
        "device": eng.device_info()["name"],
    }
    print(json.dumps(res), flush=True)
    if dist:
        dist.destroy_process_group()


def main_c5(args):
    """one noiseless state, L=34, tf=30, sharded over 8 ranks
    (32 GiB per GPU): per period the pre-exchange kicks run slice by slice (slice
    s of every destination chunk in one launch) and slice s travels to all 7
    peers at once (RCCL point-to-point over xGMI, side stream) while slice s+1
    is kicked; the fused pass (kicks of the newly local sites, RZZ/RZ, <Z_i>,
    next kick) follows (sharded.sharded_forward_pipelined).

    On one GPU the same driver runs the 2^shard_bits shards as virtual ranks
    of the full L=34 state (256 GiB) in ONE buffer: each slice's exchange is
    the in-place piece swap (dtc_shard_exchange_slice) instead of xGMI
    transfers, so the per-rank kernels run at their production sizes (n_local
    = 31).  If the state does not fit, the line reports the measured free
    bytes instead.  --L 31 (or smaller) runs the two-buffer virtual exchange."""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    import torch

    dist = None
    torch.cuda.set_device(local_rank if world > 1 else 0)
    if world > 1:
        import torch.distributed as dist

        dist.init_process_group("nccl")
    pkg = importlib.import_module(PKG)
    k = args.shard_bits
    if world > 1:
        if world & (world - 1):
            raise SystemExit("c5: the rank count must be a power of two")
        k = world.bit_length() - 1   # one shard per rank
    L = args.L if args.L != 20 else 34
    T = args.tf
    W = 1 << k
    hs, phis = pkg.load_disorder(34, 1, os.path.join(ROOT, "data"))
    spec = pkg.SweepSpec(L=L, T=T, hs=hs, phis=phis, g=0.97, use_noise=0)
    eng = pkg.DtcEngine(local_rank)
    stepper = pkg.sharded.EngineStepper(eng)
    lay = pkg.sharded.initial_layout(L, k, rank * (W // world), W // world)
    shard_bytes = 16.0 * (1 << (L - k)) * lay.n_shards      # held by this rank
    free, total = torch.cuda.mem_get_info()
    inplace = world == 1 and 2 * shard_bytes + (4 << 30) > free
    need = shard_bytes * (1 if inplace else 2) + (4 << 30)
    if need > free:
        if rank == 0:
            print(json.dumps({
                "metric": f"Floquet-periods/sec, one L={L} state sharded over {W} ranks (C5)",
                "value": None, "error": (f"the state does not fit: need {need:.0f} B "
                                         f"(state + 4 GiB), hipMemGetInfo free {free} B of "
                                         f"{total} B"), "n_gpus": world}), flush=True)
        if dist:
            dist.destroy_process_group()
        return
    bufs = stepper.alloc(lay, n_buffers=1 if inplace else 2)
    xstats = {}

    def step():
        return pkg.sharded.sharded_forward_pipelined(stepper, spec, k, rank=rank, world=world,
                                                     buffers=bufs, stats=xstats,
                                                     inplace=inplace)

    for _ in range(args.warmup):
        step()
    eng.reset_stats()
    eng.set_profiling(True)
    ex_ms, per_ms = [], []
    if dist:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        out = step()
        ex_ms += xstats.get("exchange_ms", [])
        per_ms += xstats.get("period_ms", [])
    torch.cuda.synchronize()
    if dist:
        dist.barrier()
    elapsed = time.perf_counter() - t0
    eng.set_profiling(False)
    stats = eng.kernel_stats()
    P = T - 1
    n_per = max(1, args.steps * P)
    lo_s, hi_s, xk = stats[0], stats[1], stats[5]
    pass_ms = (lo_s["total_ms"] + hi_s["total_ms"]) / n_per
    pass_bytes = (lo_s["bytes"] + hi_s["bytes"]) / n_per
    sent = shard_bytes * (W - 1) / W   # per rank per period (in place: moved per GPU)
    # in place on one GPU the slices' exchange is fused into their last kick
    # pass (dtc_shard_kick_exchange_slice): no kernel of its own, no window
    fused = inplace and xk["launches"] == 0
    if inplace:
        xch_ms = xk["total_ms"] / n_per          # the swap kernels (engine HIP events)
    else:
        xch_ms = float(np.sum(ex_ms)) / n_per    # side-stream window per period
    # per rank: period ms (engine stream), pass ms, exchange ms, exchange GB/s
    mine = torch.tensor([float(np.mean(per_ms)) if per_ms else elapsed * 1e3 / n_per, pass_ms,
                         xch_ms, sent / (xch_ms / 1e3) / 1e9 if xch_ms > 0 else 0.0, elapsed],
                        dtype=torch.float64, device="cuda")
    ranks = [mine]
    if dist:
        ranks = [torch.zeros_like(mine) for _ in range(world)]
        dist.all_gather(ranks, mine)
    ranks = [r.cpu().numpy() for r in ranks]
    elapsed = max(float(r[4]) for r in ranks)
    if args.steps:
        dump_outputs(args.dump_outputs, {k: np.asarray(v) for k, v in out.items()}, rank, world)
    if rank != 0:
        if dist:
            dist.destroy_process_group()
        return
    achieved = pass_bytes / (pass_ms / 1e3) / 1e9 if pass_ms else 0.0
    # PMC summary of this line (tools/pmc_traffic.sh with BENCH_ARGS="--config
    # c5", one GPU: tools/pmc_summary.py's per-period form), scaled to this run
    c5_traffic, c5_traffic_src = (read_traffic(pass_bytes, "_pmc_c5.json")
                                  if inplace else (None, None))
    # a per-period model for judging the 8-GPU run: the passes at
    # this rank's measured pass rate, plus the exchange of (W-1)/W of the shard
    # over 7 xGMI links at 7 x 153 GB/s (MI355X_MICROARCH/the task's figure)
    link_GBps = 7 * 153.0
    model_ms = pass_ms + (sent / (link_GBps * 1e9) * 1e3 if world > 1 else 0.0)
    res = {
        "metric": f"Floquet-periods/sec, one L={L} state sharded over {W} ranks (C5)",
        "value": args.steps * P / elapsed, "unit": "periods/s", "n_gpus": world,
        "steps": args.steps, "warmup": args.warmup, "ms_per_step": elapsed / args.steps * 1e3,
        "higher_is_better": True, "scaling": "strong", "vs_baseline": None, "dtype": "f64",
        "data": "synthetic (data/hs_L34.csv row 0, seeded generate_disorder)",
        "config": {"workload": (f"C5: one noiseless L={L} state, tf={T}, g=0.97, per-site "
                                f"<Z_i(t)> every period, {W} shards of n_local={L - k} "
                                + (f"({'virtual, 1 GPU, in-place exchange' if inplace else 'virtual, 1 GPU'})"
                                   if world == 1 else "(one per GPU)")),
                   "L": L, "tf": T, "shards": W, "n_local": L - k,
                   "state_bytes": 16.0 * (1 << L), "parallelism": f"state-sharded x{world}"},
        "roofline": {"bound": "hbm",
                     "kernel": "pass kernels (slice kicks + fused K-D-K), per-rank shard",
                     "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                     "frac": achieved / HBM_PEAK_GBS,
                     "traffic": c5_traffic, "traffic_source": c5_traffic_src,
                     "traffic_unit": "HBM bytes per period (PMC, this rank's shard)",
                     "algorithmic_bytes_per_period": pass_bytes},
        "period_ms": elapsed / n_per * 1e3,
        "pass_ms_per_period": pass_ms,
        "launches_per_period": {"kdk_pass": lo_s["launches"] / n_per,
                                "kick_pass": hi_s["launches"] / n_per,
                                "exchange": xk["launches"] / n_per},
        "exchange": {"per_period_ms": xch_ms, "fused_into_kick_pass": fused,
                     "bytes_per_period_per_rank": sent,
                     "swap_kernel_hbm_GBps": (xk["bytes"] / (xk["total_ms"] / 1e3) / 1e9
                                              if inplace and xk["total_ms"] else None),
                     "GBps_per_rank": sent / (xch_ms / 1e3) / 1e9 if xch_ms > 0 else None,
                     "window": ("none: each slice's last kick pass stores every piece at its "
                                "partner's place (dtc_shard_kick_exchange_slice)" if fused else
                                "the swap kernels' HIP events (engine stream; serial with the "
                                "kicks)" if inplace else
                                "side-stream events from the first slice's transfer to the last "
                                "one's completion (overlaps the slice kicks)"),
                     "kind": ("in-place piece swap fused into the slice kicks (virtual ranks, "
                              "one 256 GiB buffer)" if fused else
                              "in-place piece swap per slice (virtual ranks, one 256 GiB "
                              "buffer: dtc_shard_exchange_slice)" if inplace else
                              "strided device copy per slice (virtual ranks)" if world == 1 else
                              "RCCL point-to-point per slice over xGMI: every peer at once "
                              "(batch_isend_irecv of 7 sends + 7 receives)"),
                     # what has checked this exchange before this run
                     "verification": ("virtual ranks on one GPU: tests/test_gpu_c5_l34.py, "
                                      "test_gpu_sharded.py" if world == 1 else
                                      "unverified on GPUs before this run: the real-rank "
                                      "ordering ran over the loopback transport "
                                      "(test_loopback_real_rank_exchange) and gloo (world 8), "
                                      "RCCL itself only here; check z_t1_mean = cos(pi g)")},
        "per_rank": [{"rank": i, "period_ms": float(r[0]), "pass_ms": float(r[1]),
                      "exchange_ms": float(r[2]), "exchange_GBps": float(r[3])}
                     for i, r in enumerate(ranks)],
        "model_period_ms": model_ms,
        "model": ("pass_ms (this run's passes) + (W-1)/W of the shard over 7 xGMI links at "
                  "153 GB/s each, no overlap" if world > 1 else
                  "pass_ms only (one GPU: no link)"),
        "pass_time_frac": pass_ms * n_per / 1e3 / elapsed,
        "hbm_free_before_bytes": free,
        "z_t1_mean": float(out["zsite"][1].mean()),
        "kat_cos_pi_g": float(np.cos(np.pi * 0.97)),
        "device": eng.device_info()["name"],
    }
    print(json.dumps(res), flush=True)
    if dist:
        dist.destroy_process_group()


_CDEV = "cuda"


def _init_dist():
    """(world, rank, device ordinal, torch.distributed or None) of this rank."""
    global _CDEV
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    import torch

    dist = None
    dev, backend = _device_and_backend(local_rank, world)
    _CDEV = _coll_dev(backend)
    torch.cuda.set_device(dev)
    if world > 1:
        import torch.distributed as dist

        dist.init_process_group(backend)
    return world, rank, dev, dist


def _timed(eng, dist, warmup, steps, step, reduce_buf):
    """Warmup, then exactly `steps` steps between barrier + synchronize; the
    per-rank accumulator `reduce_buf` (numpy) is all-reduced once inside the
    timed region.  Returns (max-over-ranks seconds, reduced array, kernel stats)."""
    import torch

    for i in range(warmup):
        step(i)
    reduce_buf[...] = 0
    eng.reset_stats()
    eng.set_profiling(True)
    if dist:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        step(warmup + i)
    acc = torch.from_numpy(reduce_buf).to(_CDEV)
    if dist:
        dist.all_reduce(acc)
    torch.cuda.synchronize()
    if dist:
        dist.barrier()
    elapsed = time.perf_counter() - t0
    eng.set_profiling(False)
    stats = eng.kernel_stats()
    el = torch.tensor([elapsed], dtype=torch.float64, device=_CDEV)
    if dist:
        dist.all_reduce(el, op=dist.ReduceOp.MAX)
    return float(el.item()), acc.cpu().numpy(), stats


def _pass_kernels(stats, elapsed):
    """Roofline of the K-D-K pass kernel (stats kind 0) from the engine's HIP
    events, plus the other kinds' totals."""
    lo_s, hi_s = stats[0], stats[1]
    avg_lo = lo_s["total_ms"] / max(1, lo_s["launches"]) / 1e3
    avg_hi = hi_s["total_ms"] / max(1, hi_s["launches"]) / 1e3
    lo_b = lo_s["bytes"] / max(1, lo_s["launches"])
    hi_b = hi_s["bytes"] / max(1, hi_s["launches"])
    achieved = lo_b / avg_lo / 1e9 if lo_s["launches"] else 0.0
    roof = {"bound": "hbm", "kernel": "dtc_kdk_pass", "achieved": achieved,
            "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": achieved / HBM_PEAK_GBS,
            "frac_of_best_rw_stream": achieved / BEST_RW_STREAM_GBS, "traffic": None,
            "algorithmic_bytes_per_launch": lo_b, "avg_launch_ms": avg_lo * 1e3,
            "launches": lo_s["launches"]}
    kern = {"kdk_pass": {"launches": lo_s["launches"], "avg_ms": avg_lo * 1e3},
            "kick_pass": {"launches": hi_s["launches"], "avg_ms": avg_hi * 1e3,
                          "GBps": hi_b / avg_hi / 1e9 if hi_s["launches"] else None},
            "reduce": {"launches": stats[2]["launches"], "total_ms": stats[2]["total_ms"]},
            "final_pass": {"launches": stats[4]["launches"], "total_ms": stats[4]["total_ms"],
                           "GBps": stats[4]["bytes"] / (stats[4]["total_ms"] / 1e3) / 1e9
                           if stats[4]["launches"] else None},
            "kernel_time_frac": sum(stats[k]["total_ms"] for k in stats) / (elapsed * 1e3)}
    return roof, kern


def _host_threads():
    return host_cpu_info()["usable_cores"]


def main_energy(args):
    """SURVEY.md §8(f)1, the energy path (…-fast-energy.py:136-173 at L=20):
    per-trajectory <Z_i>, <Z_i Z_i+1>, <X_i> after every period of the noisy
    forward sweep (dtc_energy), L=20, g=0.97, p=0.05, vacuum, tf=30.  One step
    = `--batch` trajectories per GPU; <H(t)>/L of instance 0 is formed on the
    host from the trajectory means (energy.energy_from_observables).  Value =
    trajectories x (tf-1) periods per second over all ranks (each period also
    measures Z, ZZ and X, all in flight inside the period's pass)."""
    world, rank, local_rank, dist = _init_dist()
    pkg = importlib.import_module(PKG)
    # 1024 trajectories per step unless --batch says otherwise: the per-call host
    # work (result copies and their unpacking) then stays near 2 % of a step
    # (r3zn: 145.2k at 1024 vs 138.4k at 256 on one box)
    if not args.batch:
        args.batch = 1024
    L, T, B = args.L, args.tf, args.batch
    hs, phis = load_disorder_row(L)
    spec = pkg.SweepSpec(L=L, T=T, hs=hs, phis=phis, g=0.97, noise_prob=0.05, use_noise=1)
    eng = pkg.DtcEngine(local_rank)
    sums = np.zeros((3, T, L))
    last = {}  # the latest step's outputs (--dump-outputs)

    def step(i):
        # the estimator's trajectory sums, reduced on the device (dtc_energy_sums:
        # the same per-trajectory passes, a few KB instead of 15 MB of rows to
        # the host per step)
        off = (rank * (args.warmup + args.steps) + i) * B
        obs = eng.energy_sums(spec, B, traj_offset=off, batch=B)
        sums[0] += obs["z"][0]
        sums[1, :, :L - 1] += obs["zz"][0]
        sums[2] += obs["x"][0]
        last.update(obs)

    elapsed, acc, stats = _timed(eng, dist, args.warmup, args.steps, step, sums)
    dump_outputs(args.dump_outputs, last, rank, world)
    if rank != 0:
        if dist:
            dist.destroy_process_group()
        return
    n = world * args.steps * B
    mean = {"z": acc[0] / n, "zz": acc[1, :, :L - 1] / n, "x": acc[2] / n}
    e_t = pkg.energy.energy_from_observables(mean, L, 0.97, hs[0], phis[0], "full") / L
    roof, kern = _pass_kernels(stats, elapsed)
    roof["kernel"] = ("dtc_kdk_pass (one forward period; Z, ZZ after the diagonal and X before "
                      "each site's kick measured in flight)")
    roof["traffic"], roof["traffic_source"] = read_traffic(roof["algorithmic_bytes_per_launch"],
                                                           "_pmc_energy.json", batch=B)
    cpu = None
    if args.full and world == 1 and not args.no_cpu_baseline:
        cpu = cpu_baseline_energy(spec, args.cpu_traj or 2 * _host_threads(),
                                  min(args.cpu_tf or 6, 6), _host_threads())
    res = {
        "metric": "Floquet-periods×trajectories/sec at L=20 with <Z_i>,<Z_iZ_i+1>,<X_i> per "
                  "period (energy path); RZZ-kernel HBM GB/s vs peak",
        "value": n * (T - 1) / elapsed, "unit": "periods*trajectories/s", "n_gpus": world,
        "steps": args.steps, "warmup": args.warmup, "ms_per_step": elapsed / args.steps * 1e3,
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f64",
        "data": "synthetic (disorder row 0 of hs/phis_L20.csv)",
        "config": {"workload": (f"energy path (§8(f)1): L={L}, g=0.97, p=0.05, vacuum, tf={T}, "
                                f"{B} noisy trajectories per step per GPU, Z/ZZ/X every period"),
                   "L": L, "tf": T, "trajectories_per_step_per_gpu": B,
                   "parallelism": f"traj-sharded x{world}"},
        "roofline": roof, "kernels": kern,
        "energy_per_site_t0_3": [float(x) for x in e_t[:4]],
        "device": eng.device_info()["name"],
    }
    if cpu:
        res["cpu_baseline"] = cpu
    print(json.dumps(res), flush=True)
    if dist:
        dist.destroy_process_group()


def cpu_baseline_energy(spec, n_traj, T_sample, threads):
    """oracle/energy_oracle.py (C gate-by-gate periods + numpy observables),
    one trajectory per host thread."""
    import dataclasses
    from concurrent.futures import ThreadPoolExecutor

    from oracle import energy_oracle

    s = dataclasses.replace(spec, T=T_sample)
    t0 = time.perf_counter()
    with ThreadPoolExecutor(threads) as ex:
        list(ex.map(lambda tr: energy_oracle.trajectory_energy(s, 0, tr), range(n_traj)))
    dt = time.perf_counter() - t0
    work = n_traj * (T_sample - 1)
    return {"value": work / dt, "unit": "periods*trajectories/s", "cores": threads,
            "kind": "port",
            "sample": (f"oracle/energy_oracle.py (C oracle periods + numpy Z/ZZ/X): L={spec.L}, "
                       f"{n_traj} trajectories x T={T_sample} = {work} periods in {dt:.1f} s")}


def main_ctrl(args):
    """SURVEY.md §8(f)2, the real-time adaptive-g controller
    (…-controlled-g.py:423-532) on the committed L=20 configuration
    (controlled-autocorr_data_L20: g_initial=0.84, p=0.05, 1024 shots,
    tf=20): one step = one instance's closed loop, at every t one engine call
    for the forward and echo values of the g history (t+1 periods each) and a
    host feedback update.  Instances (disorder rows) are sharded over ranks.
    Value = period applications x trajectories per second."""
    world, rank, local_rank, dist = _init_dist()
    pkg = importlib.import_module(PKG)
    L, T, shots = args.L, args.ctrl_tf, 1024
    eng = pkg.DtcEngine(local_rank)
    cfg = pkg.control.ControllerConfig(use_optimization=int(args.ctrl_opt),
                                       prefix_cache=0 if args.no_prefix_cache else 1)
    hs, phis = load_disorder_row(L)
    res_g = np.zeros((1, T))
    last = {}  # the latest step's outputs (--dump-outputs)

    def step(i):
        r = pkg.control.realtime_adaptive(L, T, hs, phis, 0.84, cfg, noise_prob=0.05,
                                          shots=shots, seed=0x5EED0001 + 7919 * (i * world + rank),
                                          engine=eng)
        res_g[0] += r.g[0]
        last.update(forward=r.forward, echo=r.echo, g=r.g)

    elapsed, acc, stats = _timed(eng, dist, args.warmup, args.steps, step, res_g)
    dump_outputs(args.dump_outputs, last, rank, world)
    if rank != 0:
        if dist:
            dist.destroy_process_group()
        return
    per_loop = shots * sum(2 * (t + 1) for t in range(T))
    n_loops = world * args.steps
    roof, kern = _pass_kernels(stats, elapsed)
    # its own PMC passes (tools/pmc_traffic.sh with BENCH_ARGS="--config ctrl"), if any
    roof["traffic"], roof["traffic_source"] = read_traffic(roof["algorithmic_bytes_per_launch"],
                                                           "_pmc_ctrl.json", batch=shots)
    cpu = None
    # (the optimisation loop's evaluation count is data-dependent: no fixed CPU work unit)
    if args.full and world == 1 and not args.no_cpu_baseline and not args.ctrl_opt:
        hs_, phis_ = load_disorder_row(L)
        s = pkg.SweepSpec(L=L, T=args.cpu_tf or 20, hs=hs_, phis=phis_, g=0.84, noise_prob=0.05,
                          use_noise=1, t_offset=1)
        cpu = cpu_baseline(s, args.cpu_traj or 2 * _host_threads(), s.T,
                           _host_threads(), t_offset=1)
        cpu["unit"] = "periods*trajectories/s"
    if args.ctrl_opt:
        pc = "without" if args.no_prefix_cache else "with"
        head = {
            "metric": (f"controller time points/sec of the L={L} optimisation loop "
                       "(g-optimization); RZZ-kernel HBM GB/s vs peak"),
            "value": n_loops * T / elapsed, "unit": "time points/s"}
        workload = (f"optimisation controller (§8(f)2, bounded Brent per t, {pc} the forward "
                    f"prefix cache): L={L}, g_initial=0.84, p=0.05, tf={T}, {shots} "
                    f"trajectories per evaluation, one closed loop per step per GPU")
    else:
        head = {
            "metric": "Floquet-periods×trajectories/sec of the L=20 real-time adaptive-g loop "
                      "(controlled-g); RZZ-kernel HBM GB/s vs peak",
            "value": n_loops * per_loop / elapsed, "unit": "periods*trajectories/s"}
        workload = (f"adaptive-g controller (§8(f)2): L={L}, g_initial=0.84, p=0.05, "
                    f"tf={T}, {shots} trajectories per estimate, exponential "
                    f"feedback (gain 0.01), one closed loop per step per GPU")
    res = dict(head)
    res.update({
        "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": elapsed / args.steps * 1e3, "higher_is_better": True, "scaling": "weak",
        "vs_baseline": None, "dtype": "f64", "data": "synthetic (disorder row 0 of hs/phis_L20.csv)",
        "config": {"workload": workload,
                   "L": L, "tf": T, "shots": shots, "parallelism": f"instance-sharded x{world}"},
        "roofline": roof, "kernels": kern,
        "ms_per_time_point": elapsed / (args.steps * T) * 1e3,
        "g_history_mean": (acc[0] / n_loops).tolist(),
        "device": eng.device_info()["name"],
    })
    if cpu:
        res["cpu_baseline"] = cpu
    print(json.dumps(res), flush=True)
    if dist:
        dist.destroy_process_group()


if __name__ == "__main__":
    sys.exit(main() or 0)
