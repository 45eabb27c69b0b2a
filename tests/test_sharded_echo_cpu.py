"""The echo on a sharded state (sharded.sharded_autocorr*, dtc_shard_echo_*)
on CPU: the drivers with the numpy echo stepper (tests/shard_echo_model.py)
against the whole-state C oracle's echo, per trajectory -- the chain's
schedule (fork, inverse periods, measure-only end), the bit maps and the
buffer plans.  The engine's own steps are checked on the GPU
(tests/test_gpu_sharded_echo.py)."""
import dataclasses
import os
import socket

import numpy as np
import pytest
import torch.multiprocessing as mp

from oracle import c_oracle
from tests.helpers import random_disorder
from tests.shard_echo_model import NumpyEchoStepper

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-12  # the CPU tolerance of test_sharded_cpu.py

SHAPES = [
    (6, 1, 6, 0.0, "vacuum", "x", 0),
    (7, 2, 6, 0.1, "neel", "circular_left", 0),
    (9, 3, 5, 0.05, "neel", "xy", 1),
    (10, 2, 4, 0.1, "vacuum", "x", 0),    # 4 slices
]


def _spec(pkg, L, T, p=0.1, state="neel", pol="circular_left", toff=0, seed=4):
    rng = np.random.default_rng(seed)
    hs, phis = random_disorder(rng, L, 2)
    return pkg.SweepSpec(L=L, T=T, hs=hs, phis=phis, g=0.91, noise_prob=p, polarization=pol,
                         initial_state=state, t_offset=toff)


def _halves(n):
    lo = (1 << (n // 2)) - 1
    return [lo, ((1 << n) - 1) ^ lo]


_REF = {}


def _ref(pkg, shape, traj, inst=1, seed=99):
    """The whole-state oracle for one instance and trajectory (computed once)."""
    key = (shape, traj, inst, seed)
    if key not in _REF:
        L, k, T, p, state, pol, toff = shape
        spec = _spec(pkg, L, T, p, state, pol, toff)
        one = dataclasses.replace(spec, hs=spec.hs[inst:inst + 1], phis=spec.phis[inst:inst + 1])
        r = c_oracle.autocorr(one, 1, seed=seed, traj_offset=traj, want_zsite=True,
                              want_echo=True)
        _REF[key] = {"fwd": r["fwd"][0, 0], "echo": r["echo"][0, 0], "zsite": r["zsite"][0, 0]}
    return _REF[key]


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("groups", [None, _halves])
@pytest.mark.parametrize("driver", ["blocking", "pipelined"])
def test_virtual_ranks_match_oracle(pkg, shape, groups, driver):
    L, k, T, p, state, pol, toff = shape
    spec = _spec(pkg, L, T, p, state, pol, toff)
    fn = pkg.sharded.sharded_autocorr if driver == "blocking" else \
        pkg.sharded.sharded_autocorr_pipelined
    for traj in (0, 3):
        got = fn(NumpyEchoStepper(groups), spec, k, inst=1, traj=traj, seed=99)
        ref = _ref(pkg, shape, traj)
        print(driver, shape, traj, "echo err", np.abs(got["echo"] - ref["echo"]).max(),
              "fwd err", np.abs(got["fwd"] - ref["fwd"]).max())
        assert np.abs(got["echo"] - ref["echo"]).max() < TOL
        assert np.abs(got["fwd"] - ref["fwd"]).max() < TOL
        assert np.abs(got["zsite"] - ref["zsite"]).max() < TOL
        assert np.abs(got["echo_norm"] - 1.0).max() < TOL
        assert got["echo"].shape == (T,) and got["echo_zsite"].shape == (T, L)
        if p == 0.0:
            # without noise every chain returns to the prepared state
            want = 1.0 - 2.0 * np.array([(spec.init_mask >> i) & 1 for i in range(L)])
            assert np.abs(got["echo_zsite"] - want[None, :]).max() < TOL


@pytest.mark.parametrize("driver", ["blocking", "pipelined"])
def test_forward_part_is_the_forward_drivers(pkg, driver):
    """The forward is the same steps in the same order: equal results."""
    L, k, T, p, state, pol, toff = SHAPES[2]
    spec = _spec(pkg, L, T, p, state, pol, toff)
    sh = pkg.sharded
    a, f = (sh.sharded_autocorr, sh.sharded_forward) if driver == "blocking" else \
        (sh.sharded_autocorr_pipelined, sh.sharded_forward_pipelined)
    got = a(NumpyEchoStepper(_halves), spec, k, inst=1, traj=3, seed=99)
    fwd = f(NumpyEchoStepper(_halves), spec, k, inst=1, traj=3, seed=99)
    for key in ("fwd", "zsite", "norm"):
        assert np.array_equal(got[key], fwd[key])
    assert set(fwd) == {"fwd", "zsite", "norm"}


@pytest.mark.parametrize("driver", ["blocking", "pipelined"])
def test_echo_times_subset(pkg, driver):
    shape = SHAPES[1]
    L, k, T, p, state, pol, toff = shape
    spec = _spec(pkg, L, T, p, state, pol, toff)
    fn = pkg.sharded.sharded_autocorr if driver == "blocking" else \
        pkg.sharded.sharded_autocorr_pipelined
    full = fn(NumpyEchoStepper(_halves), spec, k, inst=1, traj=3, seed=99)
    sub = fn(NumpyEchoStepper(_halves), spec, k, inst=1, traj=3, seed=99, echo_times=[0, 2, 5])
    for t in range(T):
        if t in (0, 2, 5):
            assert sub["echo"][t] == full["echo"][t]
            assert np.array_equal(sub["echo_zsite"][t], full["echo_zsite"][t])
        else:
            assert sub["echo"][t] == 0.0 and sub["echo_norm"][t] == 0.0
            assert not sub["echo_zsite"][t].any()
    none = fn(NumpyEchoStepper(_halves), spec, k, inst=1, traj=3, seed=99, echo_times=[])
    assert not none["echo"].any() and np.array_equal(none["fwd"], full["fwd"])
    with pytest.raises(ValueError):
        fn(NumpyEchoStepper(_halves), spec, k, echo_times=[T])


@pytest.mark.parametrize("shape", SHAPES[1:])
@pytest.mark.parametrize("groups", [None, _halves])
def test_inplace_buffer_plans(pkg, shape, groups):
    """In place with (A, E): any times; with (A,) alone the one chain after the
    last period runs in A -- equal to the two-buffer run; any other time is
    refused."""
    L, k, T, p, state, pol, toff = shape
    spec = _spec(pkg, L, T, p, state, pol, toff)
    fn = pkg.sharded.sharded_autocorr_pipelined
    st = NumpyEchoStepper(groups)
    ref = _ref(pkg, shape, 3)
    lay = pkg.sharded.initial_layout(L, k, 0, 1 << k)
    two = fn(st, spec, k, inst=1, traj=3, seed=99, inplace=True, buffers=st.alloc(lay, 2))
    assert np.abs(two["echo"] - ref["echo"]).max() < TOL
    assert np.abs(two["fwd"] - ref["fwd"]).max() < TOL
    one = fn(st, spec, k, inst=1, traj=3, seed=99, inplace=True, buffers=st.alloc(lay, 1),
             echo_times=[T - 1])
    assert one["echo"][T - 1] == two["echo"][T - 1]
    assert np.array_equal(one["echo_zsite"][T - 1], two["echo_zsite"][T - 1])
    assert not one["echo"][:T - 1].any()
    assert np.array_equal(one["fwd"], two["fwd"])
    for bad in (None, [0], [T - 2, T - 1]):
        with pytest.raises(ValueError):
            fn(st, spec, k, inst=1, traj=3, seed=99, inplace=True, buffers=st.alloc(lay, 1),
               echo_times=bad)


def test_bond_noise_is_refused(pkg):
    spec = dataclasses.replace(_spec(pkg, 6, 3), bond_noise=0.01)
    for fn in (pkg.sharded.sharded_autocorr, pkg.sharded.sharded_autocorr_pipelined):
        with pytest.raises(NotImplementedError, match="bond noise"):  # as the forward drivers
            fn(NumpyEchoStepper(), spec, 1)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _worker(rank, world, port, k, q, L):
    import sys

    sys.path.insert(0, ROOT)
    import torch.distributed as dist

    from __graft_entry__ import load_package

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    pkg = load_package()
    spec = _spec(pkg, L, 5)
    out = pkg.sharded.sharded_autocorr_pipelined(NumpyEchoStepper(_halves), spec, k, inst=0,
                                                 traj=2, seed=5, rank=rank, world=world)
    if rank == 0:
        q.put((out["fwd"], out["echo"]))
    dist.barrier()
    dist.destroy_process_group()


def test_gloo_ranks_match_oracle(pkg):
    """Two real ranks over gloo, pipelined: the chains' slice transfers and the
    joined (forward, echo) all-reduce."""
    k, L = 1, 8
    world = 1 << k
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, k, q, L)) for r in range(world)]
    for pr in procs:
        pr.start()
    fwd, echo = q.get(timeout=180)
    for pr in procs:
        pr.join(timeout=180)
        assert pr.exitcode == 0
    spec = _spec(pkg, L, 5)
    one = dataclasses.replace(spec, hs=spec.hs[:1], phis=spec.phis[:1])
    ref = c_oracle.autocorr(one, 1, seed=5, traj_offset=2, want_echo=True)
    assert np.abs(fwd - ref["fwd"][0, 0]).max() < TOL
    assert np.abs(echo - ref["echo"][0, 0]).max() < TOL


def test_cli_state_shards_flag(pkg, tmp_path, monkeypatch):
    import pandas as pd

    ns = pkg.cli.build_parser().parse_args([])
    assert ns.state_shards == 0
    assert pkg.cli.build_parser().parse_args(["--state_shards", "3"]).state_shards == 3
    dis = tmp_path / "dis"
    dis.mkdir()
    hs, phis = random_disorder(np.random.default_rng(6), 6)
    pd.DataFrame(hs).to_csv(dis / "hs_L6.csv", index=False)
    pd.DataFrame(phis).to_csv(dis / "phis_L6.csv", index=False)

    def no_engine(*a, **kw):
        raise AssertionError("an engine was opened")

    monkeypatch.setattr(pkg.sweep, "_default_engine", no_engine)
    monkeypatch.setattr(pkg.sweep, "DtcEngine", no_engine)
    common = ["--L", "6", "--tf", "3", "--trajectories", "2", "--shots", "0", "--disorder_folder",
              str(dis), "--out_dir", str(tmp_path / "no"), "--state_shards", "1"]
    for extra in (["--use_fakebackend", "1"], ["--bond_noise_prob", "0.01"],
                  ["--use_fakebackend", "1", "--fakebackend_bond", "1"],
                  ["--independent_t", "1"]):
        with pytest.raises(SystemExit, match="state_shards"):
            pkg.cli.main(common + extra)
    assert not (tmp_path / "no").exists()


def test_null_arguments_are_rejected(pkg):
    lib = pkg._capi.load_library()
    assert lib.dtc_shard_echo_step(None, None, None, None, 0, 0, 0, 0, 0, 0, 0, 0, None, None,
                                   None) == -1
    assert b"null" in lib.dtc_last_error()
    assert lib.dtc_shard_echo_step_async(None, None, None, None, 0, 0, 0, 0, 0, 0, 0, 0, None,
                                         None, None) == -1
    assert lib.dtc_shard_echo_kick_slice(None, None, None, None, 0, 0, 0, 0, 0, 0, 0, 0,
                                         None) == -1
    assert lib.dtc_shard_echo_kick_exchange_slice(None, None, None, None, 0, 0, 0, 0, 0, 0, 0,
                                                  None) == -1
