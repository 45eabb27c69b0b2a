"""The echo on a sharded state on one GPU with virtual ranks (dtc_shard_echo_*,
sharded.sharded_autocorr*) against the single-device engine's echo of the same
trajectory (dtc_autocorr), to the 1e-10 of tests/test_gpu_sharded.py: inverse
and undo kick layers under a shard's bit map, the conjugated effective-field
tables, the fork off the forward buffer, the buffer plans, and the measure-only
end (dtc_kick_sites_final)."""
import dataclasses

import numpy as np
import pytest

from oracle import c_oracle
from tests.helpers import random_disorder

pytestmark = pytest.mark.gpu
TOL = 1e-10

SHAPES = [
    (14, 1, 6, 0.0, "vacuum", "x", 0),
    (14, 2, 6, 0.1, "neel", "circular_left", 0),
    (15, 3, 5, 0.05, "neel", "xy", 1),      # n_local = 12, one group
    (18, 2, 6, 0.05, "vacuum", "y", 0),
    (22, 3, 5, 0.05, "neel", "x", 0),       # sliced
]
PIPELINED_ONLY = [(25, 3, 4, 0.05, "neel", "xy", 1)]
# the in-place exchange needs chunks of one 4096-amplitude tile (the forward
# driver's rule): n_local - k >= 12
INPLACE = [s for s in SHAPES + PIPELINED_ONLY if s[0] - 2 * s[1] >= 12]
TRAJS = (0, 5)


@pytest.fixture(scope="module")
def stepper(pkg, engine):
    return pkg.sharded.EngineStepper(engine)


def _spec(pkg, shape):
    L, k, T, p, state, pol, toff = shape
    rng = np.random.default_rng(L * 7 + k)
    hs, phis = random_disorder(rng, L, 2)
    return pkg.SweepSpec(L=L, T=T, hs=hs, phis=phis, g=0.93, noise_prob=p, polarization=pol,
                         initial_state=state, t_offset=toff)


_REF = {}


def _ref(pkg, engine, shape, traj):
    """The single-device engine's sweep of instance 1, one trajectory (once)."""
    if (shape, traj) not in _REF:
        spec = _spec(pkg, shape)
        one = dataclasses.replace(spec, hs=spec.hs[1:2], phis=spec.phis[1:2])
        r = engine.autocorr(one, 1, seed=77, traj_offset=traj, want_zsite=True)
        _REF[shape, traj] = {k: r[k][0, 0] for k in ("fwd", "echo", "zsite")}
    return _REF[shape, traj]


def _check(got, ref, what):
    e_echo = np.abs(got["echo"] - ref["echo"]).max()
    e_fwd = np.abs(got["fwd"] - ref["fwd"]).max()
    print(what, "echo err %.3e fwd err %.3e" % (e_echo, e_fwd))
    assert e_echo < TOL
    assert e_fwd < TOL
    assert np.abs(got["echo_norm"] - 1.0).max() < TOL


@pytest.mark.parametrize("shape", SHAPES)
def test_blocking_virtual_shards_match_engine(pkg, engine, stepper, shape):
    spec, k = _spec(pkg, shape), shape[1]
    for traj in TRAJS:
        got = pkg.sharded.sharded_autocorr(stepper, spec, k, inst=1, traj=traj, seed=77)
        _check(got, _ref(pkg, engine, shape, traj), f"blocking {shape} traj {traj}")
        fwd = pkg.sharded.sharded_forward(stepper, spec, k, inst=1, traj=traj, seed=77)
        for key in ("fwd", "zsite", "norm"):  # the same launches in the same order
            assert np.array_equal(got[key], fwd[key]), key


@pytest.mark.parametrize("shape", SHAPES + PIPELINED_ONLY)
def test_pipelined_virtual_shards_match_engine(pkg, engine, stepper, shape):
    spec, k = _spec(pkg, shape), shape[1]
    for traj in TRAJS:
        got = pkg.sharded.sharded_autocorr_pipelined(stepper, spec, k, inst=1, traj=traj, seed=77)
        _check(got, _ref(pkg, engine, shape, traj), f"pipelined {shape} traj {traj}")
        fwd = pkg.sharded.sharded_forward_pipelined(stepper, spec, k, inst=1, traj=traj, seed=77)
        for key in ("fwd", "zsite", "norm"):
            assert np.array_equal(got[key], fwd[key]), key


@pytest.mark.parametrize("shape", INPLACE)
def test_pipelined_inplace_virtual_shards_match_engine(pkg, engine, stepper, shape):
    """In place with (A, E), every chain, and with (A,) alone the one chain the
    buffer can hold, each with the fused kick+exchange and with the two calls."""
    L, k, T = shape[:3]
    spec = _spec(pkg, shape)
    fn = pkg.sharded.sharded_autocorr_pipelined
    lay = pkg.sharded.initial_layout(L, k, 0, 1 << k)
    A, E = stepper.alloc(lay, 2)
    for traj in TRAJS:
        ref = _ref(pkg, engine, shape, traj)
        runs = {}
        for fuse in (True, False):
            got = fn(stepper, spec, k, inst=1, traj=traj, seed=77, inplace=True, buffers=(A, E),
                     fuse_kick_exchange=fuse)
            _check(got, ref, f"in place (A, E) fuse={fuse} {shape} traj {traj}")
            one = fn(stepper, spec, k, inst=1, traj=traj, seed=77, inplace=True, buffers=(A,),
                     echo_times=[T - 1], fuse_kick_exchange=fuse)
            e = abs(one["echo"][T - 1] - ref["echo"][T - 1])
            print(f"in place (A,) fuse={fuse} {shape} traj {traj} echo err {e:.3e}")
            assert e < TOL
            assert np.abs(one["fwd"] - ref["fwd"]).max() < TOL
            assert not one["echo"][:T - 1].any()
            runs[fuse] = (got, one)
        # fused against separate: the same kicks in another kernel
        assert np.abs(runs[True][0]["echo"] - runs[False][0]["echo"]).max() < 1e-13
        assert np.abs(runs[True][0]["echo_zsite"] - runs[False][0]["echo_zsite"]).max() < 1e-13
        assert np.abs(runs[True][1]["echo"] - runs[False][1]["echo"]).max() < 1e-13
    with pytest.raises(ValueError):
        fn(stepper, spec, k, inst=1, inplace=True, buffers=(A,), echo_times=[0])


@pytest.mark.parametrize("shape", SHAPES[:2])
def test_echo_zsite_against_host_periods(pkg, engine, stepper, shape):
    """Every site of E_t at L = 14: forward periods on stream 0, then as many
    inverse periods on stream 1 + t, through dtc_apply_periods."""
    L, k, T = shape[:3]
    spec = _spec(pkg, shape)
    one = dataclasses.replace(spec, hs=spec.hs[1:2], phis=spec.phis[1:2])
    traj = 5
    m = c_oracle.init_mask(one, 77, traj)
    F = np.zeros(1 << L, dtype=np.complex128)
    F[m] = 1.0
    want = np.zeros((T, L))
    want[0] = [-1.0 if (m >> i) & 1 else 1.0 for i in range(L)]
    for t in range(1, T):
        F, _ = engine.apply_periods(one, F, t, 1, traj=traj, stream=0, seed=77)
        _, z = engine.apply_periods(one, F, t, t, inverse=True, traj=traj, stream=1 + t, seed=77)
        want[t] = z[1:]
    for fn in (pkg.sharded.sharded_autocorr, pkg.sharded.sharded_autocorr_pipelined):
        got = fn(stepper, spec, k, inst=1, traj=traj, seed=77)
        err = np.abs(got["echo_zsite"] - want).max()
        print(fn.__name__, shape, "echo_zsite err %.3e" % err)
        assert err < TOL


def _counts(engine, run):
    engine.set_profiling(True)
    try:
        engine.reset_stats()
        run()
        engine.synchronize()
        return engine.kernel_stats()
    finally:
        engine.set_profiling(False)


def test_inverse_period_books_a_forward_periods_launches(pkg, engine, stepper):
    """(22, 3), in place with the exchange as launches of its own: an inverse
    period costs the passes and exchanges of a forward period, a chain ends in
    one measure-only pass of 16 B per amplitude, and the fork is the chain's
    first step, not an extra launch."""
    C = pkg._capi
    shape = SHAPES[4]
    L, k, T = shape[:3]
    spec = _spec(pkg, shape)
    longer = _spec(pkg, shape[:2] + (T + 1,) + shape[3:])   # one more forward period
    lay = pkg.sharded.initial_layout(L, k, 0, 1 << k)
    A, E = stepper.alloc(lay, 2)
    kw = dict(inst=1, traj=0, seed=77, inplace=True, fuse_kick_exchange=False)
    sh = pkg.sharded
    f5 = _counts(engine, lambda: sh.sharded_forward_pipelined(stepper, spec, k, buffers=(A,), **kw))
    f6 = _counts(engine, lambda: sh.sharded_forward_pipelined(stepper, longer, k, buffers=(A,),
                                                              **kw))
    a5 = _counts(engine, lambda: sh.sharded_autocorr_pipelined(stepper, spec, k, buffers=(A, E),
                                                               **kw))
    kinds = (C.KERNEL_LO_PASS, C.KERNEL_HI_PASS, C.KERNEL_EXCHANGE)
    per_period = {q: f6[q]["launches"] - f5[q]["launches"] for q in kinds}
    assert per_period[C.KERNEL_LO_PASS] == 1 and per_period[C.KERNEL_EXCHANGE] >= 1
    n_chains = T - 1                       # t = 0 has no period to invert
    n_inverse = sum(range(1, T))           # chain t: t periods
    for q in kinds:
        # (a chain's LO passes: the fork and the p - 1 fused steps after it)
        assert a5[q]["launches"] - f5[q]["launches"] == n_inverse * per_period[q], q
    assert f5[C.KERNEL_FINAL_PASS]["launches"] == 0
    assert a5[C.KERNEL_FINAL_PASS]["launches"] == n_chains
    assert a5[C.KERNEL_FINAL_PASS]["bytes"] == n_chains * 16.0 * (1 << L)


@pytest.mark.parametrize("L,k", [(14, 1), (14, 2), (22, 3)])  # 4-, 12- and 8-site top groups
def test_measure_only_end_equals_stored_end(pkg, engine, stepper, L, k):
    import torch

    shape = (L, k, 4, 0.1, "neel", "xy", 0)
    spec = _spec(pkg, shape)
    lay = pkg.sharded.initial_layout(L, k, 0, 1 << k).exchanged()
    gen = torch.Generator(device="cpu").manual_seed(L + k)
    x = torch.randn(1 << L, dtype=torch.complex128, generator=gen)
    src = (x / x.norm()).cuda()
    dst = torch.empty_like(src)
    keep = src.clone()
    t = 3
    args = (spec, lay, 77, 2, 1, t, t, lay.top_mask, False, 0)
    only = stepper.step_echo(*args, src, None, True)
    assert torch.equal(src, keep)          # nothing stored
    stored = stepper.step_echo(*args, src, dst, True)
    assert np.array_equal(only, stored)
    assert abs(only[:, 0].sum() - 1.0) < 1e-12


def test_invalid_echo_steps(pkg, engine, stepper):
    import torch

    shape = SHAPES[0]
    L, k = shape[:2]
    spec = _spec(pkg, shape)
    lay = pkg.sharded.initial_layout(L, k, 0, 1 << k)
    src, dst = stepper.alloc(lay, 2)
    src.zero_()
    torch.cuda.synchronize()
    top = lay.top_mask
    with pytest.raises(pkg._capi.DtcError, match="error -1"):   # DTC_EINVAL
        stepper.step_echo(spec, lay, 77, 0, 1, 2, 1, top, True, 0, src, None, True)
    with pytest.raises(pkg._capi.DtcError, match="error -1"):
        stepper.step_echo(spec, lay, 77, 0, 1, 2, 3, top, False, 0, src, dst, True)   # k > p
    with pytest.raises(pkg._capi.DtcError, match="error -1"):
        stepper.step_echo(spec, lay, 77, 0, 1, 2, 2, top, True, top, src, dst, True)  # post at k = p
    with pytest.raises(pkg._capi.DtcError, match="error -1"):
        stepper.kick_slice_echo(spec, lay, 77, 0, 2, 3, 1, k, 0, 0, src)
    # dst == NULL with the kicked bits in two site groups
    with pytest.raises(pkg._capi.DtcError, match="error -1"):
        stepper.step_echo(spec, lay, 77, 0, 1, 2, 2, lay.local_mask, False, 0, src, None, True)
