"""The octet batch layout against the C oracle, for every site-group plan.

A batch of eight or more states of up to 2^25 amplitudes runs in the octet
layout (csrc/dtc_kernels.h state_base / octet_spread: the eight states of an
octet interleaved in runs of 2^6 amplitudes); batch_layout in dtc_engine.cpp
picks it whenever a batch holds B >= 8 states and L_eff <= 25, and every
smaller batch runs contiguous states.  The other parity files call the engine
with one to six states, so this file runs each plan of tests/plan_table.py, with
factored (RX / RY) and general 2x2 kicks, in the layout production runs use:

  * nine or ten states in one batch (batch=0): one full octet and a partial
    one, whose padding states the passes sweep too;
  * the same trajectories in batches of one (and of five): contiguous states;
    include/dtc.h promises that results do not depend on batching, so the rows
    are the same bits (where the wavefront interior ran, which only the octet
    layout has, its tests' bounds: 1e-12 echo, 1e-13 forward);
  * the octet run's rows of the states 0, 7 and 8 -- the octet's first and last
    state and the partial octet's first -- against the oracle at 1e-10.
"""
import re

import numpy as np
import pytest

from oracle import c_oracle
from tests.helpers import harsh_device, random_disorder
from tests.plan_table import plan_id

pytestmark = pytest.mark.gpu
TOL = 1e-10
GENERAL = ("xy", "yx", "circular_left", "circular_right", "xy_cycle")


def _delta(after, before):
    return {k: after[k] - before[k] for k in after}


def _oracle_rows(spec, n_traj, seed, want_zsite, t_first, n_oracle):
    """{trajectory id: oracle rows [n_inst][...]} of the states 0, 7 and 8 of the
    batch (state = inst * n_traj + trajectory); n_oracle = 2: 7 and 8 only,
    1: 8 only."""
    t7, t8 = 7 % n_traj, 8 % n_traj
    assert t8 == t7 + 1
    calls = {3: [(0, 1), (t7, 2)], 2: [(t7, 2)], 1: [(t8, 1)]}[n_oracle]
    rows = {}
    for off, n in calls:
        ref = c_oracle.autocorr(spec, n, seed=seed, traj_offset=off, want_zsite=want_zsite,
                                t_first=t_first)
        for i in range(n):
            rows[off + i] = {k: v[:, i] for k, v in ref.items()}
    return rows


def _octet_case(pkg, eng, spec, n_traj, seed=1234, want_zsite=False, batches=(1,), n_oracle=3,
                t_first=0, same_rows=False):
    """One sweep in the octet layout (batch=0) and in contiguous batches, the
    layouts against each other and the octet run against the oracle (module
    docstring).  same_rows: a noiseless sweep, whose trajectories are all the
    oracle's one.  Returns the octet call's light-cone, schedule and wavefront
    counts, and the contiguous calls' light-cone counts per batch size."""
    S = n_traj * spec.n_inst
    assert S >= 9 and S % 8, "one full octet and a partial one"
    kw = dict(seed=seed, want_zsite=want_zsite, t_first=t_first)
    lc0, sc0, wf0 = eng.lightcone_counts(), eng.schedule_counts(), eng.wavefront_count()
    got = eng.autocorr(spec, n_traj, batch=0, **kw)
    info = {"lc": _delta(eng.lightcone_counts(), lc0), "sched": _delta(eng.schedule_counts(), sc0),
            "wf": eng.wavefront_count() - wf0, "lc_contig": {}}
    # the wavefront interior (L = 20 only) runs in the octet layout alone
    assert info["wf"] == 0 or spec.L == 20
    for b in batches:
        lc1 = eng.lightcone_counts()
        other = eng.autocorr(spec, n_traj, batch=b, **kw)
        info["lc_contig"][b] = _delta(eng.lightcone_counts(), lc1)
        for k in got:
            if info["wf"] == 0:
                assert np.array_equal(got[k], other[k]), (k, b, float(np.abs(got[k] - other[k]).max()))
            else:
                err = float(np.abs(got[k] - other[k]).max())
                assert err < (1e-12 if k == "echo" else 1e-13), (k, b, err)
    if same_rows:
        ref = c_oracle.autocorr(spec, 1, seed=seed, traj_offset=8, want_zsite=want_zsite,
                                t_first=t_first)
        rows = {tid: {k: v[:, 0] for k, v in ref.items()} for tid in range(n_traj)}
    else:
        rows = _oracle_rows(spec, n_traj, seed, want_zsite, t_first, n_oracle)
    for tid, ref in rows.items():
        for k in ref:
            err = float(np.abs(got[k][:, tid] - ref[k]).max())
            print(f"L={spec.L} trajectory {tid} {k}: {err:.3e}")
            assert err < TOL, (k, tid, err)
        assert set(ref) == set(got)
    return info


def _spec(pkg, L, T, pol, n_inst=1, p=0.05, state="vacuum", toff=0, probe=None, noiseless=False,
          device=False):
    rng = np.random.default_rng(1000 * L + 10 * T + toff)
    hs, phis = random_disorder(rng, L, n_inst)
    kw = {} if probe is None else {"probe_site": probe}
    if device:
        kw["device"] = harsh_device(pkg, L)
    elif noiseless:
        kw.update(noise_prob=0.0, use_noise=0)
    else:
        kw["noise_prob"] = p
    return pkg.SweepSpec(L=L, T=T, hs=hs, phis=phis, g=0.93, polarization=pol, initial_state=state,
                         t_offset=toff, **kw)


def _case(L, T, pol, n_inst=1, p=0.05, state="vacuum", toff=0, noiseless=False, dual=False):
    tag = "-".join(filter(None, [plan_id(L), pol, "noiseless" if noiseless else "",
                                 "2inst" if n_inst == 2 else ""]))
    return pytest.param(L, T, pol, n_inst, p, state, toff, noiseless, dual, id=tag)


# Every L runs one factored kind (x, y alternating; per-site Z: the kMeasSites
# passes; batches of five too) and one general kind (the five in turn).  T <= 6
# up to L = 19 and T = 4 from L = 21 keep the oracle to a few seconds; xy_cycle
# kicks RX for five periods and RY for the next five, so its cases run six
# periods (T = 6, t_offset = 1).  dual: the sweep folds echo starts into dual
# passes (asserted on the octet run).
PLAN_CASES = [
    _case(5, 6, "x", p=0.2, state="neel"),
    _case(5, 6, "yx", n_inst=2, toff=1),
    _case(12, 6, "y", toff=1),
    _case(12, 6, "circular_left", p=0.2, state="neel"),
    _case(13, 6, "x", n_inst=2, state="neel"),
    _case(13, 6, "circular_right", p=0.2, dual=True),
    _case(14, 6, "y", p=0.2),
    _case(14, 6, "xy_cycle", state="neel", toff=1),
    _case(15, 6, "x", toff=1),
    _case(15, 6, "xy", p=0.2, state="neel"),
    _case(16, 6, "y", state="neel", toff=1),
    _case(16, 6, "yx", n_inst=2, p=0.2),
    _case(17, 5, "x", p=0.2, state="neel"),
    _case(17, 5, "circular_left", toff=1),
    _case(17, 5, "y", noiseless=True),
    _case(18, 5, "y", state="neel"),
    _case(18, 5, "circular_right", p=0.2, toff=1),
    _case(19, 5, "x", p=0.2, toff=1),
    _case(19, 6, "xy_cycle", state="neel", toff=1),
    _case(20, 4, "y", state="neel", toff=1),
    _case(20, 4, "xy", p=0.2),
    _case(21, 4, "x", p=0.2),
    _case(21, 4, "yx", state="neel"),
    _case(22, 4, "y", state="neel"),
    _case(22, 4, "circular_left", p=0.2, toff=1),
    _case(22, 4, "x", noiseless=True),
    _case(23, 4, "x"),
    _case(23, 4, "circular_right", p=0.2, state="neel"),
]


@pytest.mark.parametrize("L,T,pol,n_inst,p,state,toff,noiseless,dual", PLAN_CASES)
def test_octet_plans_and_kinds(pkg, engine, L, T, pol, n_inst, p, state, toff, noiseless, dual):
    spec = _spec(pkg, L, T, pol, n_inst, p, state, toff, noiseless=noiseless)
    factored = pol in ("x", "y")
    info = _octet_case(pkg, engine, spec, 5 if n_inst == 2 else 9, seed=4000 + L,
                       want_zsite=factored, batches=(1, 5) if factored else (1,),
                       n_oracle=3 if L <= 20 else 2, same_rows=noiseless)
    if dual:
        assert info["sched"]["folded"] > 0, info


def test_octet_case_list_is_complete():
    """Every plan from L = 13 to 23, both factored kinds and the five general
    ones stand in the list above."""
    ids = [c.id for c in PLAN_CASES]
    for L in range(13, 24):
        assert any(i.startswith(plan_id(L) + "-") for i in ids), L
    pols = {c.values[2] for c in PLAN_CASES}
    assert pols == {"x", "y", *GENERAL}
    for L in (5, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23):
        kinds = {c.values[2] in ("x", "y") for c in PLAN_CASES if c.values[0] == L}
        assert kinds == {True, False}, L


def test_nine_states_run_the_octet_layout(pkg, monkeypatch, capfd):
    """The guard of this file's premise: batch_layout picks the octet layout for
    a batch of B >= 8 states with L_eff <= 25, so the batch=0 call of nine
    states must run them as one batch (DTC_VERBOSE reports batch=9) and the
    batch=1 call one state at a time."""
    spec = _spec(pkg, 13, 3, "x")
    with monkeypatch.context() as m:
        m.setenv("DTC_VERBOSE", "1")
        with pkg.DtcEngine(0) as eng:
            capfd.readouterr()
            eng.autocorr(spec, 9, seed=1, batch=0)
            full = [int(v) for v in re.findall(r"batch=(\d+)", capfd.readouterr().err)]
            eng.autocorr(spec, 9, seed=1, batch=1)
            single = [int(v) for v in re.findall(r"batch=(\d+)", capfd.readouterr().err)]
    assert full and min(full) >= 8, full
    assert single and max(single) == 1, single


def test_L20_layouts_with_and_without_wavefront(pkg, engine, monkeypatch):
    """L = 20, chains long enough for the wavefront interior (T = 12; the
    oracle's side of it is test_gpu_wavefront.py's).  The default engine runs
    the interior in the octet layout only, a different kernel per layout: the
    wavefront tests' bounds, 1e-12 echo and 1e-13 forward.  With
    DTC_NO_WAVEFRONT=1 both layouts run the same kernels: the same bits."""
    spec = _spec(pkg, 20, 12, "y", p=0.05, state="neel")
    kw = dict(seed=20, t_first=9)
    wf0 = engine.wavefront_count()
    a = engine.autocorr(spec, 9, batch=0, **kw)
    assert engine.wavefront_count() > wf0
    wf1 = engine.wavefront_count()
    b = engine.autocorr(spec, 9, batch=1, **kw)
    assert engine.wavefront_count() == wf1
    for k, tol in (("echo", 1e-12), ("fwd", 1e-13)):
        err = float(np.abs(a[k] - b[k]).max())
        print(f"wavefront (octet) against plain (contiguous) {k}: {err:.3e}")
        assert a[k][..., 9:].any() and err < tol, (k, err)
    with monkeypatch.context() as m:
        m.setenv("DTC_NO_WAVEFRONT", "1")
        with pkg.DtcEngine(0) as eng:
            c = eng.autocorr(spec, 9, batch=0, **kw)
            d = eng.autocorr(spec, 9, batch=1, **kw)
            assert eng.wavefront_count() == 0
    for k in c:
        assert np.array_equal(c[k], d[k]), (k, float(np.abs(c[k] - d[k]).max()))


@pytest.mark.parametrize("L,T,pol,toff", [
    pytest.param(13, 6, "circular_left", 0, id=plan_id(13) + "-circular_left"),
    pytest.param(17, 5, "y", 0, id=plan_id(17) + "-y"),
    pytest.param(20, 4, "x", 1, id=plan_id(20) + "-x"),
])
def test_octet_device_noise(pkg, engine, L, T, pol, toff):
    """Device-like noise (tests/helpers.harsh_device), ten trajectories: the
    RXU / RYU / general K-D and dual kernels on 9-site and 4-site groups."""
    spec = _spec(pkg, L, T, pol, toff=toff, device=True)
    info = _octet_case(pkg, engine, spec, 10, seed=700 + L)
    assert info["sched"]["folded"] > 0, info


# L, T, t_first, pol, state, probe, t_offset, switches, what the octet run must
# launch: lc8 (8-site end), lc10 (a 10-site end, either kernel), lcw2 / lcw3
# (the C2 forms), folded (dual passes).  Above L = 18 one oracle trajectory (8)
# and only the last time point(s), whose chains are the long ones.
LC_CASES = [
    pytest.param(14, 7, 0, "y", "neel", None, 0, (), ("lc8", "lc10"), id=plan_id(14) + "-y"),
    pytest.param(16, 6, 0, "x", "vacuum", 5, 0, (), ("lc8", "folded"),
                 id=plan_id(16) + "-x-probe5"),
    pytest.param(16, 7, 0, "y", "vacuum", 12, 1, (), ("lc8", "lc10"),
                 id=plan_id(16) + "-y-probe12"),
    pytest.param(18, 6, 0, "x", "vacuum", 13, 1, (), ("lc8", "lc10"),
                 id=plan_id(18) + "-x-probe13"),
    pytest.param(21, 8, 7, "y", "vacuum", None, 0, (), ("lcw3",), id=plan_id(21) + "-y-lcw3"),
    pytest.param(21, 8, 7, "y", "vacuum", None, 0, ("DTC_NO_LCW3",), ("lcw2",),
                 id=plan_id(21) + "-y-lcw2"),
    pytest.param(22, 6, 4, "y", "vacuum", None, 0, (), ("lc8",), id=plan_id(22) + "-y"),
]


@pytest.mark.parametrize("L,T,t_first,pol,state,probe,toff,env,expect", LC_CASES)
def test_octet_light_cone_ends(pkg, monkeypatch, L, T, t_first, pol, state, probe, toff, env,
                               expect):
    """The three light-cone ends (8-, 10- and 12-site windows) in the octet
    layout, each case on an engine of its own: the oracle's rows, the contiguous
    run's bits, and the same ends launched in both layouts (nine batches of one
    launch nine times the one batch's)."""
    spec = _spec(pkg, L, T, pol, p=0.1, state=state, toff=toff, probe=probe)
    with monkeypatch.context() as m:
        for k in env:
            m.setenv(k, "1")
        with pkg.DtcEngine(0) as eng:
            info = _octet_case(pkg, eng, spec, 9, seed=77, t_first=t_first,
                               n_oracle=3 if L <= 18 else 1)
    lc = info["lc"]
    assert info["lc_contig"][1] == {k: 9 * v for k, v in lc.items()}, info
    seen = dict(lc, lc10=lc["lcw"] + lc["lcw2"], folded=info["sched"]["folded"])
    for k in expect:
        assert seen[k] > 0, (k, info)
    if "DTC_NO_LCW3" in env:
        assert lc["lcw3"] == 0
