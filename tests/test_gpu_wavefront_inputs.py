"""The wavefront interior (csrc/dtc_wavefront.hip dtc_wf_pass, wf_replace and
wf_table_set in csrc/dtc_schedule.h) away from the inputs the other wavefront
files share -- one disorder instance, a scalar g, the probe on site 10:

  * moved probes: the probe site sets where the light cones end, so which runs
    of an echo chain the planner may replace; the six cases of
    tests/wavefront_cases.py run every wavefront pass shape (tile, kick steps,
    trailing kick-less diagonal) and every table-set key that any probe gives at
    T = 8 .. 12 (tests/test_wavefront_inputs_cpu.py holds the census);
  * several instances in one call: the kernel's instance index
    (batch_start + b) / n_traj, the [set][n_inst][slot][outside bit] strides of
    the tables and the angles wf_table_set builds them from, with octets that
    straddle an instance edge and batches that start inside the call;
  * a g list: a kick row of its own per period, so a step handed another
    layer's row shows in the values;
  * xy_cycle kicks: both kick families in one sweep, no wavefront pass.

L = 20, p = 0.05, the octet layout (eight states or more in a batch); every
call on a fresh engine with DTC_WAVEFRONT and DTC_NO_WAVEFRONT cleared.  RX
kicks (g = 0.97) from the vacuum, RY kicks (g = 0.93) from the Neel state.

Values: the fused C oracle (c_oracle.autocorr_fused, pinned to the gate-by-gate
one for these inputs in tests/test_oracle.py) for the named states at 1e-10, and
the plain interior (DTC_NO_WAVEFRONT=1) over all rows at 1e-12 (echo) / 1e-13
(fwd), the project's standing bounds.  Launches: wavefront_count() and
lightcone_counts() must be what the case's schedule dump
(tools/schedule_check.cpp) tallies, per batch.  The plain run and the oracle rows
of a case are computed once and shared.

One probe case also runs the echo alone from t_first = T - 2, whose rows must be
the full run's bits: the wavefront passes of a chain do not depend on what ran
around them, and neither does the forward chain before it."""
import subprocess

import numpy as np
import pytest

from oracle import c_oracle
from tests import wavefront_cases as wc
from tests.helpers import random_disorder
from tests.test_schedule_cpu import build

pytestmark = pytest.mark.gpu

SEED = 2210
TOL_ORACLE, TOL_ECHO, TOL_FWD = 1e-10, 1e-12, 1e-13
_REFS = {}
BY_NAME = {c.name: c for c in wc.CASES}


def _ids(cases):
    return [c.name for c in cases]


def _spec(pkg, case, inst=None):
    """The case's sweep; inst: that instance's disorder row alone."""
    rng = np.random.default_rng(3000 + wc.CASES.index(case))
    hs, phis = random_disorder(rng, wc.L, case.n_inst)
    if inst is not None:
        hs, phis = hs[inst:inst + 1], phis[inst:inst + 1]
    g = {"x": 0.97, "y": 0.93, "xy_cycle": 0.95}[case.kick]
    if case.g_list:
        g = list(np.linspace(0.84, 1.0, case.T - 1 + case.t_offset))
    return pkg.SweepSpec(L=wc.L, T=case.T, hs=hs, phis=phis, g=g, noise_prob=wc.P_NOISE,
                         polarization=case.kick,
                         initial_state="neel" if case.kick == "y" else "vacuum",
                         t_offset=case.t_offset, probe_site=case.probe)


def _run(pkg, monkeypatch, spec, n_traj, plain=False, **kw):
    """One autocorr call on a fresh engine (plain: DTC_NO_WAVEFRONT=1); the rows
    and the engine's launch counts."""
    with monkeypatch.context() as m:
        m.delenv("DTC_WAVEFRONT", raising=False)
        m.delenv("DTC_NO_WAVEFRONT", raising=False)
        if plain:
            m.setenv("DTC_NO_WAVEFRONT", "1")
        with pkg.DtcEngine(0) as eng:
            out = eng.autocorr(spec, n_traj, seed=SEED, **kw)
            lc = eng.lightcone_counts()
            counts = {"wf": eng.wavefront_count(), "lc8": lc["lc8"],
                      "lc10": lc["lcw"] + lc["lcw2"], "lc12": lc["lcw3"]}
            eng.release_buffers()
    return out, counts


def _oracle_rows(pkg, case):
    """{state: {"fwd": [T], "echo": [T]}} of the case's oracle states, each from
    a one-instance spec at the state's trajectory offset (neighbouring
    trajectories in one call: the oracle runs them side by side)."""
    rows = {}
    for inst in range(case.n_inst):
        trs = sorted(s % case.n_traj for s in case.oracle if s // case.n_traj == inst)
        spec = _spec(pkg, case, inst)
        while trs:
            lo = trs[0]
            run = [t for t in trs if t < lo + 6]
            trs = trs[len(run):]
            ref = c_oracle.autocorr_fused(spec, run[-1] - lo + 1, seed=SEED, traj_offset=lo)
            for t in run:
                rows[inst * case.n_traj + t] = {k: v[0, t - lo] for k, v in ref.items()}
    assert sorted(rows) == sorted(case.oracle)
    return rows


def _refs(pkg, monkeypatch, case):
    """(plain interior of the whole call, oracle rows), read-only"""
    if case.name not in _REFS:
        plain, counts = _run(pkg, monkeypatch, _spec(pkg, case), case.n_traj, plain=True)
        assert counts["wf"] == 0
        rows = _oracle_rows(pkg, case)
        for a in (*plain.values(), *(v for r in rows.values() for v in r.values())):
            a.setflags(write=False)
        _REFS[case.name] = (plain, rows)
    return _REFS[case.name]


@pytest.fixture(scope="module")
def sched_exe(tmp_path_factory):
    return build(tmp_path_factory.mktemp("wf_inputs_sched"), [])


def _dump_counts(sched_exe, case):
    r = subprocess.run([sched_exe, *wc.sched_args(case)], capture_output=True, text=True,
                       check=True)
    return wc.launch_counts(r.stdout)


def _assert_values(case, got, plain, rows):
    """Oracle parity of the named states, plain-schedule parity of all rows."""
    errs = {}
    for k in ("fwd", "echo"):
        flat = got[k].reshape(-1, case.T)
        errs[k] = (max(float(np.abs(flat[s] - r[k]).max()) for s, r in rows.items()),
                   float(np.abs(got[k] - plain[k]).max()))
        print(f"{case.name} {k}: oracle {errs[k][0]:.3e}  plain {errs[k][1]:.3e}")
    for k in ("fwd", "echo"):
        assert got[k].shape == (case.n_inst, case.n_traj, case.T)
        assert errs[k][0] < TOL_ORACLE, (case.name, k)
    assert errs["echo"][1] < TOL_ECHO and errs["fwd"][1] < TOL_FWD, case.name
    # the rows are no trivial ones: every state's own
    assert len(np.unique(got["echo"].reshape(-1, case.T)[:, -1])) == case.n_inst * case.n_traj


def _assert_counts(case, counts, want, n_batches=1):
    print(f"{case.name} launches {counts} in {n_batches} batch(es)")
    assert counts == {k: n_batches * v for k, v in want.items()}, (case.name, counts, want)
    assert (counts["wf"] > 0) == (case not in wc.FALLBACK_CASES)


@pytest.mark.parametrize("case", wc.PROBE_CASES, ids=_ids(wc.PROBE_CASES))
def test_moved_probe(pkg, monkeypatch, sched_exe, case):
    """Eight trajectories, one octet; oracle rows of the states 0 and 7.  Probe 0
    has no light-cone end at all (its counts are all zero), probe 5 only 8-site
    ends; probe 11 is the site both tiles hold, 12 the column group's first."""
    plain, rows = _refs(pkg, monkeypatch, case)
    got, counts = _run(pkg, monkeypatch, _spec(pkg, case), case.n_traj)
    _assert_values(case, got, plain, rows)
    want = _dump_counts(sched_exe, case)
    _assert_counts(case, counts, want)
    if case.probe == 0:
        assert counts["lc8"] == counts["lc10"] == counts["lc12"] == 0
    if case.probe == 5:
        assert counts["lc8"] > 0 and counts["lc10"] == counts["lc12"] == 0


def test_probe0_against_the_gate_oracle(pkg, monkeypatch):
    """State 3 of the probe-0 case against the gate-by-gate oracle, independent of
    the fused restatement."""
    case = wc.PROBE_CASES[0]
    assert (case.probe, case.T) == (0, 8)
    spec = _spec(pkg, case)
    got, counts = _run(pkg, monkeypatch, spec, case.n_traj)
    assert counts["wf"] > 0
    ref = c_oracle.autocorr(spec, 1, seed=SEED, traj_offset=3)
    for k in ("fwd", "echo"):
        err = float(np.abs(got[k][0, 3] - ref[k][0, 0]).max())
        print(f"{case.name} {k}: gate-by-gate oracle {err:.3e}")
        assert err < TOL_ORACLE, k


def _run_dual_off(pkg, monkeypatch, spec, n_traj, **kw):
    with monkeypatch.context() as m:
        m.setenv("DTC_NO_DUAL", "1")
        return _run(pkg, monkeypatch, spec, n_traj, **kw)


def test_echo_alone_from_t_first_is_the_full_runs(pkg, monkeypatch):
    """want_fwd = False and t_first = T - 2 (other launches around the same two
    chains, which run the same wavefront passes): the echo rows it computes must
    be the full run's bits, the rest 0.

    The forward chain has to be the same arithmetic in both runs: a full run
    folds each echo start into the forward pass (the dual pass), a t_first run
    starts no chain before t_first, and the 8-site group's dual pass applies its
    kicks in Pauli-frame form.  Its plain forward pass once ran the variant
    branches, whose butterflies round differently, and these rows then differed
    from the full run's by up to 5.6e-16 (with DTC_NO_WAVEFRONT=1 too: not the
    wavefront's doing); now the group's forward K-D-K runs in frame form whether
    or not it starts a chain (dtc_kdk_pass_fr in csrc/dtc_kernels.hip)."""
    case = BY_NAME["probe5-T11-off1-x"]
    spec = _spec(pkg, case)
    lo = case.T - 2
    full, counts = _run(pkg, monkeypatch, spec, case.n_traj)
    part, pcounts = _run(pkg, monkeypatch, spec, case.n_traj, want_fwd=False, t_first=lo)
    assert counts["wf"] > 0 and pcounts["wf"] > 0
    assert set(part) == {"echo"}
    assert part["echo"][..., lo:].all() and not part["echo"][..., :lo].any()
    err = float(np.abs(part["echo"][..., lo:] - full["echo"][..., lo:]).max())
    print(f"{case.name} echo alone from t_first = {lo} against the full run: {err:.3e}")
    assert np.array_equal(part["echo"][..., lo:], full["echo"][..., lo:]), err
    # ... and with the forward rows: the forward state is the full run's too
    late, _ = _run(pkg, monkeypatch, spec, case.n_traj, t_first=lo)
    for k in ("fwd", "echo"):
        assert np.array_equal(late[k][..., lo:], full[k][..., lo:]), k
        assert not late[k][..., :lo].any()


def test_echo_alone_is_the_full_runs_bits(pkg, monkeypatch):
    """want_fwd = False on its own (every chain still starts in a dual pass):
    every echo row is the full run's, bit for bit."""
    case = BY_NAME["probe5-T11-off1-x"]
    spec = _spec(pkg, case)
    full, counts = _run(pkg, monkeypatch, spec, case.n_traj)
    part, pcounts = _run(pkg, monkeypatch, spec, case.n_traj, want_fwd=False)
    assert counts == pcounts and counts["wf"] > 0
    assert set(part) == {"echo"} and np.array_equal(part["echo"], full["echo"])


def test_t_first_is_the_full_runs_bits_without_dual_passes(pkg, monkeypatch):
    """DTC_NO_DUAL=1, the wavefront interior on: every forward pass is a plain
    one whatever t_first is, and the rows from t_first = T - 2 on (forward and
    echo, and the echo alone) are the full run's bits -- the wavefront passes of
    the two chains do not depend on what ran around them."""
    case = BY_NAME["probe5-T11-off1-x"]
    spec = _spec(pkg, case)
    lo = case.T - 2
    full, counts = _run_dual_off(pkg, monkeypatch, spec, case.n_traj)
    part, pcounts = _run_dual_off(pkg, monkeypatch, spec, case.n_traj, t_first=lo)
    alone, _ = _run_dual_off(pkg, monkeypatch, spec, case.n_traj, want_fwd=False, t_first=lo)
    assert counts["wf"] > pcounts["wf"] > 0
    for k in ("fwd", "echo"):
        assert np.array_equal(part[k][..., lo:], full[k][..., lo:]), k
        assert not part[k][..., :lo].any()
    assert np.array_equal(alone["echo"], part["echo"])


def test_two_instances_in_every_batching(pkg, monkeypatch, sched_exe):
    """2 x 12 states, probe 4, T = 10, t_offset 1, RX.  batch=0: one batch, whose
    second octet (states 8 .. 15) straddles the instance edge 11 | 12; batch=8:
    batches at 0, 8 and 16, the middle one straddling; batch=16: the second batch
    a lone octet at 16.  The same bits every way, and each instance's rows the
    bits of a call with that instance's disorder row alone (12 states, the same
    kernels in the octet layout).  Oracle rows of the states 7, 8, 11, 12, 15,
    16 and 23."""
    case = BY_NAME["inst2x12-probe4-T10-off1-x"]
    spec = _spec(pkg, case)
    assert np.abs(spec.hs[0] - spec.hs[1]).min() > 1e-3
    plain, rows = _refs(pkg, monkeypatch, case)
    want = _dump_counts(sched_exe, case)
    got, counts = _run(pkg, monkeypatch, spec, case.n_traj, batch=0)
    _assert_values(case, got, plain, rows)
    _assert_counts(case, counts, want)
    for batch, n_batches in ((8, 3), (16, 2)):
        other, ocounts = _run(pkg, monkeypatch, spec, case.n_traj, batch=batch)
        _assert_counts(case, ocounts, want, n_batches)
        for k in ("fwd", "echo"):
            assert np.array_equal(got[k], other[k]), (k, batch, float(np.abs(got[k] - other[k]).max()))
    for inst in range(case.n_inst):
        one, icounts = _run(pkg, monkeypatch, _spec(pkg, case, inst), case.n_traj)
        _assert_counts(case, icounts, want)
        for k in ("fwd", "echo"):
            assert np.array_equal(got[k][inst], one[k][0]), \
                (k, inst, float(np.abs(got[k][inst] - one[k][0]).max()))
    # every trajectory's rows differ between the instances by far more than any
    # bound here
    assert np.abs(got["echo"][0] - got["echo"][1]).max(axis=-1).min() > 1e-3


def test_three_instances_in_one_octet(pkg, monkeypatch, sched_exe):
    """3 x 3 states, the default probe, T = 11, RY from the Neel state: the
    octet holds the instances 0, 1 and most of 2, a partial octet the last state.
    Oracle rows of the states 2, 3, 7 and 8.  A call with one instance's row has
    three states, which run contiguous and without the wavefront: against those
    at the plain-schedule bounds."""
    case = BY_NAME["inst3x3-T11-y"]
    plain, rows = _refs(pkg, monkeypatch, case)
    got, counts = _run(pkg, monkeypatch, _spec(pkg, case), case.n_traj)
    _assert_values(case, got, plain, rows)
    _assert_counts(case, counts, _dump_counts(sched_exe, case))
    for inst in range(case.n_inst):
        one, icounts = _run(pkg, monkeypatch, _spec(pkg, case, inst), case.n_traj)
        assert icounts["wf"] == 0
        for k, tol in (("echo", TOL_ECHO), ("fwd", TOL_FWD)):
            err = float(np.abs(got[k][inst] - one[k][0]).max())
            print(f"{case.name} instance {inst} alone {k}: {err:.3e}")
            assert err < tol, (k, inst)


@pytest.mark.parametrize("case", wc.G_LIST_CASES, ids=_ids(wc.G_LIST_CASES))
def test_g_list(pkg, monkeypatch, sched_exe, case):
    """g = linspace(0.84, 1.0, T - 1 + t_offset), eight trajectories: every layer
    of a wavefront pass has a kick row of its own.  Oracle rows of the states 0
    and 7."""
    spec = _spec(pkg, case)
    assert spec.kick.shape[0] == case.T - 1 + case.t_offset
    assert all(np.abs(spec.kick[r] - spec.kick[r + 1]).max() > 1e-3
               for r in range(spec.kick.shape[0] - 1))
    plain, rows = _refs(pkg, monkeypatch, case)
    got, counts = _run(pkg, monkeypatch, spec, case.n_traj)
    _assert_values(case, got, plain, rows)
    _assert_counts(case, counts, _dump_counts(sched_exe, case))


def test_xy_cycle_runs_the_plain_interior(pkg, monkeypatch, sched_exe):
    """xy_cycle kicks, T = 12, nine states in one batch (batch=0, the octet
    layout): every row is RX or RY, so the sweep is one the wavefront applies
    to, and every run spans the RX | RY edge, so no pass may be planned.
    Oracle rows of the states 0, 7 and 8; the bits of the contiguous run
    (batch=1)."""
    case = wc.FALLBACK_CASES[0]
    spec = _spec(pkg, case)
    plain, rows = _refs(pkg, monkeypatch, case)
    got, counts = _run(pkg, monkeypatch, spec, case.n_traj, batch=0)
    _assert_values(case, got, plain, rows)
    _assert_counts(case, counts, _dump_counts(sched_exe, case))
    assert counts["wf"] == 0
    one, ocounts = _run(pkg, monkeypatch, spec, case.n_traj, batch=1)
    assert ocounts["wf"] == 0
    for k in ("fwd", "echo"):
        assert np.array_equal(got[k], one[k]), (k, float(np.abs(got[k] - one[k]).max()))
