"""The wavefront pass at four workgroups per CU (csrc/dtc_wavefront.hip,
DTC_WF_WG4): LDS holds only the per-register table of every diagonal, each
thread fetches its own entry of the other table from the global table -- the
index XORed with the step's part of the frame's X, the last diagonal's entry
negated by the parity of that index under the frame's Z -- and the trailing
diagonal runs inside the step loop.

The wavefront interior only exists at L = 20 with the octet layout, so the
shapes are small by batch and T: 8, 12 and 16 trajectories from id 1016 (12: a
partial second octet, whose padding states return before the first barrier; 16
straddles 1023 | 1024).  RY kicks from the Neel state with t_offset = 1 at
T = 10, and RX kicks from the vacuum at T = 11, one row more: without the time
offset the planner finds no chain worth a wavefront pass up to T = 10 (0
launches at every cap: test_rx_vacuum_t10_plans_no_wavefront_pass holds that
reason in place), and 11 is the first T with launches at the default cap and at
caps 2 and 3 (4, 6, 4).  Both at p = 0.05 and at p = 0.5 (dense frames:
X masks on the table bits of both halves, Z on the last diagonal); at the
default layer cap and at caps 2 and 3 (odd step counts: the trailing diagonal
runs in layout 0 / 1 and is fetched there).

Values: the C oracle per trajectory at 1e-10; the plain interior
(DTC_NO_WAVEFRONT=1): fwd identical (the forward chain has no wavefront pass),
echo within 1e-12, the project's bound between schedules.  The same call twice
is bit-identical (a missing barrier shows as run-to-run differences), and one
batch of 16 is bit-identical to two of 8.  Wavefront launches are counted in
every case, so a silent fall-back to the plain interior cannot pass.  The
oracle and the plain run of a spec are computed once for the 16 trajectories
and shared."""
import numpy as np
import pytest

from oracle import c_oracle
from tests.helpers import random_disorder

pytestmark = pytest.mark.gpu

OFF = 1016
SEED = 2110
T = {"rx_vacuum": 11, "ry_neel": 10}
SPECS = ["rx_vacuum", "ry_neel"]
_REFS = {}


def _spec(pkg, name, p, t=None):
    rng = np.random.default_rng(410)
    hs, phis = random_disorder(rng, 20, 1)
    if name == "rx_vacuum":
        return pkg.SweepSpec(L=20, T=t or T[name], hs=hs, phis=phis, g=0.97, noise_prob=p,
                             initial_state="vacuum")
    return pkg.SweepSpec(L=20, T=T[name], hs=hs, phis=phis, g=0.93, noise_prob=p,
                         polarization="y", initial_state="neel", t_offset=1)


def _env(m, cap):
    """cap: None = the default wavefront interior, 0 = the plain interior"""
    m.delenv("DTC_WAVEFRONT", raising=False)
    m.delenv("DTC_NO_WAVEFRONT", raising=False)
    if cap == 0:
        m.setenv("DTC_NO_WAVEFRONT", "1")
    elif cap:
        m.setenv("DTC_WAVEFRONT", str(cap))


def _refs(pkg, monkeypatch, name, p):
    """(plain interior, C oracle) of trajectories OFF .. OFF + 15, read-only"""
    key = (name, p)
    if key not in _REFS:
        spec = _spec(pkg, name, p)
        with monkeypatch.context() as m:
            _env(m, 0)
            with pkg.DtcEngine(0) as eng:
                plain = eng.autocorr(spec, 16, seed=SEED, traj_offset=OFF)
                assert eng.wavefront_count() == 0
                eng.release_buffers()
        ref = c_oracle.autocorr(spec, 16, seed=SEED, traj_offset=OFF)
        for a in (*plain.values(), *ref.values()):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _REFS[key] = (plain, ref)
    return _REFS[key]


def _assert_values(got, plain, ref, n):
    errs = {k: (float(np.abs(got[k] - ref[k][:, :n]).max()),
                float(np.abs(got[k] - plain[k][:, :n]).max())) for k in ("fwd", "echo")}
    for k, (eo, ep) in errs.items():
        print(f"{k}: oracle {eo:.3e}  plain {ep:.3e}")
    for k in ("fwd", "echo"):
        assert errs[k][0] < 1e-10, k
    assert errs["fwd"][1] == 0.0
    assert errs["echo"][1] <= 1e-12


@pytest.mark.parametrize("cap", [None, 2, 3])
@pytest.mark.parametrize("n_traj", [8, 12])
@pytest.mark.parametrize("p", [0.05, 0.5])
@pytest.mark.parametrize("name", SPECS)
def test_wg4_values(pkg, monkeypatch, name, p, n_traj, cap):
    plain, ref = _refs(pkg, monkeypatch, name, p)
    with monkeypatch.context() as m:
        _env(m, cap)
        with pkg.DtcEngine(0) as eng:
            got = eng.autocorr(_spec(pkg, name, p), n_traj, seed=SEED, traj_offset=OFF)
            count = eng.wavefront_count()
            eng.release_buffers()
    print(f"wavefront launches {count}")
    assert count > 0
    _assert_values(got, plain, ref, n_traj)


@pytest.mark.parametrize("cap", [None, 2, 3])
@pytest.mark.parametrize("p", [0.05, 0.5])
@pytest.mark.parametrize("name", SPECS)
def test_wg4_repeatable_and_batch_independent(pkg, monkeypatch, name, p, cap):
    plain, ref = _refs(pkg, monkeypatch, name, p)
    spec = _spec(pkg, name, p)
    with monkeypatch.context() as m:
        _env(m, cap)
        with pkg.DtcEngine(0) as eng:
            a = eng.autocorr(spec, 16, seed=SEED, traj_offset=OFF)
            b = eng.autocorr(spec, 16, seed=SEED, traj_offset=OFF)
            lo = eng.autocorr(spec, 8, seed=SEED, traj_offset=OFF)
            hi = eng.autocorr(spec, 8, seed=SEED, traj_offset=OFF + 8)
            count = eng.wavefront_count()
            eng.release_buffers()
    print(f"wavefront launches {count}")
    assert count > 0
    _assert_values(a, plain, ref, 16)
    for k in ("fwd", "echo"):
        assert np.array_equal(a[k], b[k]), k
        assert np.array_equal(a[k], np.concatenate([lo[k], hi[k]], axis=1)), k


@pytest.mark.parametrize("cap", [None, 2, 3])
def test_rx_vacuum_t10_plans_no_wavefront_pass(pkg, monkeypatch, cap):
    """Why the RX sweep above has T = 11: at T = 10 its echo chains are too
    short for the planner to save a launch (wf_replace, csrc/dtc_schedule.h), so
    no wavefront pass runs at any cap and `count > 0` could not hold there.  If
    this starts failing, the planner reaches T = 10 and the RX cases can move
    down to it."""
    with monkeypatch.context() as m:
        _env(m, cap)
        with pkg.DtcEngine(0) as eng:
            eng.autocorr(_spec(pkg, "rx_vacuum", 0.05, t=10), 8, seed=SEED, traj_offset=OFF)
            count = eng.wavefront_count()
            eng.release_buffers()
    assert count == 0
