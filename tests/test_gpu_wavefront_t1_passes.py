"""Tile 1's wavefront passes of every length (csrc/dtc_wavefront.hip): the
layout-0 diagonals read their register table from LDS in rows of 17
(dtc_wf_frame.h, wf_pad0), and the same shapes are what the swap form
(-DDTC_WF_T1_SWAP=1, off in the product) has to get right, so the test runs
against whichever form the library was built with and prints which.

L = 20 (the wavefront interior exists only there), 16 trajectories, p = 0.05,
seed and disorder row of tests/test_gpu_wavefront_wg4.py; trajectory offsets 0
and 8 (an octet edge inside the batch).  RX kicks from the vacuum and RY kicks
from the Neel state.  T = 14 at the default cap: tile-1 passes of 1, 2, 3 and 4
steps (the schedule dump of tools/schedule_check.cpp is asked for exactly that,
and the engine's launch count must be the dump's); T = 11 at the default cap
and at caps 2 and 3 (two- and three-step passes, odd and even endings).  No
schedule of these sizes gives tile 1 a trailing kick-less diagonal (the dump is
asked for that too): with the probe on site 10 it does not occur.  A moved probe
gives it after 1, 3 and 4 kick steps, and tests/test_gpu_wavefront_inputs.py runs
those passes on the GPU under RX and RY kicks (the CPU models of that path:
tools/wavefront_frame_check.cpp, tools/wavefront_t1_swap_check.cpp).

Values: the C oracle per trajectory at 1e-10; the plain interior
(DTC_NO_WAVEFRONT=1): fwd identical, echo within 1e-12, the project's bound
between schedules.  The oracle and the plain run of a (kicks, T) pair are
computed once for trajectories 0 .. 23 and shared."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from oracle import c_oracle
from tests.helpers import random_disorder
from tests.test_schedule_cpu import WF_SHAPE, build, parse

pytestmark = pytest.mark.gpu

SEED = 2110
N_TRAJ = 16
OFFSETS = (0, 8)
CASES = [(14, None), (11, None), (11, 2), (11, 3)]
_REFS = {}


def _spec(pkg, kind, T):
    rng = np.random.default_rng(410)
    hs, phis = random_disorder(rng, 20, 1)
    if kind == "rx":
        return pkg.SweepSpec(L=20, T=T, hs=hs, phis=phis, g=0.97, noise_prob=0.05,
                             initial_state="vacuum")
    return pkg.SweepSpec(L=20, T=T, hs=hs, phis=phis, g=0.93, noise_prob=0.05,
                         polarization="y", initial_state="neel")


def _env(m, cap):
    """cap: None = the default wavefront interior, 0 = the plain interior"""
    m.delenv("DTC_WAVEFRONT", raising=False)
    m.delenv("DTC_NO_WAVEFRONT", raising=False)
    if cap == 0:
        m.setenv("DTC_NO_WAVEFRONT", "1")
    elif cap:
        m.setenv("DTC_WAVEFRONT", str(cap))


def _refs(pkg, monkeypatch, kind, T):
    """(plain interior, C oracle) of trajectories 0 .. 23, read-only"""
    key = (kind, T)
    if key not in _REFS:
        spec = _spec(pkg, kind, T)
        n = max(OFFSETS) + N_TRAJ
        with monkeypatch.context() as m:
            _env(m, 0)
            with pkg.DtcEngine(0) as eng:
                plain = eng.autocorr(spec, n, seed=SEED, traj_offset=0)
                assert eng.wavefront_count() == 0
                eng.release_buffers()
        ref = c_oracle.autocorr(spec, n, seed=SEED, traj_offset=0)
        for a in (*plain.values(), *ref.values()):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _REFS[key] = (plain, ref)
    return _REFS[key]


@pytest.fixture(scope="module")
def sched_exe(tmp_path_factory):
    return build(tmp_path_factory.mktemp("t1_sched"), [])


def _tile1_passes(sched_exe, kind, T, cap):
    """(all wavefront launches, the set of (steps, trailing diagonal) of tile 1's)"""
    args = ["T=%d" % T, "kick=%s" % ("x" if kind == "rx" else "y")]
    if cap:
        args.append("wf_cap=%d" % cap)
    r = subprocess.run([sched_exe, *args], capture_output=True, text=True, check=True)
    wf = [l["wf"] for l in parse(r.stdout) if l["shape"] == WF_SHAPE]
    return len(wf), {(w[0], (w[2] >> w[0]) & 1) for w in wf if w[1] == 0}


def test_build_form_is_reported(pkg):
    """The library says which program tile 1 runs (a data symbol of
    csrc/dtc_wavefront.hip); the product's is the three-layout snake."""
    lib = ctypes.CDLL(os.environ.get("DTC_LIB", pkg._capi.LIB_PATH))
    form = ctypes.c_int.in_dll(lib, "dtc_wf_t1_swap_form").value
    print("tile 1 swap form:", form)
    assert form in (0, 1)


@pytest.mark.parametrize("off", OFFSETS)
@pytest.mark.parametrize("T,cap", CASES)
@pytest.mark.parametrize("kind", ["rx", "ry"])
def test_tile1_pass_lengths(pkg, monkeypatch, sched_exe, kind, T, cap, off):
    n_wf, t1 = _tile1_passes(sched_exe, kind, T, cap)
    print("wavefront launches", n_wf, "tile-1 (steps, trailing):", sorted(t1))
    want = {(14, None): {1, 2, 3, 4}, (11, None): {2, 4}, (11, 2): {2}, (11, 3): {3}}[(T, cap)]
    assert {s for s, _ in t1} == want
    assert not any(tr for _, tr in t1)
    plain, ref = _refs(pkg, monkeypatch, kind, T)
    with monkeypatch.context() as m:
        _env(m, cap)
        with pkg.DtcEngine(0) as eng:
            got = eng.autocorr(_spec(pkg, kind, T), N_TRAJ, seed=SEED, traj_offset=off)
            count = eng.wavefront_count()
            eng.release_buffers()
    assert count == n_wf
    sl = slice(off, off + N_TRAJ)
    errs = {k: (float(np.abs(got[k] - ref[k][:, sl]).max()),
                float(np.abs(got[k] - plain[k][:, sl]).max())) for k in ("fwd", "echo")}
    for k, (eo, ep) in errs.items():
        print(f"{k}: oracle {eo:.3e}  plain {ep:.3e}")
    for k in ("fwd", "echo"):
        assert errs[k][0] < 1e-10, k
    assert errs["fwd"][1] == 0.0
    assert errs["echo"][1] <= 1e-12
