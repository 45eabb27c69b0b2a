"""Pauli-frame kicks of the wavefront pass (csrc/dtc_wf_frame.h,
dtc_wavefront.hip) with a busy frame: p = 0.5 puts a Pauli after most
sub-gates, so all four butterfly variants of the standard records occur and
the frame's X and Z masks are rarely zero; g = 0.97 is form B by itself, g = 0.4
form A.  RX and RY kicks.  As tests/test_gpu_wavefront.py's _parity: L = 20,
T = 14; every case against the C oracle per trajectory at 1e-10 and against the
plain interior (DTC_NO_WAVEFRONT=1) at 1e-12 (echo) / 1e-13 (fwd), with
wavefront launches counted; at the default layer cap, at caps 2 and 3 (odd step
counts at steady state: the tile ends in layout 0), and with two octets whose
trajectory ids straddle 1023 | 1024.  The oracle and the plain run of a
(g, polarization, n) are computed once and shared.

Cap 2 lifts a tile's sites by two layers per pass, the plain rate, so its plan
never has fewer launches than the plain schedule (tools/wavefront_check.cpp
--table); the engine runs it all the same at that setting (wf_replace), which
makes DTC_WAVEFRONT=2 the switch for the two-step passes: one record row used,
the masks in the other."""
import numpy as np
import pytest

from oracle import c_oracle
from tests.helpers import random_disorder

pytestmark = pytest.mark.gpu

_REFS = {}


def _spec(pkg, g, pol):
    rng = np.random.default_rng(2024)
    hs, phis = random_disorder(rng, 20, 1)
    kw = {"polarization": "y"} if pol == "y" else {}
    return pkg.SweepSpec(L=20, T=14, hs=hs, phis=phis, g=g, noise_prob=0.5, **kw)


def _run(pkg, monkeypatch, spec, n, cap, **kw):
    """cap: None = the default wavefront interior, 0 = the plain interior"""
    with monkeypatch.context() as m:
        m.delenv("DTC_WAVEFRONT", raising=False)
        m.delenv("DTC_NO_WAVEFRONT", raising=False)
        if cap == 0:
            m.setenv("DTC_NO_WAVEFRONT", "1")
        elif cap:
            m.setenv("DTC_WAVEFRONT", str(cap))
        with pkg.DtcEngine(0) as eng:
            out = eng.autocorr(spec, n, **kw)
            count = eng.wavefront_count()
            eng.release_buffers()
    return out, count


def _refs(pkg, monkeypatch, g, pol, n, off):
    key = (g, pol, n, off)
    if key not in _REFS:
        spec = _spec(pkg, g, pol)
        plain, count = _run(pkg, monkeypatch, spec, n, 0, seed=95, traj_offset=off)
        assert count == 0
        ref = c_oracle.autocorr(spec, n, seed=95, traj_offset=off)
        for a in (*plain.values(), *ref.values()):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _REFS[key] = (plain, ref)
    return _REFS[key]


def _check(pkg, monkeypatch, g, pol, n, off, cap):
    plain, ref = _refs(pkg, monkeypatch, g, pol, n, off)
    got, count = _run(pkg, monkeypatch, _spec(pkg, g, pol), n, cap, seed=95, traj_offset=off)
    for k in ("fwd", "echo"):
        print(f"{k}: oracle {float(np.abs(got[k] - ref[k]).max()):.3e}  "
              f"plain {float(np.abs(got[k] - plain[k]).max()):.3e}")
    print(f"wavefront launches {count}")
    for k in ("fwd", "echo"):
        assert float(np.abs(got[k] - ref[k]).max()) < 1e-10, k
    assert float(np.abs(got["echo"] - plain["echo"]).max()) < 1e-12
    assert float(np.abs(got["fwd"] - plain["fwd"]).max()) < 1e-13
    assert count > 0


@pytest.mark.parametrize("cap", [None, 2, 3])
@pytest.mark.parametrize("pol", ["x", "y"])
@pytest.mark.parametrize("g", [0.97, 0.4])
def test_busy_frame_one_octet(pkg, monkeypatch, g, pol, cap):
    _check(pkg, monkeypatch, g, pol, 8, 0, cap)


@pytest.mark.parametrize("pol", ["x", "y"])
@pytest.mark.parametrize("g", [0.97, 0.4])
def test_busy_frame_two_octets_straddling_1024(pkg, monkeypatch, g, pol):
    _check(pkg, monkeypatch, g, pol, 16, 1016, None)
