"""The re-layout chain of the wavefront pass (csrc/dtc_wavefront.hip): the column
tile (tile 2) snakes between layouts 2 and 1 only, kicks its nibble-0 site 11
across lanes (wf_kick_lane3) and applies its odd steps' diagonals in layout 1
from the register / thread table pair of csrc/dtc_wf_frame.h; tile 1 keeps the
three-layout snake, whose 1 <-> 0 re-layouts stay inside a wave and may run
without workgroup barriers (csrc/dtc_device.h exchange, WAVE).

The wavefront interior only exists at L = 20 with the octet layout, so the
shapes are tests/test_gpu_wavefront.py's: T = 14, 8 trajectories (one octet) and
16 whose ids straddle 1023 | 1024.  RX kicks from the vacuum and RY kicks from
the Neel state with t_offset = 1 (the lane-signed cross-lane kick), at p = 0.05
and at p = 0.5 (busy Pauli frames: the layout-1 tables staged under nonzero X
and Z masks); at the default layer cap and at caps 2 and 3, so passes with even
and with odd step counts occur (an odd count ends tile 2 in layout 1 and tile 1
in layout 0).

Values: the C oracle per trajectory at 1e-10 and the plain interior
(DTC_NO_WAVEFRONT=1) at 1e-12 (echo) / 1e-13 (fwd), the tolerances of
tests/test_gpu_wavefront.py, with wavefront launches counted.  The oracle and
the plain run of a spec are computed once for the 16 trajectories and shared
(the one-octet cases take the first eight).

Races: a barrier that was needed shows as run-to-run differences, so the same
call twice in one engine is bit-identical, and one batch of 16 is bit-identical
to two batches of 8 at offsets 1016 and 1024 (a state's arithmetic does not
depend on its batch, and the two shapes schedule the workgroups differently)."""
import numpy as np
import pytest

from oracle import c_oracle
from tests.helpers import random_disorder

pytestmark = pytest.mark.gpu

OFF = 1016
SEED = 96
SPECS = ["rx_vacuum", "ry_neel"]
_REFS = {}


def _spec(pkg, name, p):
    rng = np.random.default_rng(2025)
    hs, phis = random_disorder(rng, 20, 1)
    if name == "rx_vacuum":
        return pkg.SweepSpec(L=20, T=14, hs=hs, phis=phis, g=0.97, noise_prob=p,
                             initial_state="vacuum")
    return pkg.SweepSpec(L=20, T=14, hs=hs, phis=phis, g=0.93, noise_prob=p,
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


def _assert_values(got, plain, ref, lo, hi):
    for k in ("fwd", "echo"):
        print(f"{k}: oracle {float(np.abs(got[k] - ref[k][:, lo:hi]).max()):.3e}  "
              f"plain {float(np.abs(got[k] - plain[k][:, lo:hi]).max()):.3e}")
    for k in ("fwd", "echo"):
        assert float(np.abs(got[k] - ref[k][:, lo:hi]).max()) < 1e-10, k
    assert float(np.abs(got["echo"] - plain["echo"][:, lo:hi]).max()) < 1e-12
    assert float(np.abs(got["fwd"] - plain["fwd"][:, lo:hi]).max()) < 1e-13


@pytest.mark.parametrize("cap", [None, 2, 3])
@pytest.mark.parametrize("p", [0.05, 0.5])
@pytest.mark.parametrize("name", SPECS)
def test_chain_one_octet(pkg, monkeypatch, name, p, cap):
    plain, ref = _refs(pkg, monkeypatch, name, p)
    with monkeypatch.context() as m:
        _env(m, cap)
        with pkg.DtcEngine(0) as eng:
            got = eng.autocorr(_spec(pkg, name, p), 8, seed=SEED, traj_offset=OFF)
            count = eng.wavefront_count()
            eng.release_buffers()
    print(f"wavefront launches {count}")
    _assert_values(got, plain, ref, 0, 8)
    assert count > 0


@pytest.mark.parametrize("cap", [None, 3])
@pytest.mark.parametrize("p", [0.05, 0.5])
@pytest.mark.parametrize("name", SPECS)
def test_chain_repeatable_and_batch_independent(pkg, monkeypatch, name, p, cap):
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
    _assert_values(a, plain, ref, 0, 16)
    assert count > 0
    for k in ("fwd", "echo"):
        assert np.array_equal(a[k], b[k]), k
        assert np.array_equal(a[k], np.concatenate([lo[k], hi[k]], axis=1)), k
