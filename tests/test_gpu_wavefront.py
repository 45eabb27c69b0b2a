"""Wavefront interior of the echo chains (csrc/dtc_wavefront.h, dtc_wavefront.hip).

By default the run of plain stored K-D-K passes between an echo
chain's first pass and its light-cone end is replaced by deeper passes over two
tiles that share site 11 (index bits 0..11; three column bits + sites 11..19).
Any order that keeps the three-point stencil dependencies is the same operator
(DESIGN.md section 4), so: the C oracle per trajectory at 1e-10, the plain
schedule (DTC_NO_WAVEFRONT=1) at 1e-12 (echo) / 1e-13 (fwd), fewer stored
passes, and the plain schedule wherever the conditions do not hold (no octet
layout, L != 20).  T = 14 gives interior runs of up to 6 plain passes: both
parities, both entry frontiers, both ramps.
"""
import json
import os

import numpy as np
import pytest

from oracle import c_oracle
from tests.helpers import random_disorder

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(pkg, monkeypatch, spec, n, wavefront, **kw):
    with monkeypatch.context() as m:
        m.delenv("DTC_WAVEFRONT", raising=False)
        m.delenv("DTC_NO_WAVEFRONT", raising=False)
        if not wavefront:
            m.setenv("DTC_NO_WAVEFRONT", "1")
        with pkg.DtcEngine(0) as eng:
            eng.set_profiling(True)
            out = eng.autocorr(spec, n, **kw)
            lo = eng.kernel_stats()[pkg._capi.KERNEL_LO_PASS]
            count = eng.wavefront_count()
            eng.release_buffers()
    return out, lo, count


def _parity(pkg, monkeypatch, spec, n, **kw):
    got, lo, count = _run(pkg, monkeypatch, spec, n, True, **kw)
    plain, lo_plain, count_plain = _run(pkg, monkeypatch, spec, n, False, **kw)
    ref = c_oracle.autocorr(spec, n, **kw)
    for k in ("fwd", "echo"):
        err = float(np.abs(got[k] - ref[k]).max())
        print(f"{k}: oracle {err:.3e}  plain {float(np.abs(got[k] - plain[k]).max()):.3e}")
    print(f"wavefront launches {count}; stored passes {lo['launches']} (plain {lo_plain['launches']})")
    for k in ("fwd", "echo"):
        assert float(np.abs(got[k] - ref[k]).max()) < 1e-10, k
    assert float(np.abs(got["echo"] - plain["echo"]).max()) < 1e-12
    assert float(np.abs(got["fwd"] - plain["fwd"]).max()) < 1e-13
    assert count > 0 and count_plain == 0
    assert lo["launches"] < lo_plain["launches"]
    # a wavefront launch is booked like a plain one: 32 B per amplitude
    saved = lo_plain["launches"] - lo["launches"]
    assert lo_plain["bytes"] - lo["bytes"] == pytest.approx(saved * 32.0 * n * (1 << 20))


@pytest.mark.parametrize("n,off", [(8, 0), (16, 1016)])
def test_wavefront_rx_matches_oracle_and_plain(pkg, monkeypatch, n, off):
    """RX kicks, p = 0.05, T = 14: one octet, and two octets whose trajectory
    ids straddle 1023 | 1024."""
    rng = np.random.default_rng(2014)
    hs, phis = random_disorder(rng, 20, 1)
    spec = pkg.SweepSpec(L=20, T=14, hs=hs, phis=phis, g=0.97, noise_prob=0.05)
    _parity(pkg, monkeypatch, spec, n, seed=91, traj_offset=off)


def test_wavefront_ry_neel_t_offset(pkg, monkeypatch):
    rng = np.random.default_rng(2015)
    hs, phis = random_disorder(rng, 20, 1)
    spec = pkg.SweepSpec(L=20, T=14, hs=hs, phis=phis, g=0.93, noise_prob=0.05,
                         polarization="y", initial_state="neel", t_offset=1)
    _parity(pkg, monkeypatch, spec, 8, seed=92, traj_offset=1016)


def test_wavefront_noiseless(pkg, monkeypatch):
    rng = np.random.default_rng(2016)
    hs, phis = random_disorder(rng, 20, 1)
    spec = pkg.SweepSpec(L=20, T=14, hs=hs, phis=phis, g=0.97, noise_prob=0.0, use_noise=0)
    _parity(pkg, monkeypatch, spec, 8, seed=93)


@pytest.mark.parametrize("L,n", [(20, 3), (21, 8)])
def test_wavefront_fallback(pkg, monkeypatch, L, n):
    """No octet layout (B = 3) or L = 21: the plain schedule runs, and the
    results are the oracle's."""
    rng = np.random.default_rng(2017 + L)
    hs, phis = random_disorder(rng, L, 1)
    spec = pkg.SweepSpec(L=L, T=10, hs=hs, phis=phis, g=0.97, noise_prob=0.05)
    got, _, count = _run(pkg, monkeypatch, spec, n, True, seed=94)
    assert count == 0
    ref = c_oracle.autocorr(spec, n, seed=94)
    for k in ("fwd", "echo"):
        assert float(np.abs(got[k] - ref[k]).max()) < 1e-10, k


def test_wavefront_headline_shape(pkg, monkeypatch, engine):
    """The headline batch once (L = 20, T = 30, p = 0.05, B = 1024, ids from
    0): trajectories 0, 7, 8 and 1023 equal the fused oracle at 1e-10."""
    import torch

    engine.release_buffers()
    torch.cuda.empty_cache()
    with open(os.path.join(ROOT, "tests", "golden", "disorder.json")) as f:
        d = json.load(f)["L20"]
    spec = pkg.SweepSpec(L=20, T=30, hs=np.array(d["hs"][:1]), phis=np.array(d["phis"][:1]),
                         g=0.97, noise_prob=0.05, use_noise=1, initial_state="vacuum")
    seed = 0x5EED0001
    got, _, count = _run(pkg, monkeypatch, spec, 1024, True, seed=seed, traj_offset=0,
                         batch=1024)
    assert count > 0
    for lo, hi in ((0, 1), (7, 9), (1023, 1024)):
        ref = c_oracle.autocorr_fused(spec, hi - lo, seed=seed, traj_offset=lo)
        for i in range(hi - lo):
            for k in ("fwd", "echo"):
                err = float(np.abs(got[k][0, lo + i] - ref[k][0, i]).max())
                assert err < 1e-10, (k, lo + i, err)
