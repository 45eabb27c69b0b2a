"""dtc_apply_periods against the C oracle, amplitude for amplitude.

test_gpu_parity.py::test_apply_periods_random_state compares a state vector
with the oracle at six sizes, always with general kicks ("xy") and p = 0.1.
This file takes its bounds -- 1e-12 for the state, global phase included, and
1e-11 for the [norm, Z_i] row -- to what it leaves out:

  * the factored RX / RY forms, whose Pauli-frame records carry a global factor
    and a power of i that no observable shows (an autocorrelator or a forward /
    inverse round trip cancels a wrong one);
  * every site-group plan of tests/plan_table.py from one site to three groups;
  * single periods (a chain of one layer starts and ends in the same pass);
  * noiseless kicks (identity frames).

The hook's contract is the state itself, so nothing here compares up to a phase.
"""
import functools

import numpy as np
import pytest

from oracle import c_oracle
from tests.helpers import random_disorder
from tests.plan_table import plan_id

pytestmark = pytest.mark.gpu
KINDS = ("x", "y", "circular_left")
SIZES = (1, 3, 7, 11, 13, 15, 16, 17, 19, 21, 22, 23, 24)


@functools.lru_cache(maxsize=2)
def _random_state(L):
    """One random normalised state per size, shared by that size's cases (which
    run next to each other) and never written to."""
    rng = np.random.default_rng(900 + L)
    psi = rng.normal(size=1 << L) + 1j * rng.normal(size=1 << L)
    psi /= np.linalg.norm(psi)
    psi.flags.writeable = False
    return psi


def _check(pkg, engine, L, pol, inverse, first, n_periods, noiseless=False):
    rng = np.random.default_rng(L + 7 * inverse)
    hs, phis = random_disorder(rng, L, 2)
    kw = dict(noise_prob=0.0, use_noise=0) if noiseless else dict(noise_prob=0.1)
    spec = pkg.SweepSpec(L=L, T=5, hs=hs, phis=phis, g=0.97, polarization=pol, **kw)
    psi = _random_state(L)
    args = dict(inverse=inverse, inst=1, traj=11, stream=4, seed=99)
    ga, gz = engine.apply_periods(spec, psi, first, n_periods, **args)
    oa, oz = c_oracle.apply_periods(spec, psi, first, n_periods, **args)
    assert np.abs(oa - psi).max() > 0.1 * np.abs(psi).max()  # (the periods do something)
    err_a, err_z = float(np.abs(ga - oa).max()), float(np.abs(gz - oz).max())
    print(f"L={L} {pol} inverse={inverse}: state {err_a:.3e}, [norm, Z_i] {err_z:.3e}")
    assert err_a < 1e-12
    assert err_z < 1e-11


def _id(L, pol, inverse, extra=""):
    return "-".join(filter(None, [plan_id(L), pol, "inverse" if inverse else "forward", extra]))


@pytest.mark.parametrize("L,pol,inverse", [
    pytest.param(L, pol, inv, id=_id(L, pol, inv))
    for L in SIZES for pol in KINDS for inv in (False, True)])
def test_three_periods_match_oracle(pkg, engine, L, pol, inverse):
    """Forward periods 2, 3, 4; inverse periods 3, 2, 1 (as the existing test)."""
    _check(pkg, engine, L, pol, inverse, 3 if inverse else 2, 3)


@pytest.mark.parametrize("L,pol,inverse", [
    pytest.param(L, pol, inv, id=_id(L, pol, inv, "single"))
    for L in (11, 14, 17, 18, 22) for pol in KINDS for inv in (False, True)])
def test_single_period_matches_oracle(pkg, engine, L, pol, inverse):
    """One period each way on one, two and three site groups (10 + 4 and 10 + 8
    sites among them, which the three-period sizes leave to the existing test)."""
    _check(pkg, engine, L, pol, inverse, 3 if inverse else 2, 1)


@pytest.mark.parametrize("L,pol,inverse", [
    pytest.param(L, pol, inv, id=_id(L, pol, inv, "noiseless"))
    for L in (12, 17, 20, 22) for pol in ("x", "y") for inv in (False, True)])
def test_noiseless_periods_match_oracle(pkg, engine, L, pol, inverse):
    """p = 0 (use_noise = 0): every Pauli frame is the identity."""
    _check(pkg, engine, L, pol, inverse, 3 if inverse else 2, 3, noiseless=True)
