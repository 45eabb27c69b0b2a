"""Bond noise (include/dtc.h dtc_bond_noise) without a GPU: the host sampler
``dtc_bond_draws``, the literal numpy model against the exact channel, the
engine's flip rules against the literal model, the facade, the CLI file name,
the calibration helper and the argument errors of ``dtc_autocorr_bond``.

Reference: Aer's ``depolarizing_error(p, 2)`` on ``["rzz"]`` next to
autocorr-delta-a-single-qiskit-fast.py:84-86, gate order of fast.py:111-121
(forward) and 140-143 (inverse).
"""
import ctypes

import numpy as np
import pytest

from tests import bond_model as bm
from tests.helpers import random_disorder


def _draws(pkg, p_bond, L, seed, traj, stream, counter):
    return pkg.engine.bond_draws(p_bond, L, seed, traj, stream, counter)


def test_draws_deterministic_and_independent_of_other_layers(pkg):
    L, seed = 9, 0xB07D
    a = _draws(pkg, 0.5, L, seed, 3, 0, 2)
    # other layers, trajectories and streams asked for in between
    for args in ((3, 0, 1), (3, 0, 3), (4, 0, 2), (3, 1, 2), (3, 7, 1)):
        _draws(pkg, 0.5, L, seed, *args)
    b = _draws(pkg, 0.5, L, seed, 3, 0, 2)
    assert a.shape == (L - 1,) and a.dtype == np.int32
    assert np.array_equal(a, b)
    assert np.all((a >= 0) & (a < 16))
    # layers differ from one another (8 bonds at p = 0.5: equal by chance ~ 1e-3 each)
    others = [_draws(pkg, 0.5, L, seed, 3, 0, c) for c in (1, 3, 4, 5)]
    assert any(not np.array_equal(a, o) for o in others)
    # a bond's draw does not depend on the other bonds' parameters
    pb = np.full(L - 1, 0.5)
    pb[0] = 0.0
    c = _draws(pkg, pb, L, seed, 3, 0, 2)
    assert c[0] == 0 and np.array_equal(c[1:], a[1:])
    # p = 0: never an error
    for t in range(50):
        assert not _draws(pkg, 0.0, L, seed, t, 0, 1).any()


@pytest.mark.parametrize("p", [0.3, 16.0 / 15.0])
def test_draw_frequencies(pkg, p):
    L = 32
    n_layers = 1300
    counts = np.zeros(16)
    for c in range(n_layers):
        codes = _draws(pkg, p, L, 0xF00D + 1, 11, 0, c)
        counts += np.bincount(codes, minlength=16)
    N = n_layers * (L - 1)
    q = np.full(16, p / 16.0)
    q[0] = 1.0 - 15.0 * p / 16.0
    f = counts / N
    assert np.all(np.abs(f - q) <= 5.0 * np.sqrt(q * (1.0 - q) / N)), (f, q)


@pytest.mark.parametrize("state", ["neel", "vacuum"])
def test_literal_model_matches_exact_channel(pkg, state):
    L, T, pb, N = 4, 4, 0.2, 4096
    rng = np.random.default_rng(41)
    hs, phis = random_disorder(rng, L)
    spec = pkg.SweepSpec(L=L, T=T, hs=hs, phis=phis, g=0.93, noise_prob=0.0, use_noise=0,
                         initial_state=state)
    ref_f, ref_e = bm.exact_sweep(L, T, spec.hs[0], spec.phis[0], spec.kick, pb, 0.0,
                                  spec.init_mask, spec.probe_site)
    acc_f, acc_e = np.zeros(T), np.zeros(T)
    seed = 0xC0FFEE
    for r in range(N):
        f, e, _ = bm.literal_trajectory(
            L, T, spec.hs[0], spec.phis[0], spec.kick, spec.init_mask, spec.probe_site,
            lambda s, c: _draws(pkg, pb, L, seed, r, s, c))
        acc_f += f
        acc_e += e
    bound = 5.0 / np.sqrt(N)  # every value has modulus <= 1
    assert np.abs(acc_f / N - ref_f).max() <= bound
    assert np.abs(acc_e / N - ref_e).max() <= bound
    # the channel does something at this strength (the bound is not vacuous)
    clean_f, clean_e = bm.exact_sweep(L, T, spec.hs[0], spec.phis[0], spec.kick, 0.0, 0.0,
                                      spec.init_mask, spec.probe_site)
    assert max(np.abs(clean_f - ref_f).max(), np.abs(clean_e - ref_e).max()) > 2 * bound


@pytest.mark.parametrize("L", [5, 6])
@pytest.mark.parametrize("inverse", [False, True])
def test_flip_rules_equal_literal_layer(L, inverse):
    rng = np.random.default_rng(100 + L)
    for _ in range(200):
        hs = rng.uniform(-np.pi, np.pi, L)
        phis = rng.uniform(-np.pi, np.pi, L - 1)
        codes = rng.integers(0, 16, L - 1)
        psi = rng.normal(size=1 << L) + 1j * rng.normal(size=1 << L)
        psi /= np.linalg.norm(psi)
        a = bm.literal_layer(psi, L, hs, phis, codes, inverse)
        b = bm.rule_layer(psi, L, hs, phis, codes, inverse)
        ph = np.vdot(b, a)
        assert abs(abs(ph) - 1.0) < 1e-12
        assert np.abs(a - ph * b).max() < 1e-12


def test_rule_trajectory_equals_literal(pkg):
    """Whole sweeps (kicks between the layers, the echo's first layer after
    P_t) with the rule layer in place of the literal one."""
    L, T = 5, 4
    rng = np.random.default_rng(5)
    hs, phis = random_disorder(rng, L)
    spec = pkg.SweepSpec(L=L, T=T, hs=hs, phis=phis, g=0.9, noise_prob=0.0, use_noise=0,
                         initial_state="neel")
    for r in range(8):
        def draw(s, c):
            return _draws(pkg, 0.6, L, 99, r, s, c)
        args = (L, T, spec.hs[0], spec.phis[0], spec.kick, spec.init_mask, spec.probe_site, draw)
        for x, y in zip(bm.literal_trajectory(*args), bm.literal_trajectory(*args,
                                                                           layer=bm.rule_layer)):
            assert np.abs(x - y).max() < 1e-12


def _dtc_circuit(pkg, L, n_fwd, hs, phis, g, echo=False):
    return pkg.circuit.dtc_circuit(L, n_fwd, hs, phis,
                                   lambda step: pkg.kicks.period_gate_specs("x", g, step),
                                   echo=echo)


def test_facade_accepts_two_qubit_error_on_rzz(pkg):
    aer = pkg.aer
    err2 = aer.depolarizing_error(0.03, 2)
    assert err2.num_qubits == 2 and err2.p == 0.03
    with pytest.raises(ValueError):
        aer.depolarizing_error(1.1, 2)
    with pytest.raises(NotImplementedError):
        aer.depolarizing_error(0.1, 3)
    nm = aer.NoiseModel()
    nm.add_all_qubit_quantum_error(aer.depolarizing_error(0.05, 1), ["u1", "u2", "u3"])
    nm.add_all_qubit_quantum_error(err2, ["rzz"])
    assert "rzz" in nm.noise_instructions and not nm.is_ideal()
    assert aer._noise_p(nm) == 0.05  # the single-qubit probability is unaffected
    for bad in (["cx"], ["rzz", "cx"], ["u3"], "cz"):
        with pytest.raises(NotImplementedError):
            aer.NoiseModel().add_all_qubit_quantum_error(err2, bad)
    rng = np.random.default_rng(2)
    hs, phis = random_disorder(rng, 4)
    circ = _dtc_circuit(pkg, 4, 2, hs[0], phis[0], 0.97, echo=True)
    f = aer.fold_circuit(circ, nm)
    assert f.bond_p == 0.03 and f.n_fwd == 2 and f.echo
    assert aer.fold_circuit(circ, aer.NoiseModel()).bond_p == 0.0
    only2 = aer.NoiseModel()
    only2.add_all_qubit_quantum_error(err2, ["rzz"])
    assert not only2.is_ideal() and aer._noise_p(only2) == 0.0
    assert aer.fold_circuit(circ, only2).bond_p == 0.03


def test_spec_and_refusals(pkg):
    rng = np.random.default_rng(3)
    hs, phis = random_disorder(rng, 5)
    base = dict(L=5, T=3, hs=hs, phis=phis)
    assert pkg.SweepSpec(**base).bond_noise is None
    assert not pkg.SweepSpec(**base).has_bond_noise
    s = pkg.SweepSpec(**base, bond_noise=0.01)
    assert s.bond_noise.shape == (4,) and np.all(s.bond_noise == 0.01) and s.has_bond_noise
    s = pkg.SweepSpec(**base, bond_noise=[0.0, 0.1, 0.0, 0.2])
    assert s.has_bond_noise
    assert not pkg.SweepSpec(**base, bond_noise=0.0).has_bond_noise
    for bad in (-0.1, 1.2, [0.1, 0.1]):
        with pytest.raises(ValueError):
            pkg.SweepSpec(**base, bond_noise=bad)
    # paths without bond noise refuse before touching a device
    eng = pkg.DtcEngine.__new__(pkg.DtcEngine)
    for call in (lambda: eng.energy(s, 2), lambda: eng.energy_sums(s, 2),
                 lambda: eng.prefix_build(s, 2, 1), lambda: eng.autocorr_prefixed(s, 2),
                 lambda: pkg.sharded.sharded_forward(None, s, 1),
                 lambda: pkg.sharded.sharded_forward_pipelined(None, s, 1),
                 lambda: pkg.sharded.loopback_forward_pipelined([None, None], s, 1)):
        with pytest.raises(NotImplementedError):
            call()
    eng._ctx = None


def test_cli_file_name(pkg):
    args = ("vacuum", 0.97, 20, 1, 30, 1, 0.0, 1.0, 0.05, 1)
    plain = ("autocorr_data_vacuum_g0.97_L20_inst1_tf30_randomphi1_delta0.0_amplitude1.0"
             "_noise0.05_usenoise1.csv")
    assert pkg.sweep.autocorr_csv_name(*args) == plain
    assert pkg.sweep.autocorr_csv_name(*args, bond_noise_prob=0.0) == plain
    assert pkg.sweep.autocorr_csv_name(*args, bond_noise_prob=0.01) == plain[:-4] + "_bond0.01.csv"
    ns = pkg.cli.build_parser().parse_args([])
    assert ns.bond_noise_prob == 0.0
    assert pkg.cli.build_parser().parse_args(["--bond_noise_prob", "0.02"]).bond_noise_prob == 0.02


def test_calibration_bond_noise(pkg):
    cal = pkg.DeviceCalibration(name="t", qubits=[], sx_gate_ns=35.0, cz_error=7e-3)
    p2 = 4.0 * 7e-3 / 3.0
    b = cal.bond_noise(6)
    assert b.shape == (5,) and np.allclose(b, 1.0 - (1.0 - p2) ** 2, rtol=0, atol=1e-15)
    assert np.allclose(cal.bond_noise(6, gates_per_rzz=1), p2, rtol=0, atol=1e-15)
    assert np.allclose(cal.bond_noise(3, gates_per_rzz=3), 1.0 - (1.0 - p2) ** 3, atol=1e-15)
    # composing depolarizing channels multiplies their (1 - p): check on a density matrix
    rho = np.diag([0.7, 0.1, 0.15, 0.05]).astype(complex)
    rho[0, 3] = rho[3, 0] = 0.1
    twice = bm._depol2(bm._depol2(rho, 2, 0, p2), 2, 0, p2)
    assert np.abs(twice - bm._depol2(rho, 2, 0, b[0])).max() < 1e-15
    assert pkg.SweepSpec(L=6, T=2, hs=np.zeros((1, 6)), phis=np.zeros((1, 5)),
                         bond_noise=b).has_bond_noise


def test_autocorr_bond_argument_errors(pkg):
    capi = pkg._capi
    lib = capi.load_library()
    rng = np.random.default_rng(4)
    hs, phis = random_disorder(rng, 5)
    spec = pkg.SweepSpec(L=5, T=3, hs=hs, phis=phis)
    pr = pkg.DtcEngine._problem(spec)
    nz = pkg.DtcEngine._noise(spec)
    out = np.zeros((1, 2, 3))

    def call(p_bond, problem=pr):
        bd = pkg.engine.bond_struct(np.ascontiguousarray(p_bond, dtype=np.float64))
        return lib.dtc_autocorr_bond(None, ctypes.byref(problem), ctypes.byref(nz), None,
                                     ctypes.byref(bd), ctypes.c_uint64(1), ctypes.c_int64(0),
                                     ctypes.c_int32(2), capi.as_dptr(out), capi.as_dptr(out),
                                     None)

    assert call(np.full(4, 0.1)) == -1
    assert b"ctx" in lib.dtc_last_error()
    for bad in (1.07, -0.01, float("nan")):
        pb = np.full(4, 0.1)
        pb[2] = bad
        assert call(pb) == -1
        assert b"p_bond" in lib.dtc_last_error()
    codes = np.zeros(4, dtype=np.int32)
    bd = pkg.engine.bond_struct(np.full(4, 2.0))
    assert lib.dtc_bond_draws(ctypes.byref(bd), 5, ctypes.c_uint64(1), ctypes.c_int64(0), 0, 1,
                              codes.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))) == -1
    with pytest.raises(capi.DtcError):
        pkg.engine.bond_draws(np.full(4, 2.0), 5, 1, 0, 0, 1)
