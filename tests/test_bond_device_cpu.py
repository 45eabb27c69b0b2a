"""Bond noise with noisy kicks and in the energy path, without a GPU: the host
sampler of the kick draws (dtc_kick_draws), the literal gate-by-gate model of
tests/bond_device_model.py against the C oracle, the observable sign rules of
the energy path, the factored form of the device-noise kick with the outgoing
Pauli as its right factor, the exact channel, and the Python plumbing.
"""
import ctypes

import numpy as np
import pytest

from oracle import c_oracle, energy_oracle
from tests import bond_device_model as bdm
from tests import bond_model as bm
from tests.helpers import random_disorder


def harsh_device(pkg, L):
    return pkg.DeviceNoise(p_gate=np.full(L, 0.02), t1_us=np.linspace(1.5, 3.0, L),
                           t2_us=np.linspace(1.0, 4.0, L), gate_ns=120.0, anc_factor=0.9,
                           readout_p01=0.02, readout_p10=0.035)


def _spec(pkg, L, T, pol, noise, seed=5, n_inst=1, **kw):
    rng = np.random.default_rng(100 * L + seed)
    hs, phis = random_disorder(rng, L, n_inst)
    extra = dict(device=harsh_device(pkg, L)) if noise == "device" else dict(noise_prob=0.05)
    return pkg.SweepSpec(L=L, T=T, hs=hs, phis=phis, g=0.93, polarization=pol,
                         initial_state="neel", **extra, **kw)


def _draws(pkg, spec, seed, traj, p_bond=None):
    return bdm.Draws(pkg, spec.L, spec.n_sub, seed, traj, p=spec.p, device=spec.device,
                     p_bond=p_bond)


def _autocorr_row(pkg, spec, inst, draws):
    dev = spec.device
    fac = dev.anc_factor if dev is not None else (1.0 - spec.p) ** pkg.N_ANCILLA_NOISY_GATES
    ro = ((1.0 - dev.readout_p01 - dev.readout_p10, dev.readout_p10 - dev.readout_p01)
          if dev is not None else (1.0, 0.0))
    return bdm.literal_autocorr(spec.L, spec.T, spec.hs[inst], spec.phis[inst], spec.kick,
                                spec.init_mask, spec.probe_site, draws, fac, ro)


# ---- 2. the literal model against the C oracle (bond noise off) -----------------
@pytest.mark.parametrize("noise", ["depol", "device"])
@pytest.mark.parametrize("L,pol", [(4, "x"), (5, "xy"), (5, "x"), (4, "xy")])
def test_literal_model_matches_c_oracle(pkg, L, pol, noise):
    T, n_traj, seed = 4, 5, 21
    spec = _spec(pkg, L, T, pol, noise)
    ref = c_oracle.autocorr(spec, n_traj, seed=seed, want_zsite=True)
    jumps = 0
    for r in range(n_traj):
        d = _draws(pkg, spec, seed, r)
        f, e, z = _autocorr_row(pkg, spec, 0, d)
        for got, key in ((f, "fwd"), (e, "echo"), (z, "zsite")):
            assert np.abs(got - ref[key][0, r]).max() < 1e-12, (key, r)
        ez, ezz, ex = energy_oracle.trajectory_energy(spec, 0, r, seed=seed)
        gz, gzz, gx = bdm.literal_energy(L, T, spec.hs[0], spec.phis[0], spec.kick,
                                         spec.init_mask, d)
        assert max(np.abs(gz - ez).max(), np.abs(gzz - ezz).max(), np.abs(gx - ex).max()) < 1e-12
        jumps += sum(int(d.kick(s, c)[1].sum()) for s, c in [(0, t) for t in range(1, T)])
    if noise == "device":
        assert jumps > 0  # the harsh device's amplitude-damping jumps are exercised


# ---- 3. dtc_kick_draws ------------------------------------------------------------
def test_kick_draws(pkg):
    L, n_sub, seed = 6, 2, 77
    kd = pkg.engine.kick_draws
    a = kd(L, n_sub, seed, 3, 0, 2, p=0.3)
    b = pkg.DtcEngine.kick_draws(L, n_sub, seed, 3, 0, 2, p=0.3)
    assert np.array_equal(a[0], b[0]) and a[0].shape == (L, n_sub) and not a[1].any()
    seen = set()
    for traj in range(4):
        for stream, counter in [(0, 1), (0, 2), (3, 1), (bdm.STREAM_PREP, 0)]:
            pauli, _ = kd(L, n_sub, seed, traj, stream, counter, p=0.3)
            for i in range(L):
                for q in range(n_sub):
                    want = c_oracle.sample_pauli(0.3, seed, traj, stream, counter, i, q)
                    assert pauli[i, q] == want
                    seen.add(int(want))
    assert seen == {0, 1, 2, 3}
    assert not kd(L, n_sub, seed, 0, 0, 1, p=0.0)[0].any()
    # device-like draws: deterministic, jumps present, none for the preparation
    dev = harsh_device(pkg, L)
    p1, j1 = kd(L, 1, seed, 1, 0, 1, device=dev)
    p2, j2 = kd(L, 1, seed, 1, 0, 1, device=dev)
    assert np.array_equal(p1, p2) and np.array_equal(j1, j2)
    assert sum(int(kd(L, 1, seed, r, 0, 1, device=dev)[1].sum()) for r in range(40)) > 0
    assert not any(kd(L, 1, seed, r, bdm.STREAM_PREP, 0, device=dev)[1].any() for r in range(40))
    # the neel preparation of the C oracle under device noise follows these draws
    spec = _spec(pkg, L, 2, "x", "device")
    for r in range(20):
        assert _draws(pkg, spec, seed, r).prep_mask(spec.init_mask) == c_oracle.init_mask(
            spec, seed, r)
    # the bond sampler is untouched by it
    before = pkg.engine.bond_draws(0.4, L, seed, 1, 0, 1)
    kd(L, 1, seed, 1, 0, 1, p=0.3)
    assert np.array_equal(before, pkg.engine.bond_draws(0.4, L, seed, 1, 0, 1))
    with pytest.raises(ValueError):
        kd(L + 1, 1, seed, 0, 0, 1, device=dev)


def test_kick_draws_argument_errors(pkg):
    lib = pkg._capi.load_library()
    nz = pkg._capi.DtcNoise()
    nz.p = 0.1
    buf = (ctypes.c_int32 * 8)()
    args = (ctypes.c_uint64(1), ctypes.c_int64(0), ctypes.c_uint32(0), ctypes.c_uint32(1))
    assert lib.dtc_kick_draws(None, None, 4, 2, *args, buf, None) == -1
    assert b"null" in lib.dtc_last_error()
    assert lib.dtc_kick_draws(ctypes.byref(nz), None, 4, 2, *args, None, None) == -1
    assert lib.dtc_kick_draws(ctypes.byref(nz), None, 4, 2, *args, buf, None) == 0  # jump nullable
    assert lib.dtc_kick_draws(ctypes.byref(nz), None, 40, 2, *args, buf, None) == -1
    assert lib.dtc_kick_draws(ctypes.byref(nz), None, 4, 9, *args, buf, None) == -1
    assert lib.dtc_kick_draws(ctypes.byref(nz), None, 4, 2, ctypes.c_uint64(1),
                              ctypes.c_int64(-1), 0, 1, buf, None) == -1
    nz.p = 2.0
    assert lib.dtc_kick_draws(ctypes.byref(nz), None, 4, 2, *args, buf, None) == -1
    # the new energy entry points reject a null context and a bad p_bond before any device call
    spec = _spec(pkg, 5, 3, "x", "depol")
    pr = pkg.DtcEngine._problem(spec)
    nz = pkg.DtcEngine._noise(spec)
    out = np.zeros((1, 2, 3, 5))
    for fn in (lib.dtc_energy_bond, lib.dtc_energy_sums_bond):
        for pb, word in ((np.full(4, 0.1), b"null"), (np.full(4, 1.07), b"p_bond")):
            bd = pkg.engine.bond_struct(pb)
            assert fn(None, ctypes.byref(pr), ctypes.byref(nz), None, ctypes.byref(bd),
                      ctypes.c_uint64(1), ctypes.c_int64(0), ctypes.c_int32(2),
                      pkg._capi.as_dptr(out), pkg._capi.as_dptr(out),
                      pkg._capi.as_dptr(out)) == -1
            assert word in lib.dtc_last_error()


# ---- 4. the observable sign rules -----------------------------------------------
def test_observable_sign_rules():
    L = 4
    rng = np.random.default_rng(8)
    psi = rng.normal(size=1 << L) + 1j * rng.normal(size=1 << L)
    psi /= np.linalg.norm(psi)
    before = bdm.observables(psi, L)
    assert min(np.abs(v).min() for v in before) > 1e-3  # no sign is hidden by a zero
    cases = []
    for bond in range(L - 1):  # both edge bonds and the interior one
        for code in range(16):
            codes = np.zeros(L - 1, dtype=np.int32)
            codes[bond] = code
            cases.append(codes)
    cases += [rng.integers(0, 16, L - 1).astype(np.int32) for _ in range(64)]  # merged Paulis
    for codes in cases:
        want = bdm.observables(bdm.apply_outgoing(psi.copy(), L, codes), L)
        got = bdm.sign_rules(L, codes, *before)
        for g, w in zip(got, want):
            assert np.abs(g - w).max() < 1e-12, codes


# ---- 5. the factored form with the outgoing Pauli as the right factor -----------------
X = np.array([[0, 1], [1, 0]], complex)
Y = np.array([[0, -1j], [1j, 0]])
Z = np.diag([1.0, -1.0]).astype(complex)
I2 = np.eye(2, dtype=complex)


def rx(th):
    c, s = np.cos(th / 2), np.sin(th / 2)
    return np.array([[c, -1j * s], [-1j * s, c]])


def ry(th):
    c, s = np.cos(th / 2), np.sin(th / 2)
    return np.array([[c, -s], [s, c]], complex)


def canonicalise(kind, m):
    """(k, w, rho0, rho1, coef, form_b) as csrc/dtc_kernels.hip canonicalise computes
    them for kKindRXU / kKindRYU."""
    m = m.flatten()
    if kind == "rx":
        a_form = m[0].imag == 0 and m[1].real == 0 and m[2].real == 0 and m[3].imag == 0
        a = m[0].real if a_form else m[0].imag
        b = m[1].imag if a_form else -m[1].real
        c = m[2].imag if a_form else -m[2].real
        d = m[3].real if a_form else m[3].imag
        k = 0 if a_form else 1
    else:
        real = all(v.imag == 0 for v in m)
        a, b, c, d = [(v.real if real else v.imag) for v in m]
        k = 0 if real else 1
    is_rx = kind == "rx"
    if a != 0 or b != 0:
        form_b = abs(a) < abs(b)
        w = b if form_b else a
        coef = a / b if form_b else b / a
        rho0 = 1.0
        rho1 = ((c / b if is_rx else -c / b) if form_b else d / a)
    elif c != 0 or d != 0:
        form_b = abs(d) < abs(c)
        w = (c if is_rx else -c) if form_b else d
        coef = d / w if form_b else (c / d if is_rx else -c / d)
        rho0, rho1 = 0.0, 1.0
    else:
        return k, 0.0, 0.0, 0.0, 0.0, False
    return k, w, rho0, rho1, coef, form_b


def rebuild(kind, k, w, rho0, rho1, coef, form_b):
    if kind == "rx":
        s = (np.array([[coef, 1j], [1j, coef]]) if form_b
             else np.array([[1, 1j * coef], [1j * coef, 1]]))
    else:
        s = (np.array([[coef, 1], [-1, coef]], complex) if form_b
             else np.array([[1, coef], [-coef, 1]], complex))
    return (1j ** k) * w * np.diag([rho0, rho1]) @ s


@pytest.mark.parametrize("kind", ["rx", "ry"])
def test_device_kick_with_outgoing_pauli_factors(kind):
    """Pauli . Kraus . G . P_0 (build_site_kick with bond_on under device noise:
    P_0 first, then the gate, the Kraus factor and the drawn Pauli) keeps the
    form i^k w diag(rho0, rho1) S, and so does the pure-Pauli kick."""
    rng = np.random.default_rng(17)
    gate = rx if kind == "rx" else ry
    paulis = [I2, X, Y, Z]
    worst = 0.0
    for p0 in paulis:
        for p1 in paulis:
            for jump in (False, True):
                for inverse in (False, True):
                    for _ in range(40):
                        g = gate(rng.uniform(0.1, 2 * np.pi - 0.1))
                        if inverse:
                            g = g.conj().T
                        a0, a1, b = rng.uniform(0.3, 1.5, 3)
                        kraus = np.array([[0, b], [0, 0]]) if jump else np.diag([a0, a1])
                        # the order of the kernel's products: m = P_0; m = G m; Kraus; Pauli
                        m = p1 @ (kraus @ (g @ p0))
                        parts = canonicalise(kind, m)
                        worst = max(worst, float(np.abs(rebuild(kind, *parts) - m).max()))
        # kKickBondPauli: the Pauli alone (and the merged pair of two bonds)
        for p1 in paulis:
            m = p1 @ p0
            # the kernel merges codes with pauli_left, phases included: Y Y = I, X Z = -i Y ...
            parts = canonicalise(kind, m)
            assert parts[1] != 0.0
            worst = max(worst, float(np.abs(rebuild(kind, *parts) - m).max()))
    assert worst < 1e-14, worst


# ---- 6. the exact channel ---------------------------------------------------------------
# Parameters shared with tests/test_gpu_bond_device.py (chosen here, on the exact
# curves alone).  A trajectory's value has a spread of order 1 (a read-out
# expectation, times Kraus weights close to 1), so at N = 8192 the standard error
# of a mean is about 1 / sqrt(N) = 0.011, at most 0.02 with the weights' spread.
# The GPU test asks the exact curves with and without the bond channel to differ
# by more than twice its largest standard error: 0.08 here leaves that a factor 2.
EXACT = dict(L=4, T=5, p_bond=0.25, p=0.05, seed=0xB0D, g=0.9)


def exact_spec(pkg, noise, energy=False):
    L, T = EXACT["L"], EXACT["T"]
    rng = np.random.default_rng(31)
    hs, phis = random_disorder(rng, L)
    extra = dict(device=harsh_device(pkg, L)) if noise == "device" else dict(
        noise_prob=EXACT["p"])
    kw = dict(init_mask_value=0b0100) if energy else dict(initial_state="neel")
    return pkg.SweepSpec(L=L, T=T, hs=hs, phis=phis, g=EXACT["g"], bond_noise=EXACT["p_bond"],
                         **extra, **kw)


@pytest.mark.parametrize("noise", ["depol", "device"])
def test_exact_channel_is_resolved_and_matches_literal_mean(pkg, noise):
    spec = exact_spec(pkg, noise)
    L, T, pb = spec.L, spec.T, EXACT["p_bond"]
    args = (L, T, spec.hs[0], spec.phis[0], spec.kick)
    kw = dict(p=spec.p, device=spec.device, init_mask=spec.init_mask)
    f1, e1 = bdm.exact_autocorr(*args, pb, probe=spec.probe_site, **kw)
    f0, e0 = bdm.exact_autocorr(*args, 0.0, probe=spec.probe_site, **kw)
    # without bond noise the exact model is the project's density-matrix oracle
    from oracle import dm_oracle

    if noise == "device":
        rf, re_ = dm_oracle.device_folded_sweep(L, T, spec.hs[0], spec.phis[0], spec.kick,
                                                spec.device, initial_state="neel")
    else:
        rf, re_ = dm_oracle.folded_sweep(L, T, spec.hs[0], spec.phis[0], spec.kick, spec.p,
                                         initial_state="neel")
    assert max(np.abs(f0 - rf).max(), np.abs(e0 - re_).max()) < 1e-12
    assert max(np.abs(f1 - f0).max(), np.abs(e1 - e0).max()) > 0.08
    espec = exact_spec(pkg, noise, energy=True)
    ekw = dict(p=espec.p, device=espec.device, init_mask=espec.init_mask)
    ex1 = bdm.exact_energy(*args, pb, **ekw)
    ex0 = bdm.exact_energy(*args, 0.0, **ekw)
    assert max(np.abs(a - b).max() for a, b in zip(ex1, ex0)) > 0.08
    # the literal model's trajectory mean at small N
    N = 300
    rows_f, rows_e, rows_z = [], [], []
    for r in range(N):
        d = _draws(pkg, spec, EXACT["seed"], r, p_bond=pb)
        f, e, _ = _autocorr_row(pkg, spec, 0, d)
        rows_f.append(f)
        rows_e.append(e)
        ed = _draws(pkg, espec, EXACT["seed"], r, p_bond=pb)
        rows_z.append(np.concatenate(bdm.literal_energy(L, T, espec.hs[0], espec.phis[0],
                                                        espec.kick, espec.init_mask, ed),
                                     axis=1))
    for rows, exact in ((np.array(rows_f), f1), (np.array(rows_e), e1),
                        (np.array(rows_z), np.concatenate(ex1, axis=1))):
        se = rows.std(axis=0, ddof=1) / np.sqrt(N) + 1e-12
        zscore = (rows.mean(axis=0) - exact) / se
        assert np.abs(zscore).max() < 4.5, zscore


# ---- 7. refusals and plumbing --------------------------------------------------------
def test_refusals_and_plumbing(pkg):
    spec = _spec(pkg, 5, 3, "x", "depol", bond_noise=0.1)
    eng = pkg.DtcEngine.__new__(pkg.DtcEngine)
    for call, word in ((lambda: eng.energy(spec, 2), "energy_bond"),
                       (lambda: eng.energy_sums(spec, 2), "energy_sums_bond")):
        with pytest.raises(NotImplementedError, match=word):
            call()
    for call in (lambda: eng.prefix_build(spec, 2, 1), lambda: eng.autocorr_prefixed(spec, 2),
                 lambda: pkg.sharded.sharded_forward(None, spec, 1)):
        with pytest.raises(NotImplementedError):
            call()
    eng._ctx = None
    assert hasattr(pkg.DtcEngine, "energy_bond") and hasattr(pkg.DtcEngine, "energy_sums_bond")
    # parsers and file names
    for mod in (pkg.cli, pkg.energy_cli):
        ns = mod.build_parser().parse_args([])
        assert ns.fakebackend_bond == 0 and ns.bond_noise_prob == 0.0
        ns = mod.build_parser().parse_args(["--fakebackend_bond", "1"])
        assert ns.fakebackend_bond == 1
        with pytest.raises(SystemExit):
            mod.build_parser().parse_args(["--fakebackend_bond", "2"])
    assert pkg.energy_cli.build_parser().parse_args(
        ["--bond_noise_prob", "0.02"]).bond_noise_prob == 0.02
    eargs = ("energy_data", "vacuum", 0.97, 4, 1, 1, 0.0, 1.0, 0.05, 1)
    plain = ("energy_data_vacuum_g0.97_L4_inst1_randomphi1_delta0.0_amplitude1.0_noise0.05"
             "_usenoise1.csv")
    assert pkg.energy.energy_csv_name(*eargs) == plain
    assert pkg.energy.energy_csv_name(*eargs, bond_noise_prob=0.0) == plain
    assert pkg.energy.energy_csv_name(*eargs, bond_noise_prob=0.01) == plain[:-4] + "_bond0.01.csv"
    assert pkg.energy.energy_csv_name(*eargs, bond_noise_prob="cal") == plain[:-4] + "_bondcal.csv"
    cal = pkg.DeviceCalibration(name="t", qubits=[], sx_gate_ns=35.0, cz_error=7e-3)
    ns = pkg.cli.build_parser().parse_args([])
    assert pkg.cli.bond_from_args(ns, None, 5) == (None, 0.0)
    assert pkg.cli.bond_from_args(ns, cal, 5) == (None, 0.0)
    ns = pkg.cli.build_parser().parse_args(["--bond_noise_prob", "0.02"])
    assert pkg.cli.bond_from_args(ns, cal, 5) == (0.02, 0.02)
    ns = pkg.cli.build_parser().parse_args(["--fakebackend_bond", "1"])
    b, tag = pkg.cli.bond_from_args(ns, cal, 5)
    assert tag == "cal" and np.array_equal(b, cal.bond_noise(5))
    with pytest.raises(SystemExit):
        pkg.cli.bond_from_args(ns, None, 5)
    # the facade keeps a two-qubit error next to a calibration
    nm = pkg.NoiseModel()
    nm.add_all_qubit_quantum_error(pkg.depolarizing_error(0.03, 2), ["rzz"])
    assert nm.bond_error.p == 0.03
