"""Numpy references for bond noise together with noisy kicks (include/dtc.h
dtc_autocorr_bond with dv, dtc_energy_bond): TEST INFRASTRUCTURE ONLY.

* ``literal_autocorr`` / ``literal_energy``: one trajectory gate by gate.  The
  kick sub-gates are noisy -- depolarizing (a drawn Pauli after the gate) or
  device-like (the gate G, then the weighted amplitude-damping operator
  K1 = b |0><1| on a jump or K0 = diag(a0, a1) otherwise, then the drawn Pauli)
  -- with the draws of ``dtc_kick_draws``; the bonds take the Pauli pairs of
  ``dtc_bond_draws`` right after each RZZ / RZZ^+ (tests/bond_model.py).
  Inverse periods take their sub-gates reversed and daggered, the neel
  preparation the Pauli part only.
* ``sign_rules``: the energy path's observable signs under an outgoing Pauli.
* ``exact_autocorr`` / ``exact_energy``: the exact density-matrix evolution
  with the channels themselves, L <= 4.
"""
import numpy as np

from tests import bond_model as bm

STREAM_PREP = 0xFFFFFFFF


def has_z(code: int) -> int:
    return 1 if code in (2, 3) else 0


def kraus_weights(device):
    """Per site (a0, a1, b): K0 = diag(a0, a1) drawn w.p. q0 = 1 - q1 and
    K1 = b |0><1| w.p. q1 = gamma / 2, both weighted by 1 / sqrt(q)."""
    out = []
    for gamma, _, _ in device.site_channels():
        q1 = gamma / 2.0
        out.append((1.0 / np.sqrt(1.0 - q1), np.sqrt(1.0 - gamma) / np.sqrt(1.0 - q1),
                    np.sqrt(gamma / q1) if q1 > 0 else 0.0))
    return out


class Draws:
    """The draws of one trajectory: ``kick(stream, counter)`` -> (pauli, jump)
    [L][n_sub], ``bond(stream, counter)`` -> codes [L-1]."""

    def __init__(self, pkg, L, n_sub, seed, traj, p=0.0, device=None, p_bond=None):
        self.pkg, self.L, self.n_sub, self.seed, self.traj = pkg, L, n_sub, seed, traj
        self.p, self.device, self.p_bond = p, device, p_bond

    def kick(self, stream, counter):
        return self.pkg.engine.kick_draws(self.L, self.n_sub, self.seed, self.traj, stream,
                                          counter, p=self.p, device=self.device)

    def bond(self, stream, counter):
        if self.p_bond is None:
            return np.zeros(max(self.L - 1, 0), dtype=np.int32)
        return self.pkg.engine.bond_draws(self.p_bond, self.L, self.seed, self.traj, stream,
                                          counter)

    def prep_mask(self, init_mask):
        """Neel X gates followed by their Pauli draw: X or Y undo the flip."""
        if self.device is None and self.p == 0.0:
            return init_mask
        pauli, _ = self.kick(STREAM_PREP, 0)
        m = init_mask
        for i in range(self.L):
            if (init_mask >> i) & 1 and pauli[i, 0] in (1, 2):
                m &= ~(1 << i)
        return m


def kick_layer(psi, L, gates, pauli, jump, kraus, inverse):
    """One noisy kick layer: per site the sub-gates (reversed and daggered for
    an inverse period), each followed by its Kraus operator (device) and Pauli."""
    for i in range(L):
        n = len(gates[i])
        for q in range(n):
            M = gates[i][n - 1 - q].conj().T if inverse else gates[i][q]
            if kraus is not None:
                a0, a1, b = kraus[i]
                K = (np.array([[0, b], [0, 0]], dtype=np.complex128) if jump[i, q]
                     else np.diag([a0, a1]).astype(np.complex128))
                M = K @ M
            # (one pass over the state per sub-gate: its three factors as one 2x2)
            psi = bm.apply_1q(psi, L, i, bm.PAULI[int(pauli[i, q])] @ M)
    return psi


def weighted_z(psi, L):
    """<psi| Z_i |psi> without normalising (the Kraus-weighted expectation)."""
    return bm.z_expectations(psi, L)


def observables(psi, L):
    """Unnormalised <Z_i>, <Z_i Z_i+1>, <X_i>."""
    z = bm.z_expectations(psi, L)
    pr = np.abs(psi) ** 2
    zz = np.zeros(max(L - 1, 0))
    for i in range(L - 1):
        v = pr.reshape(-1, 2, 2, 1 << i)
        zz[i] = v[:, 0, 0, :].sum() + v[:, 1, 1, :].sum() - v[:, 0, 1, :].sum() - v[:, 1, 0, :].sum()
    xs = np.zeros(L)
    for i in range(L):
        v = psi.reshape(-1, 2, 1 << i)
        xs[i] = 2.0 * float(np.real(np.vdot(v[:, 0, :], v[:, 1, :])))
    return z, zz, xs


def _forward_period(psi, L, hs, phis, kick_row, draws, kraus, q):
    pauli, jump = draws.kick(0, q)
    psi = kick_layer(psi, L, bm.kick_gates(kick_row), pauli, jump, kraus, False)
    return bm.literal_layer(psi, L, hs, phis, draws.bond(0, q), False)


def literal_autocorr(L, T, hs, phis, kick, init_mask, probe, draws, fac=1.0, ro=(1.0, 0.0)):
    """One trajectory of the folded autocorrelator circuit: fwd [T], echo [T]
    (= ro_a * fac * z_j(prep) <Z_j> + ro_b) and zsite [T][L] (unnormalised)."""
    kraus = kraus_weights(draws.device) if draws.device is not None else None
    m = draws.prep_mask(init_mask)
    psi = np.zeros(1 << L, dtype=np.complex128)
    psi[m] = 1.0
    zinit = -1.0 if (m >> probe) & 1 else 1.0
    fwd, echo, zs = np.zeros(T), np.zeros(T), np.zeros((T, L))
    for t in range(T):
        if t > 0:
            psi = _forward_period(psi, L, hs, phis, kick[t - 1], draws, kraus, t)
        zs[t] = weighted_z(psi, L)
        fwd[t] = ro[0] * fac * zinit * zs[t, probe] + ro[1]
        e = psi.copy()
        for k in range(1, t + 1):
            e = bm.literal_layer(e, L, hs, phis, draws.bond(1 + t, k), True)
            pauli, jump = draws.kick(1 + t, k)
            e = kick_layer(e, L, bm.kick_gates(kick[t - k]), pauli, jump, kraus, True)
        echo[t] = ro[0] * fac * zinit * weighted_z(e, L)[probe] + ro[1]
    return fwd, echo, zs


def literal_energy(L, T, hs, phis, kick, init_mask, draws, t_offset=0):
    """One trajectory of the energy circuit (forward periods only):
    z [T][L], zz [T][L-1], x [T][L], unnormalised."""
    kraus = kraus_weights(draws.device) if draws.device is not None else None
    psi = np.zeros(1 << L, dtype=np.complex128)
    psi[draws.prep_mask(init_mask)] = 1.0
    z, zz, xs = np.zeros((T, L)), np.zeros((T, max(L - 1, 0))), np.zeros((T, L))
    for s in range(T + t_offset):
        if s > 0:
            psi = _forward_period(psi, L, hs, phis, kick[s - 1], draws, kraus, s)
        if s - t_offset >= 0:
            z[s - t_offset], zz[s - t_offset], xs[s - t_offset] = observables(psi, L)
    return z, zz, xs


# ---- the sign rules of the energy path ----------------------------------------
def outgoing_z(L, codes):
    """Z content (Y or Z) per site of the layer's outgoing Pauli."""
    out = np.zeros(L, dtype=int)
    for b in range(L - 1):
        out[b] ^= has_z(codes[b] & 3)
        out[b + 1] ^= has_z(codes[b] >> 2)
    return out


def sign_rules(L, codes, z, zz, xs):
    """Observables after the outgoing Pauli P of ``codes`` from those before
    it: <Z_i> flips where P has X content on i, <Z_i Z_i+1> by the product of
    the two sites' flips, <X_i> where P has Z content on i."""
    sx = 1 - 2 * bm.outgoing_x(L, codes)
    sz = 1 - 2 * outgoing_z(L, codes)
    return sx * z, sx[:-1] * sx[1:] * zz, sz * xs


def apply_outgoing(psi, L, codes):
    """P applied literally: the pair of every bond, site by site."""
    for b in range(L - 1):
        psi = bm.apply_pauli(psi, L, b, codes[b] & 3)
        psi = bm.apply_pauli(psi, L, b + 1, codes[b] >> 2)
    return psi


# ---- exact channels (density matrix, L <= 4) ------------------------------------
def _site_channel(rho, L, i, chan):
    """``chan``: depolarizing p (float) or the device's (gamma, d, p) of the site."""
    if not isinstance(chan, tuple):
        return bm._depol1(rho, L, i, chan)
    gamma, d, p = chan
    K0 = bm._embed(L, {i: np.diag([1.0, np.sqrt(1.0 - gamma)]).astype(np.complex128)})
    K1 = bm._embed(L, {i: np.array([[0, np.sqrt(gamma)], [0, 0]], dtype=np.complex128)})
    rho = bm._conj(rho, K0) + bm._conj(rho, K1)
    rho = (1.0 - d) * rho + d * bm._conj(rho, bm._embed(L, {i: bm.PAULI[3]}))
    return bm._depol1(rho, L, i, p)


def _dm_period(rho, L, gates, hs, phis, chans, p_bond, inverse):
    z = bm.zbits(L)
    sgn = -1.0 if inverse else 1.0

    def diag(rho, ang):
        ph = np.exp(-0.5j * sgn * ang)
        return ph[:, None] * rho * ph.conj()[None, :]

    def kicks(rho):
        for i in range(L):
            for G in (reversed(gates[i]) if inverse else gates[i]):
                rho = bm._conj(rho, bm._embed(L, {i: G.conj().T if inverse else G}))
                rho = _site_channel(rho, L, i, chans[i])
        return rho

    if not inverse:
        rho = kicks(rho)
    else:
        for i in range(L):
            rho = diag(rho, hs[i] * z[i])
    for b in bm.bond_order(L, inverse):
        rho = diag(rho, phis[b] * z[b] * z[b + 1])
        rho = bm._depol2(rho, L, b, p_bond[b])
    if not inverse:
        for i in range(L):
            rho = diag(rho, hs[i] * z[i])
    else:
        rho = kicks(rho)
    return rho


def _channels(L, p, device):
    return [tuple(c) for c in device.site_channels()] if device is not None else [float(p)] * L


def _prep_weights(L, init_mask, chans):
    x = np.arange(1 << L)
    w = np.ones(1 << L)
    for i in range(L):
        p = chans[i][2] if isinstance(chans[i], tuple) else chans[i]
        pf = (1 - p / 2) if (init_mask >> i) & 1 else 0.0  # X or Y after the X undo the flip
        w = w * np.where((x >> i) & 1, pf, 1 - pf)
    return w


def exact_autocorr(L, T, hs, phis, kick, p_bond, p=0.0, device=None, init_mask=0, probe=None,
                   n_anc=6):
    """Exact A_fwd(t), A_echo(t) with noisy kicks (depolarizing ``p`` with the
    (1-p)^n_anc ancilla factor, or ``device`` with its anc_factor and read-out
    map) and depolarizing_error(p_bond[b], 2) after every RZZ / RZZ^+."""
    assert L <= 4
    j = int(L / 2) if probe is None else probe
    p_bond = np.broadcast_to(np.asarray(p_bond, dtype=float), (L - 1,))
    chans = _channels(L, p, device)
    zj = bm.zbits(L)[j]
    sigma = np.diag(_prep_weights(L, init_mask, chans) * zj).astype(np.complex128)

    def out(v):
        return device.readout(device.anc_factor * v) if device is not None \
            else (1 - p) ** n_anc * v

    fwd, echo = np.zeros(T), np.zeros(T)
    for t in range(T):
        if t > 0:
            sigma = _dm_period(sigma, L, bm.kick_gates(kick[t - 1]), hs, phis, chans, p_bond,
                               False)
        fwd[t] = out(float(np.real(zj @ np.diag(sigma))))
        e = sigma
        for k in range(t, 0, -1):
            e = _dm_period(e, L, bm.kick_gates(kick[k - 1]), hs, phis, chans, p_bond, True)
        echo[t] = out(float(np.real(zj @ np.diag(e))))
    return fwd, echo


def exact_energy(L, T, hs, phis, kick, p_bond, p=0.0, device=None, init_mask=0):
    """Exact <Z_i>, <Z_i Z_i+1>, <X_i> of the energy circuit, t = 0..T-1."""
    assert L <= 4
    p_bond = np.broadcast_to(np.asarray(p_bond, dtype=float), (L - 1,))
    chans = _channels(L, p, device)
    rho = np.diag(_prep_weights(L, init_mask, chans)).astype(np.complex128)
    zb = bm.zbits(L)
    x = np.arange(1 << L)
    z, zz, xs = np.zeros((T, L)), np.zeros((T, L - 1)), np.zeros((T, L))
    for t in range(T):
        if t > 0:
            rho = _dm_period(rho, L, bm.kick_gates(kick[t - 1]), hs, phis, chans, p_bond, False)
        d = np.real(np.diag(rho))
        z[t] = zb @ d
        for i in range(L - 1):
            zz[t, i] = (zb[i] * zb[i + 1]) @ d
        for i in range(L):
            lo = x[((x >> i) & 1) == 0]
            xs[t, i] = 2.0 * float(np.real(rho[lo ^ (1 << i), lo]).sum())
    return z, zz, xs
