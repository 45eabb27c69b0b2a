"""Numpy references for the bond noise (include/dtc.h dtc_bond_noise): Aer's
``depolarizing_error(p, 2)`` after every RZZ of a forward period and every
RZZ^+ of an inverse period (autocorr-delta-a-single-qiskit-fast.py:111-121,
140-143).  TEST INFRASTRUCTURE ONLY.

* ``literal_layer`` / ``literal_trajectory``: a statevector model that applies
  every gate of the reference's period one by one and inserts the drawn Pauli
  pair right after each RZZ / RZZ^+.  The draws come from ``dtc_bond_draws``
  (``codes[b] = P_site_b + 4 * P_site_b+1``, 0 I, 1 X, 2 Y, 3 Z).
* ``rule_layer``: the engine's form of the same layer -- the diagonal with the
  angle signs of DESIGN.md's flip rules, then the merged outgoing Paulis.
* ``exact_sweep``: the exact density-matrix evolution of the folded circuit
  with the channel itself (and the single-qubit depolarizing noise of the
  kicks, the neel preparation and the ancilla), for L <= 4.
"""
import numpy as np

PAULI = [np.eye(2, dtype=np.complex128),
         np.array([[0, 1], [1, 0]], dtype=np.complex128),
         np.array([[0, -1j], [1j, 0]], dtype=np.complex128),
         np.array([[1, 0], [0, -1]], dtype=np.complex128)]


def has_x(code: int) -> int:
    return 1 if code in (1, 2) else 0


def zbits(L):
    x = np.arange(1 << L)
    return 1 - 2 * ((x[None, :] >> np.arange(L)[:, None]) & 1)


def apply_1q(psi, L, i, U):
    """U on site i (bit i of the index)."""
    v = psi.reshape(-1, 2, 1 << i)
    out = np.empty_like(v)
    out[:, 0, :] = U[0, 0] * v[:, 0, :] + U[0, 1] * v[:, 1, :]
    out[:, 1, :] = U[1, 0] * v[:, 0, :] + U[1, 1] * v[:, 1, :]
    return out.reshape(-1)


def apply_pauli(psi, L, i, code):
    return psi if code == 0 else apply_1q(psi, L, i, PAULI[code])


def apply_rz(psi, L, i, theta):
    """exp(-i theta Z_i / 2), in place."""
    v = psi.reshape(-1, 2, 1 << i)
    v[:, 0, :] *= np.exp(-0.5j * theta)
    v[:, 1, :] *= np.exp(0.5j * theta)
    return psi


def apply_rzz(psi, L, b, theta):
    """exp(-i theta Z_b Z_b+1 / 2), in place."""
    v = psi.reshape(-1, 2, 2, 1 << b)
    for hi in (0, 1):
        for lo in (0, 1):
            v[:, hi, lo, :] *= np.exp((-0.5j if hi == lo else 0.5j) * theta)
    return psi


def z_expectations(psi, L):
    pr = np.abs(psi) ** 2
    out = np.zeros(L)
    for i in range(L):
        v = pr.reshape(-1, 2, 1 << i)
        out[i] = v[:, 0, :].sum() - v[:, 1, :].sum()
    return out


def kick_gates(kick_row):
    """[L][n_sub][8] ABI row -> per-site list of 2x2 matrices."""
    out = []
    for i in range(kick_row.shape[0]):
        r = kick_row[i].reshape(kick_row.shape[1], 4, 2)
        out.append([(g[:, 0] + 1j * g[:, 1]).reshape(2, 2) for g in r])
    return out


def bond_order(L, inverse):
    even, odd = list(range(0, L - 1, 2)), list(range(1, L - 1, 2))
    return odd + even if inverse else even + odd


def literal_layer(psi, L, hs, phis, codes, inverse):
    """The diagonal part of one period gate by gate, the Pauli pair of bond b
    right after its RZZ (forward: RZZ even, RZZ odd, RZ) or RZZ^+ (inverse:
    RZ^+, RZZ^+ odd, RZZ^+ even)."""
    sgn = -1.0 if inverse else 1.0
    psi = psi.copy()
    if inverse:
        for i in range(L):
            psi = apply_rz(psi, L, i, sgn * hs[i])
    for b in bond_order(L, inverse):
        psi = apply_rzz(psi, L, b, sgn * phis[b])
        psi = apply_pauli(psi, L, b, codes[b] & 3)
        psi = apply_pauli(psi, L, b + 1, codes[b] >> 2)
    if not inverse:
        for i in range(L):
            psi = apply_rz(psi, L, i, sgn * hs[i])
    return psi


def flip_signs(L, codes, inverse):
    """(field signs [L], bond signs [L-1]) of the layer after its errors are
    pushed to the end: forward, odd bond b gets (-1)^(xR_{b-1} + xL_{b+1}) and
    field i (-1)^(xR_{i-1} + xL_i); inverse, even bond b gets
    (-1)^(xR_{b-1} + xL_{b+1})."""
    def xl(b):
        return has_x(codes[b] & 3) if 0 <= b < L - 1 else 0

    def xr(b):
        return has_x(codes[b] >> 2) if 0 <= b < L - 1 else 0

    sh = np.ones(L)
    sb = np.ones(max(L - 1, 0))
    for b in range(L - 1):
        late = (b % 2 == 0) if inverse else (b % 2 == 1)
        if late and (xr(b - 1) + xl(b + 1)) % 2:
            sb[b] = -1.0
    if not inverse:
        for i in range(L):
            if (xr(i - 1) + xl(i)) % 2:
                sh[i] = -1.0
    return sh, sb


def outgoing_x(L, codes):
    """X content per site of the layer's outgoing Pauli."""
    out = np.zeros(L, dtype=int)
    for b in range(L - 1):
        out[b] ^= has_x(codes[b] & 3)
        out[b + 1] ^= has_x(codes[b] >> 2)
    return out


def rule_layer(psi, L, hs, phis, codes, inverse):
    """The same layer as signed angles plus merged Paulis (equal to
    ``literal_layer`` up to a global phase)."""
    z = zbits(L)
    sh, sb = flip_signs(L, codes, inverse)
    ang = np.zeros(1 << L)
    for i in range(L):
        ang += sh[i] * hs[i] * z[i]
    for b in range(L - 1):
        ang += sb[b] * phis[b] * z[b] * z[b + 1]
    psi = psi * np.exp((0.5j if inverse else -0.5j) * ang)
    for i in range(L):
        P = np.eye(2, dtype=np.complex128)
        if i > 0:
            P = PAULI[codes[i - 1] >> 2] @ P
        if i < L - 1:
            P = P @ PAULI[codes[i] & 3]
        psi = apply_1q(psi, L, i, P)
    return psi


def literal_trajectory(L, T, hs, phis, kick, init_mask, probe, draw, layer=literal_layer):
    """One trajectory without kick noise: ``draw(stream, counter)`` gives the
    layer's codes (forward layer p: (0, p); step k of the echo at t:
    (1 + t, k)).  Returns fwd [T], echo [T] (= z_j(init) <Z_j>) and
    zsite [T][L]."""
    psi = np.zeros(1 << L, dtype=np.complex128)
    psi[init_mask] = 1.0
    zinit = -1.0 if (init_mask >> probe) & 1 else 1.0
    fwd, echo, zs = np.zeros(T), np.zeros(T), np.zeros((T, L))
    for t in range(T):
        if t > 0:
            for i, gs in enumerate(kick_gates(kick[t - 1])):
                for G in gs:
                    psi = apply_1q(psi, L, i, G)
            psi = layer(psi, L, hs, phis, draw(0, t), False)
        zs[t] = z_expectations(psi, L)
        fwd[t] = zinit * zs[t, probe]
        e = psi.copy()
        for k in range(1, t + 1):
            e = layer(e, L, hs, phis, draw(1 + t, k), True)
            for i, gs in enumerate(kick_gates(kick[t - k])):
                for G in reversed(gs):
                    e = apply_1q(e, L, i, G.conj().T)
        echo[t] = zinit * z_expectations(e, L)[probe]
    return fwd, echo, zs


# ---- exact channel (density matrix, L <= 4) -----------------------------------
def _embed(L, ops):
    """Operator with ops[i] on site i (bit i of the index; missing = identity)."""
    m = np.eye(1, dtype=np.complex128)
    for i in reversed(range(L)):
        m = np.kron(m, ops.get(i, PAULI[0]))
    return m


def _conj(rho, U):
    return U @ rho @ U.conj().T


def _depol1(rho, L, i, p):
    if p == 0.0:
        return rho
    return (1 - p) * rho + (p / 4) * sum(_conj(rho, _embed(L, {i: P})) for P in PAULI)


def _depol2(rho, L, b, p):
    """(1 - p) rho + p Tr_{b,b+1}(rho) x I/4 = (1 - p) rho + p/16 sum_PQ PQ rho PQ."""
    if p == 0.0:
        return rho
    acc = sum(_conj(rho, _embed(L, {b: P, b + 1: Q})) for P in PAULI for Q in PAULI)
    return (1 - p) * rho + (p / 16) * acc


def _dm_period(rho, L, gates, hs, phis, p, p_bond, inverse):
    z = zbits(L)
    sgn = -1.0 if inverse else 1.0

    def diag(ang):
        ph = np.exp(-0.5j * sgn * ang)
        return ph[:, None] * rho * ph.conj()[None, :]

    def kicks(rho):
        for i in (reversed(range(L)) if inverse else range(L)):
            for G in (reversed(gates[i]) if inverse else gates[i]):
                rho = _conj(rho, _embed(L, {i: G.conj().T if inverse else G}))
                rho = _depol1(rho, L, i, p)
        return rho

    if not inverse:
        rho = kicks(rho)
    else:
        for i in range(L):
            rho = diag(hs[i] * z[i])
    for b in bond_order(L, inverse):
        rho = diag(phis[b] * z[b] * z[b + 1])
        rho = _depol2(rho, L, b, p_bond[b])
    if not inverse:
        for i in range(L):
            rho = diag(hs[i] * z[i])
    else:
        rho = kicks(rho)
    return rho


def exact_sweep(L, T, hs, phis, kick, p_bond, p=0.0, init_mask=0, probe=None, n_anc=6):
    """Exact A_fwd(t), A_echo(t), t = 0..T-1, of the folded circuit
    (A = (1-p)^n_anc Tr[Z_j E_t(rho0 Z_j)]) with depolarizing_error(p, 1) after
    every kick sub-gate and preparation X, and depolarizing_error(p_bond[b], 2)
    after every RZZ / RZZ^+ of bond b."""
    assert L <= 4
    j = int(L / 2) if probe is None else probe
    p_bond = np.broadcast_to(np.asarray(p_bond, dtype=float), (L - 1,))
    x = np.arange(1 << L)
    w = np.ones(1 << L)
    for i in range(L):
        pf = (1 - p / 2) if (init_mask >> i) & 1 else 0.0  # X or Y after the X undo the flip
        w = w * np.where((x >> i) & 1, pf, 1 - pf)
    sigma = np.diag(w * zbits(L)[j]).astype(np.complex128)
    fac = (1 - p) ** n_anc
    zj = zbits(L)[j]
    fwd, echo = np.zeros(T), np.zeros(T)
    for t in range(T):
        if t > 0:
            sigma = _dm_period(sigma, L, kick_gates(kick[t - 1]), hs, phis, p, p_bond, False)
        fwd[t] = fac * float(np.real(zj @ np.diag(sigma)))
        e = sigma
        for k in range(t, 0, -1):
            e = _dm_period(e, L, kick_gates(kick[k - 1]), hs, phis, p, p_bond, True)
        echo[t] = fac * float(np.real(zj @ np.diag(e)))
    return fwd, echo
