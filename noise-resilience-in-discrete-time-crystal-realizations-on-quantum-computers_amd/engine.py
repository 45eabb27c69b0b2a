"""Host-side handle on the HIP engine (one ``dtc_ctx`` per device).

This is the layer the reference's drivers reach through
``AerSimulator(...).run(circ, shots).result().get_counts()`` (fast.py:156,
211-212); here the whole t-sweep of a disorder instance is one call, see
``include/dtc.h``.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass, field

import numpy as np

from . import _capi
from .kicks import kick_table, n_sub_of

N_ANCILLA_NOISY_GATES = 6  # H, CZ=u2.cx.u2 (x2), H on the ancilla -> six noisy u2


@dataclass
class SweepSpec:
    """Everything that defines one autocorrelator sweep (fast.py argparse +
    disorder).  ``hs``: [n_inst][L], ``phis``: [n_inst][L-1]."""

    L: int
    T: int
    hs: np.ndarray
    phis: np.ndarray
    g: float | list = 0.97
    polarization: str = "x"
    circular_frequency: float = 1.0
    initial_state: str = "vacuum"
    noise_prob: float = 0.05
    use_noise: int = 1
    t_offset: int = 0
    probe_site: int | None = None
    kick: np.ndarray | None = field(default=None, repr=False)
    init_mask_value: int | None = None   # explicit Z-basis prep (overrides initial_state)
    device: object | None = field(default=None, repr=False)  # DeviceNoise (use_fakebackend=1)
    # depolarizing_error(p, 2) after every RZZ / RZZ^+ (include/dtc.h dtc_bond_noise):
    # a float for every bond, an [L-1] array, or None
    bond_noise: float | np.ndarray | None = None

    def __post_init__(self):
        if self.bond_noise is not None:
            b = np.asarray(self.bond_noise, dtype=np.float64)
            n = max(self.L - 1, 0)
            if b.ndim == 0:
                b = np.full(n, float(b))
            if b.shape != (n,):
                raise ValueError(f"bond_noise must be a float or an [L-1] = [{n}] array")
            if np.any(~(b >= 0.0)) or np.any(b > 16.0 / 15.0):
                raise ValueError("bond_noise must lie in [0, 16/15]")
            self.bond_noise = np.ascontiguousarray(b)
        self.hs = np.ascontiguousarray(np.atleast_2d(self.hs)[:, : self.L], dtype=np.float64)
        ph = np.atleast_2d(self.phis)
        self.phis = np.ascontiguousarray(ph[:, : max(self.L - 1, 0)], dtype=np.float64)
        if self.L == 1:
            self.phis = np.zeros((self.hs.shape[0], 1))
        if self.probe_site is None:
            self.probe_site = int(self.L / 2)  # fast.py:221
        if self.kick is None:
            self.kick = kick_table(self.L, self.n_periods, self.g, self.polarization,
                                   self.circular_frequency)
        self.kick = np.ascontiguousarray(self.kick, dtype=np.float64)

    @property
    def n_inst(self) -> int:
        return self.hs.shape[0]

    @property
    def n_periods(self) -> int:
        return max(1, self.T - 1 + self.t_offset)

    @property
    def n_sub(self) -> int:
        return self.kick.shape[2]

    @property
    def p(self) -> float:
        return float(self.noise_prob) if self.use_noise else 0.0

    @property
    def has_bond_noise(self) -> bool:
        return self.bond_noise is not None and bool(np.any(self.bond_noise > 0.0))

    @property
    def init_mask(self) -> int:
        if self.init_mask_value is not None:
            return int(self.init_mask_value)
        return init_mask(self.L, self.initial_state)


def init_mask(L: int, initial_state: str) -> int:
    """fast.py:127-130: ``neel`` = X on circuit qubits 2, 4, ... (sites 1, 3, ...)."""
    if initial_state == "vacuum":
        return 0
    if initial_state == "neel":
        m = 0
        for q in range(1, L + 1):
            if q % 2 == 0:
                m |= 1 << (q - 1)
        return m
    raise ValueError(f"initial_state must be 'vacuum' or 'neel', got {initial_state!r}")


def energy_init_mask(L: int, initial_state: str) -> int:
    """The energy scripts' preparation (autocorr-delta-a-single-qiskit-fast-energy.py:137-141,
    the same loop in every ``-energy*.py``): ``for i in range(1, L+1): if i % 2 == 0:
    circ.x(i)`` on ``QuantumCircuit(L)`` -- L qubits, no ancilla, so qubit i IS site i.
    For odd L that flips sites 2, 4, ..., L-1; for even L the loop reaches
    ``circ.x(L)`` on an L-qubit circuit and qiskit raises (index out of range), so
    this raises too.  (The autocorrelator's ``init_mask`` differs: there qubit 0
    is the ancilla and circuit qubit i is site i-1.)"""
    if initial_state == "vacuum":
        return 0
    if initial_state != "neel":
        raise ValueError(f"initial_state must be 'vacuum' or 'neel', got {initial_state!r}")
    m = 0
    for i in range(1, L + 1):
        if i % 2 == 0:
            if i >= L:
                raise ValueError(
                    f"neel preparation of the {L}-qubit energy circuit applies X to qubit {i}, "
                    f"out of range(0, {L}) (the reference's circ.x({i}) raises for even L)")
            m |= 1 << i
    return m


def refuse_bond_noise(spec: SweepSpec, what: str, instead: str | None = None) -> None:
    """Bond noise exists on the autocorrelator sweep and the ``*_bond`` energy
    methods only."""
    if getattr(spec, "has_bond_noise", False):
        raise NotImplementedError(
            f"{what} does not support bond noise (SweepSpec.bond_noise); "
            + (f"use {instead}" if instead else
               "only DtcEngine.autocorr, energy_bond and energy_sums_bond do"))


def refuse_energy_echo(spec: SweepSpec, what: str) -> None:
    """The energy echo runs depolarizing or noiseless kicks only."""
    if getattr(spec, "device", None) is not None:
        raise NotImplementedError(
            f"{what} does not support device-like noise (SweepSpec.device): nothing may be "
            "measured across a Kraus kick, so the echo chains' ends would need stored states "
            "and X-basis passes, which are not built")
    if getattr(spec, "has_bond_noise", False):
        raise NotImplementedError(
            f"{what} does not support bond noise (SweepSpec.bond_noise): its per-state "
            "diagonal tables and plain chains are not built for the energy echo")


def refuse_sample(spec: SweepSpec, what: str) -> None:
    """Measurement sampling runs depolarizing or noiseless kicks only."""
    if getattr(spec, "device", None) is not None:
        raise NotImplementedError(
            f"{what} does not support device-like noise (SweepSpec.device): a shot of a "
            "Kraus-weighted trajectory would have to carry the trajectory's norm as a weight")
    if getattr(spec, "has_bond_noise", False):
        raise NotImplementedError(
            f"{what} does not support bond noise (SweepSpec.bond_noise): there is no sampled "
            "entry point taking its per-state diagonal tables")


def sample_draws(seed: int, traj: int, p: int, basis: int, n_shots: int) -> np.ndarray:
    """Host only (dtc_sample_draws): the uniforms in [0, 1) of the ``n_shots``
    measurement shots of trajectory ``traj`` after ``p`` periods in ``basis``
    (0 = Z, 1 = X)."""
    lib = _capi.load_library()
    u = np.zeros(int(n_shots))
    _capi.check(lib.dtc_sample_draws(
        ctypes.c_uint64(seed), ctypes.c_int64(traj), ctypes.c_int32(p), ctypes.c_int32(basis),
        ctypes.c_int32(n_shots), _capi.as_dptr(u)))
    return u


def sample_state(psi, L: int, basis: int, u) -> np.ndarray:
    """Host only (dtc_sample_state), the sampling contract's reference: the
    outcome of every uniform of ``u`` on the state ``psi`` (2^L amplitudes, site
    i = bit i): the smallest x whose running sum of ``|psi|^2`` in index order
    exceeds ``u W``; ``basis`` 1 applies a Hadamard to every site first."""
    lib = _capi.load_library()
    buf = np.ascontiguousarray(np.asarray(psi, dtype=np.complex128).reshape(-1))
    if buf.size != 1 << L:
        raise ValueError(f"psi must hold 2^L = {1 << L} amplitudes")
    uu = np.ascontiguousarray(np.atleast_1d(np.asarray(u, dtype=np.float64)))
    bits = np.zeros(uu.size, dtype=np.uint64)
    _capi.check(lib.dtc_sample_state(
        _capi.as_dptr(buf.view(np.float64)), ctypes.c_int32(L), ctypes.c_int32(basis),
        _capi.as_dptr(uu), ctypes.c_int32(uu.size),
        bits.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))))
    return bits


def refuse_correlations(spec: SweepSpec, what: str) -> None:
    """The all-pair correlators run depolarizing or noiseless kicks only."""
    if getattr(spec, "device", None) is not None:
        raise NotImplementedError(
            f"{what} does not support device-like noise (SweepSpec.device): the correlator "
            "sweep has no Kraus kick kinds (the sums stay linear there; not built)")
    if getattr(spec, "has_bond_noise", False):
        raise NotImplementedError(
            f"{what} does not support bond noise (SweepSpec.bond_noise): there is no correlator "
            "entry point taking its per-state diagonal tables")


def correlations_state(psi, L: int, basis: int):
    """Host only (dtc_correlations_state), the correlator contract's reference:
    ``(z [L], zz [L(L-1)/2])`` of the state ``psi`` (2^L amplitudes, site i = bit
    i), ``z_i = sum |psi|^2 z_i``, ``zz_(i,j) = sum |psi|^2 z_i z_j`` with the pairs
    in the order of ``correlations.pair_index``; ``basis`` 1 applies a Hadamard to
    every site first (X_i, X_i X_j)."""
    lib = _capi.load_library()
    buf = np.ascontiguousarray(np.asarray(psi, dtype=np.complex128).reshape(-1))
    if buf.size != 1 << L:
        raise ValueError(f"psi must hold 2^L = {1 << L} amplitudes")
    z = np.zeros(L)
    zz = np.zeros(L * (L - 1) // 2)
    _capi.check(lib.dtc_correlations_state(
        _capi.as_dptr(buf.view(np.float64)), ctypes.c_int32(L), ctypes.c_int32(basis),
        _capi.as_dptr(z), _capi.as_dptr(zz) if L > 1 else None))
    return z, zz


def refuse_rdm(spec: SweepSpec, what: str) -> None:
    """The reduced density matrices run depolarizing or noiseless kicks only."""
    if getattr(spec, "device", None) is not None:
        raise NotImplementedError(
            f"{what} does not support device-like noise (SweepSpec.device): the density-matrix "
            "sweep has no Kraus kick kinds (rho stays linear there; not built)")
    if getattr(spec, "has_bond_noise", False):
        raise NotImplementedError(
            f"{what} does not support bond noise (SweepSpec.bond_noise): there is no density-"
            "matrix entry point taking its per-state diagonal tables")


def window_array(windows) -> np.ndarray:
    """``windows`` (one window of sites, or a list of windows of one size) as a
    contiguous int32 [n_win][k] array.  Validity is the library's to check."""
    w = np.asarray(windows, dtype=np.int64)
    if w.ndim == 1:
        w = w[None, :]
    if w.ndim != 2 or w.shape[0] < 1 or w.shape[1] < 1:
        raise ValueError("windows must be [n_win][k] site lists of one size k")
    return np.ascontiguousarray(w.astype(np.int32))


def rdm_state(psi, L: int, sites) -> np.ndarray:
    """Host only (dtc_rdm_state), the density-matrix contract's reference: the
    complex128 [d][d] matrix ``rho[a][a'] = sum_c psi(a, c) conj psi(a', c)`` of
    the window ``sites`` (ascending, at most 4) of the state ``psi`` (2^L
    amplitudes, site i = bit i); bit m of ``a`` is the bit of ``sites[m]``."""
    lib = _capi.load_library()
    buf = np.ascontiguousarray(np.asarray(psi, dtype=np.complex128).reshape(-1))
    if buf.size != 1 << L:
        raise ValueError(f"psi must hold 2^L = {1 << L} amplitudes")
    s = np.ascontiguousarray(np.asarray(sites, dtype=np.int32).reshape(-1))
    k = int(s.size)
    d = 1 << k if 1 <= k <= 4 else 1  # (a bad k is the library's to refuse)
    rho = np.zeros((d, d), dtype=np.complex128)
    _capi.check(lib.dtc_rdm_state(
        _capi.as_dptr(buf.view(np.float64)), ctypes.c_int32(L),
        s.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), ctypes.c_int32(k),
        _capi.as_dptr(rho.view(np.float64))))
    return rho


def block_array(blocks) -> np.ndarray:
    """``blocks`` (one ``(start, k)`` pair, or a list of them of one size k) as
    an int32 [n_blk][2] array.  Validity is the library's to check."""
    b = np.asarray(blocks, dtype=np.int64)
    if b.ndim == 1:
        b = b[None, :]
    if b.ndim != 2 or b.shape[0] < 1 or b.shape[1] != 2:
        raise ValueError("blocks must be (start, k) pairs of one size k")
    if np.any(b[:, 1] != b[0, 1]):
        raise ValueError("all blocks of a call share one size k")
    return np.ascontiguousarray(b.astype(np.int32))


def rdm_block_state(psi, L: int, start: int, k: int):
    """Host only (dtc_rdm_block_state), the block contract's reference: the
    complex128 [d][d] matrix of the block of sites ``start .. start + k - 1``
    (5 <= k <= 10, 2 k <= L) of the state ``psi`` (2^L amplitudes, site i =
    bit i) and its purity ``sum |rho|^2``; bit m of a row index is the bit of
    site ``start + m``.  Returns ``(rho, purity)``."""
    lib = _capi.load_library()
    buf = np.ascontiguousarray(np.asarray(psi, dtype=np.complex128).reshape(-1))
    if not 1 <= L <= 32 or buf.size != 1 << L:
        raise ValueError("psi must hold 2^L amplitudes, 1 <= L <= 32")
    d = 1 << k if 5 <= k <= 10 else 1  # (a bad k is the library's to refuse)
    rho = np.zeros((d, d), dtype=np.complex128)
    pur = np.zeros(1)
    _capi.check(lib.dtc_rdm_block_state(
        _capi.as_dptr(buf.view(np.float64)), ctypes.c_int32(L), ctypes.c_int32(start),
        ctypes.c_int32(k), _capi.as_dptr(rho.view(np.float64)), _capi.as_dptr(pur)))
    return rho, float(pur[0])


def bond_struct(p_bond: np.ndarray) -> "_capi.DtcBondNoise":
    b = _capi.DtcBondNoise()
    b.p_bond = _capi.as_dptr(p_bond)
    return b


def bond_draws(p_bond, L: int, seed: int, traj: int, stream: int, counter: int) -> np.ndarray:
    """Host only (dtc_bond_draws): the Pauli pairs of one diagonal layer of one
    trajectory, ``codes[b] = P_site_b + 4 * P_site_b+1`` (0 I, 1 X, 2 Y, 3 Z).
    Forward layer p: (stream, counter) = (0, p); step k of the echo at t:
    (1 + t, k)."""
    lib = _capi.load_library()
    pb = np.asarray(p_bond, dtype=np.float64)
    if pb.ndim == 0:
        pb = np.full(max(L - 1, 0), float(pb))
    pb = np.ascontiguousarray(pb)
    if pb.shape != (max(L - 1, 0),):
        raise ValueError("p_bond must be a float or an [L-1] array")
    if pb.size == 0:
        return np.zeros(0, dtype=np.int32)
    codes = np.zeros(L - 1, dtype=np.int32)
    b = bond_struct(pb)
    _capi.check(lib.dtc_bond_draws(
        ctypes.byref(b), ctypes.c_int32(L), ctypes.c_uint64(seed), ctypes.c_int64(traj),
        ctypes.c_uint32(stream), ctypes.c_uint32(counter),
        codes.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))))
    return codes


def kick_draws(L: int, n_sub: int, seed: int, traj: int, stream: int, counter: int,
               p: float = 0.0, device=None):
    """Host only (dtc_kick_draws): the Pauli code after every kick sub-gate of
    one layer of one trajectory, ``pauli[site][sub]`` (0 I, 1 X, 2 Y, 3 Z), and
    the amplitude-damping jump flags ``jump[site][sub]`` (all 0 without
    ``device``).  Depolarizing noise of probability ``p``, or the device-like
    noise of ``device`` (a DeviceNoise).  Forward period q: (stream, counter) =
    (0, q); step k of the echo at t: (1 + t, k); the neel preparation:
    (0xFFFFFFFF, 0), sub-gate 0."""
    lib = _capi.load_library()
    pauli = np.zeros((L, n_sub), dtype=np.int32)
    jump = np.zeros((L, n_sub), dtype=np.int32)
    nz = _capi.DtcNoise()
    nz.p = float(p)
    nz.n_anc = N_ANCILLA_NOISY_GATES
    dv = None
    if device is not None:
        if device.L != L:
            raise ValueError("device noise has a different number of sites")
        dv = _capi.device_struct(device)
    ip = ctypes.POINTER(ctypes.c_int32)
    _capi.check(lib.dtc_kick_draws(
        ctypes.byref(nz), ctypes.byref(dv) if dv is not None else None, ctypes.c_int32(L),
        ctypes.c_int32(n_sub), ctypes.c_uint64(seed), ctypes.c_int64(traj),
        ctypes.c_uint32(stream), ctypes.c_uint32(counter), pauli.ctypes.data_as(ip),
        jump.ctypes.data_as(ip)))
    return pauli, jump


class DtcEngine:
    """Owns one device context of libdtc_hip.so."""

    def __init__(self, device: int = 0):
        self._lib = _capi.load_library()
        ctx = ctypes.c_void_p()
        _capi.check(self._lib.dtc_open(int(device), ctypes.byref(ctx)))
        self._ctx = ctx
        self.device = device

    def close(self):
        if getattr(self, "_ctx", None) is not None and self._ctx.value:
            self._lib.dtc_close(self._ctx)
            self._ctx = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- structs -------------------------------------------------------
    @staticmethod
    def _problem(spec: SweepSpec, want_fwd=True, want_echo=True, batch=0, t_first=0):
        pr = _capi.DtcProblem()
        pr.L = spec.L
        pr.T = spec.T
        pr.n_inst = spec.n_inst
        pr.probe_site = spec.probe_site
        pr.t_offset = spec.t_offset
        pr.n_sub = spec.n_sub
        pr.init_mask = spec.init_mask
        pr.h = _capi.as_dptr(spec.hs)
        pr.phi = _capi.as_dptr(spec.phis)
        pr.kick = _capi.as_dptr(spec.kick)
        pr.want_fwd = int(bool(want_fwd))
        pr.want_echo = int(bool(want_echo))
        pr.batch = int(batch)
        pr.t_first = int(t_first)
        return pr

    @staticmethod
    def _noise(spec: SweepSpec):
        nz = _capi.DtcNoise()
        nz.p = spec.p
        nz.n_anc = N_ANCILLA_NOISY_GATES
        return nz

    @staticmethod
    def _device(spec: SweepSpec):
        """dtc_device_noise of ``spec.device`` (None without one)."""
        if spec.device is None:
            return None
        if spec.device.L != spec.L:
            raise ValueError("device noise has a different number of sites")
        return _capi.device_struct(spec.device)

    # -- API -------------------------------------------------------------
    def autocorr(self, spec: SweepSpec, n_traj: int, seed: int = 0x5EED0001,
                 traj_offset: int = 0, want_fwd: bool = True, want_echo: bool = True,
                 want_zsite: bool = False, batch: int = 0, t_first: int = 0):
        """Per-trajectory ancilla expectations.

        Returns dict with ``fwd``/``echo`` of shape [n_inst][n_traj][T] and
        optionally ``zsite`` [n_inst][n_traj][T][L] (forward <Z_i>(t)).
        """
        n_inst, T, L = spec.n_inst, spec.T, spec.L
        fwd = np.zeros((n_inst, n_traj, T)) if want_fwd else None
        echo = np.zeros((n_inst, n_traj, T)) if want_echo else None
        zs = np.zeros((n_inst, n_traj, T, L)) if want_zsite else None
        pr = self._problem(spec, want_fwd, want_echo, batch, t_first)
        if spec.has_bond_noise:
            # with spec.device: device-like kick noise plus the bond channel
            dv = self._device(spec)
            nz = self._noise(spec)
            bd = bond_struct(spec.bond_noise)
            _capi.check(self._lib.dtc_autocorr_bond(
                self._ctx, ctypes.byref(pr), ctypes.byref(nz),
                ctypes.byref(dv) if dv is not None else None, ctypes.byref(bd),
                ctypes.c_uint64(seed), ctypes.c_int64(traj_offset), ctypes.c_int32(n_traj),
                _capi.as_dptr(fwd), _capi.as_dptr(echo), _capi.as_dptr(zs)))
        elif spec.device is not None:
            # device-like noise (include/dtc.h dtc_device_noise); spec.noise_prob unused
            if spec.device.L != spec.L:
                raise ValueError("device noise has a different number of sites")
            dv = _capi.device_struct(spec.device)
            _capi.check(self._lib.dtc_autocorr_device(
                self._ctx, ctypes.byref(pr), ctypes.byref(dv), ctypes.c_uint64(seed),
                ctypes.c_int64(traj_offset), ctypes.c_int32(n_traj), _capi.as_dptr(fwd),
                _capi.as_dptr(echo), _capi.as_dptr(zs)))
        else:
            nz = self._noise(spec)
            _capi.check(self._lib.dtc_autocorr(
                self._ctx, ctypes.byref(pr), ctypes.byref(nz), ctypes.c_uint64(seed),
                ctypes.c_int64(traj_offset), ctypes.c_int32(n_traj), _capi.as_dptr(fwd),
                _capi.as_dptr(echo), _capi.as_dptr(zs)))
        out = {}
        if want_fwd:
            out["fwd"] = fwd
        if want_echo:
            out["echo"] = echo
        if want_zsite:
            out["zsite"] = zs
        return out

    # -- forward prefix cache (dtc_prefix_*; user: control.optimize_g) ------
    @staticmethod
    def bond_draws(p_bond, L: int, seed: int, traj: int, stream: int, counter: int):
        """The bond-noise Pauli pairs of one diagonal layer (module ``bond_draws``)."""
        return bond_draws(p_bond, L, seed, traj, stream, counter)

    @staticmethod
    def kick_draws(L: int, n_sub: int, seed: int, traj: int, stream: int, counter: int,
                   p: float = 0.0, device=None):
        """The kick sub-gates' Pauli codes and jump flags of one layer (module
        ``kick_draws``)."""
        return kick_draws(L, n_sub, seed, traj, stream, counter, p, device)

    def prefix_build(self, spec: SweepSpec, n_traj: int, n_periods: int,
                     seed: int = 0x5EED0001, traj_offset: int = 0):
        """Keep every trajectory's state after periods 1..n_periods on the device."""
        refuse_bond_noise(spec, "prefix_build")
        pr = self._problem(spec)
        dv = _capi.device_struct(spec.device) if spec.device is not None else None
        _capi.check(self._lib.dtc_prefix_build(
            self._ctx, ctypes.byref(pr), ctypes.byref(self._noise(spec)),
            ctypes.byref(dv) if dv is not None else None, ctypes.c_uint64(seed),
            ctypes.c_int64(traj_offset), ctypes.c_int32(n_traj), ctypes.c_int32(n_periods)))

    def autocorr_prefixed(self, spec: SweepSpec, n_traj: int, seed: int = 0x5EED0001,
                          traj_offset: int = 0, want_fwd: bool = True, want_echo: bool = True,
                          t_first: int = 0, batch: int = 0):
        """``autocorr`` continuing from the prefix (periods after it and every
        echo drawn from ``seed``); same outputs without ``zsite``."""
        refuse_bond_noise(spec, "autocorr_prefixed")
        n_inst, T = spec.n_inst, spec.T
        fwd = np.zeros((n_inst, n_traj, T)) if want_fwd else None
        echo = np.zeros((n_inst, n_traj, T)) if want_echo else None
        pr = self._problem(spec, want_fwd, want_echo, batch, t_first)
        dv = _capi.device_struct(spec.device) if spec.device is not None else None
        _capi.check(self._lib.dtc_autocorr_prefixed(
            self._ctx, ctypes.byref(pr), ctypes.byref(self._noise(spec)),
            ctypes.byref(dv) if dv is not None else None, ctypes.c_uint64(seed),
            ctypes.c_int64(traj_offset), ctypes.c_int32(n_traj), _capi.as_dptr(fwd),
            _capi.as_dptr(echo)))
        out = {}
        if want_fwd:
            out["fwd"] = fwd
        if want_echo:
            out["echo"] = echo
        return out

    def prefix_release(self):
        _capi.check(self._lib.dtc_prefix_release(self._ctx))

    def apply_periods(self, spec: SweepSpec, state: np.ndarray, first_period: int,
                      n_periods: int, inverse: bool = False, inst: int = 0, traj: int = 0,
                      stream: int = 0, seed: int = 0x5EED0001):
        """Apply periods to a host statevector (complex128 [2^L]); returns
        ``(new_state, [norm, <Z_0>, ..., <Z_{L-1}>])``."""
        psi = np.ascontiguousarray(state, dtype=np.complex128).copy()
        if psi.shape != (1 << spec.L,):
            raise ValueError("state must have 2^L amplitudes")
        buf = psi.view(np.float64)
        z = np.zeros(1 + spec.L)
        pr = self._problem(spec)
        nz = self._noise(spec)
        _capi.check(self._lib.dtc_apply_periods(
            self._ctx, ctypes.byref(pr), ctypes.byref(nz), ctypes.c_uint64(seed),
            ctypes.c_int32(inst), ctypes.c_int64(traj), ctypes.c_uint32(stream),
            ctypes.c_int32(first_period), ctypes.c_int32(n_periods),
            ctypes.c_int32(int(inverse)), _capi.as_dptr(buf), _capi.as_dptr(z)))
        return psi, z

    def energy(self, spec: SweepSpec, n_traj: int, seed: int = 0x5EED0001,
               traj_offset: int = 0, batch: int = 0):
        """Per-trajectory energy observables of the forward sweep (dtc_energy,
        or dtc_energy_device when ``spec.device`` is set: Kraus-weighted
        expectations, read-out error not applied): ``z`` [n_inst][n_traj][T][L],
        ``zz`` [..][L-1], ``x`` [..][L]."""
        refuse_bond_noise(spec, "energy", "DtcEngine.energy_bond")
        n_inst, T, L = spec.n_inst, spec.T, spec.L
        z = np.zeros((n_inst, n_traj, T, L))
        zz = np.zeros((n_inst, n_traj, T, max(L - 1, 0)))
        x = np.zeros((n_inst, n_traj, T, L))
        pr = self._problem(spec, True, False, batch, 0)
        outs = (_capi.as_dptr(z), _capi.as_dptr(zz) if L > 1 else None, _capi.as_dptr(x))
        if spec.device is not None:
            if spec.device.L != spec.L:
                raise ValueError("device noise has a different number of sites")
            dv = _capi.device_struct(spec.device)
            _capi.check(self._lib.dtc_energy_device(
                self._ctx, ctypes.byref(pr), ctypes.byref(dv), ctypes.c_uint64(seed),
                ctypes.c_int64(traj_offset), ctypes.c_int32(n_traj), *outs))
        else:
            _capi.check(self._lib.dtc_energy(
                self._ctx, ctypes.byref(pr), ctypes.byref(self._noise(spec)),
                ctypes.c_uint64(seed), ctypes.c_int64(traj_offset), ctypes.c_int32(n_traj),
                *outs))
        return {"z": z, "zz": zz, "x": x}

    def energy_sums(self, spec: SweepSpec, n_traj: int, seed: int = 0x5EED0001,
                    traj_offset: int = 0, batch: int = 0):
        """``energy``'s observables summed over each instance's ``n_traj``
        trajectories on the device (dtc_energy_sums; device-like noise when
        ``spec.device`` is set): ``z`` [n_inst][T][L], ``zz`` [..][L-1], ``x``
        [..][L].  Divide by ``n_traj`` for the estimator's means."""
        refuse_bond_noise(spec, "energy_sums", "DtcEngine.energy_sums_bond")
        n_inst, T, L = spec.n_inst, spec.T, spec.L
        z = np.zeros((n_inst, T, L))
        zz = np.zeros((n_inst, T, max(L - 1, 0)))
        x = np.zeros((n_inst, T, L))
        pr = self._problem(spec, True, False, batch, 0)
        dv = None
        if spec.device is not None:
            if spec.device.L != spec.L:
                raise ValueError("device noise has a different number of sites")
            dv = _capi.device_struct(spec.device)
        _capi.check(self._lib.dtc_energy_sums(
            self._ctx, ctypes.byref(pr), ctypes.byref(self._noise(spec)),
            ctypes.byref(dv) if dv is not None else None, ctypes.c_uint64(seed),
            ctypes.c_int64(traj_offset), ctypes.c_int32(n_traj), _capi.as_dptr(z),
            _capi.as_dptr(zz) if L > 1 else None, _capi.as_dptr(x)))
        return {"z": z, "zz": zz, "x": x}

    def _energy_echo(self, fn, spec: SweepSpec, lead: tuple, n_traj: int, seed: int,
                     traj_offset: int, batch: int, t_first: int):
        T, L = spec.T, spec.L
        z = np.zeros(lead + (T, L))
        zz = np.zeros(lead + (T, max(L - 1, 0)))
        x = np.zeros(lead + (T, L))
        pr = self._problem(spec, False, True, batch, t_first)
        _capi.check(fn(
            self._ctx, ctypes.byref(pr), ctypes.byref(self._noise(spec)), ctypes.c_uint64(seed),
            ctypes.c_int64(traj_offset), ctypes.c_int32(n_traj), _capi.as_dptr(z),
            _capi.as_dptr(zz) if L > 1 else None, _capi.as_dptr(x)))
        return {"z": z, "zz": zz, "x": x}

    def energy_echo(self, spec: SweepSpec, n_traj: int, seed: int = 0x5EED0001,
                    traj_offset: int = 0, batch: int = 0, t_first: int = 0):
        """``energy``'s observables of the Loschmidt echo (dtc_energy_echo): row t
        is taken on the forward state after t + t_offset periods followed by as
        many inverse periods -- the state ``autocorr`` measures its echo on, the
        same trajectory bit for bit.  Rows before ``t_first`` stay 0.
        Depolarizing or noiseless kicks only."""
        refuse_energy_echo(spec, "energy_echo")
        return self._energy_echo(self._lib.dtc_energy_echo, spec, (spec.n_inst, n_traj), n_traj,
                                 seed, traj_offset, batch, t_first)

    def energy_echo_sums(self, spec: SweepSpec, n_traj: int, seed: int = 0x5EED0001,
                         traj_offset: int = 0, batch: int = 0, t_first: int = 0):
        """``energy_echo`` summed over each instance's trajectories on the device
        (dtc_energy_echo_sums); shapes of ``energy_sums``."""
        refuse_energy_echo(spec, "energy_echo_sums")
        return self._energy_echo(self._lib.dtc_energy_echo_sums, spec, (spec.n_inst,), n_traj,
                                 seed, traj_offset, batch, t_first)

    def _energy_bond(self, fn, spec: SweepSpec, lead: tuple, n_traj: int, seed: int,
                     traj_offset: int, batch: int):
        T, L = spec.T, spec.L
        z = np.zeros(lead + (T, L))
        zz = np.zeros(lead + (T, max(L - 1, 0)))
        x = np.zeros(lead + (T, L))
        pr = self._problem(spec, True, False, batch, 0)
        dv = self._device(spec)
        bd = bond_struct(spec.bond_noise) if spec.has_bond_noise else None
        _capi.check(fn(
            self._ctx, ctypes.byref(pr), ctypes.byref(self._noise(spec)),
            ctypes.byref(dv) if dv is not None else None,
            ctypes.byref(bd) if bd is not None else None, ctypes.c_uint64(seed),
            ctypes.c_int64(traj_offset), ctypes.c_int32(n_traj), _capi.as_dptr(z),
            _capi.as_dptr(zz) if L > 1 else None, _capi.as_dptr(x)))
        return {"z": z, "zz": zz, "x": x}

    def energy_bond(self, spec: SweepSpec, n_traj: int, seed: int = 0x5EED0001,
                    traj_offset: int = 0, batch: int = 0):
        """``energy`` with ``spec.bond_noise`` after every RZZ (dtc_energy_bond;
        depolarizing or device-like kick noise).  Without bond noise in the spec
        it returns ``energy``'s rows."""
        return self._energy_bond(self._lib.dtc_energy_bond, spec, (spec.n_inst, n_traj), n_traj,
                                 seed, traj_offset, batch)

    def energy_sums_bond(self, spec: SweepSpec, n_traj: int, seed: int = 0x5EED0001,
                         traj_offset: int = 0, batch: int = 0):
        """``energy_sums`` with ``spec.bond_noise`` after every RZZ
        (dtc_energy_sums_bond)."""
        return self._energy_bond(self._lib.dtc_energy_sums_bond, spec, (spec.n_inst,), n_traj,
                                 seed, traj_offset, batch)

    def sample(self, spec: SweepSpec, n_traj: int, n_shots: int = 1, bases: str = "zx",
               seed: int = 0x5EED0001, traj_offset: int = 0, batch: int = 0, t_first: int = 0):
        """Measurement outcomes of the forward sweep (dtc_sample): for every
        trajectory of ``energy`` and every time t, ``n_shots`` bitstrings per
        requested basis, ``{"z": uint64 [n_inst][n_traj][T][n_shots], "x": ...}``
        (site i = bit i; in ``x`` a set bit means X_i = -1).  Rows before
        ``t_first`` stay 0.  Depolarizing or noiseless kicks only."""
        refuse_sample(spec, "sample")
        bases = str(bases).lower()
        if not bases or set(bases) - set("zx"):
            raise ValueError(f"bases must name 'z', 'x' or both, got {bases!r}")
        shape = (spec.n_inst, int(n_traj), spec.T, int(n_shots))
        out = {b: np.zeros(shape, dtype=np.uint64) for b in "zx" if b in bases}
        up = ctypes.POINTER(ctypes.c_uint64)
        pr = self._problem(spec, True, False, batch, t_first)
        _capi.check(self._lib.dtc_sample(
            self._ctx, ctypes.byref(pr), ctypes.byref(self._noise(spec)), ctypes.c_uint64(seed),
            ctypes.c_int64(traj_offset), ctypes.c_int32(n_traj), ctypes.c_int32(n_shots),
            out["z"].ctypes.data_as(up) if "z" in out else None,
            out["x"].ctypes.data_as(up) if "x" in out else None))
        return out

    def _correlations(self, fn: str, what: str, spec: SweepSpec, lead: tuple, n_traj: int,
                      bases: str, seed: int, traj_offset: int, batch: int, t_first: int):
        refuse_correlations(spec, what)
        bases = str(bases).lower()
        if not bases or set(bases) - set("zx"):
            raise ValueError(f"bases must name 'z', 'x' or both, got {bases!r}")
        T, L = spec.T, spec.L
        out = {}
        for b in "zx":
            if b in bases:
                out[b] = np.zeros(lead + (T, L))
                out[2 * b] = np.zeros(lead + (T, L * (L - 1) // 2))
        pr = self._problem(spec, True, False, batch, t_first)
        _capi.check(getattr(self._lib, fn)(
            self._ctx, ctypes.byref(pr), ctypes.byref(self._noise(spec)), ctypes.c_uint64(seed),
            ctypes.c_int64(traj_offset), ctypes.c_int32(n_traj),
            *(_capi.as_dptr(out.get(k)) for k in ("z", "zz", "x", "xx"))))
        return out

    def correlations(self, spec: SweepSpec, n_traj: int, bases: str = "z",
                     seed: int = 0x5EED0001, traj_offset: int = 0, batch: int = 0,
                     t_first: int = 0):
        """All-pair correlators of the forward sweep (dtc_correlations): for every
        trajectory of ``energy`` and every time t, ``z`` [n_inst][n_traj][T][L] =
        <Z_i> and ``zz`` [n_inst][n_traj][T][L(L-1)/2] = <Z_i Z_j>, i < j, in the
        order of ``correlations.pair_index``; with "x" in ``bases`` also ``x`` and
        ``xx`` (<X_i>, <X_i X_j>).  Rows before ``t_first`` stay 0.  Depolarizing
        or noiseless kicks only."""
        return self._correlations("dtc_correlations", "correlations", spec,
                                  (spec.n_inst, int(n_traj)), n_traj, bases, seed, traj_offset,
                                  batch, t_first)

    def correlation_sums(self, spec: SweepSpec, n_traj: int, bases: str = "z",
                         seed: int = 0x5EED0001, traj_offset: int = 0, batch: int = 0,
                         t_first: int = 0):
        """``correlations`` summed over each instance's ``n_traj`` trajectories on
        the device (dtc_correlation_sums): [n_inst][T][.].  Divide by ``n_traj``
        for the means."""
        return self._correlations("dtc_correlation_sums", "correlation_sums", spec,
                                  (spec.n_inst,), n_traj, bases, seed, traj_offset, batch, t_first)

    def _rdm(self, fn: str, what: str, spec: SweepSpec, lead: tuple, n_traj: int, windows,
             seed: int, traj_offset: int, batch: int, t_first: int) -> np.ndarray:
        refuse_rdm(spec, what)
        win = window_array(windows)
        n_win, k = win.shape
        if not 1 <= k <= 4:
            raise ValueError(f"window size must be in [1, 4], got {k}")
        d = 1 << k
        rho = np.zeros(lead + (spec.T, n_win, d, d), dtype=np.complex128)
        pr = self._problem(spec, True, False, batch, t_first)
        _capi.check(getattr(self._lib, fn)(
            self._ctx, ctypes.byref(pr), ctypes.byref(self._noise(spec)), ctypes.c_uint64(seed),
            ctypes.c_int64(traj_offset), ctypes.c_int32(n_traj),
            win.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), ctypes.c_int32(n_win),
            ctypes.c_int32(k), _capi.as_dptr(rho.view(np.float64))))
        return rho

    def rdm(self, spec: SweepSpec, n_traj: int, windows, seed: int = 0x5EED0001,
            batch: int = 0, traj_offset: int = 0, t_first: int = 0) -> np.ndarray:
        """Reduced density matrices of site windows of the forward sweep
        (dtc_rdm): complex128 [n_inst][n_traj][T][n_win][d][d], d = 2^k, for every
        trajectory of ``energy`` and every time t.  ``windows`` is one window or a
        list of windows of one size k <= 4, each strictly ascending; bit m of a
        row index is the bit of the window's m-th site.  Rows before ``t_first``
        stay 0.  Depolarizing or noiseless kicks only."""
        return self._rdm("dtc_rdm", "rdm", spec, (spec.n_inst, int(n_traj)), n_traj, windows,
                         seed, traj_offset, batch, t_first)

    def rdm_sums(self, spec: SweepSpec, n_traj: int, windows, seed: int = 0x5EED0001,
                 batch: int = 0, traj_offset: int = 0, t_first: int = 0) -> np.ndarray:
        """``rdm`` summed over each instance's ``n_traj`` trajectories on the
        device (dtc_rdm_sums): [n_inst][T][n_win][d][d].  Divide by ``n_traj``
        for the noise-averaged state."""
        return self._rdm("dtc_rdm_sums", "rdm_sums", spec, (spec.n_inst,), n_traj, windows,
                         seed, traj_offset, batch, t_first)

    def rdm_block_sums(self, spec: SweepSpec, n_traj: int, blocks, seed: int = 0x5EED0001,
                       traj_offset: int = 0, batch: int = 0, t_first: int = 0) -> dict:
        """Reduced density matrices of blocks of contiguous sites of the forward
        sweep (dtc_rdm_block_sums).  ``blocks`` is one ``(start, k)`` pair or a
        list of them of one size 5 <= k <= 10, 2 k <= L.  Returns ``rho_sum``,
        complex128 [n_inst][T][n_blk][d][d], the sum over each instance's
        trajectories of the per-state rho (divide by ``n_traj`` for the
        noise-averaged state); ``purity`` [n_inst][n_traj][T][n_blk], ``Tr rho^2``
        of every trajectory's own state (``-ln`` of it: the trajectory-resolved
        second Renyi entanglement entropy); ``blocks`` int32 [n_blk][2].  Rows
        before ``t_first`` stay 0.  Depolarizing or noiseless kicks only."""
        refuse_rdm(spec, "rdm_block_sums")
        blk = block_array(blocks)
        n_blk, k = blk.shape[0], int(blk[0, 1])
        if not 5 <= k <= 10:
            raise ValueError(f"block size must be in [5, 10], got {k} (k <= 4: rdm)")
        d = 1 << k
        n_traj = int(n_traj)
        starts = np.ascontiguousarray(blk[:, 0])
        rho = np.zeros((spec.n_inst, spec.T, n_blk, d, d), dtype=np.complex128)
        pur = np.zeros((spec.n_inst, n_traj, spec.T, n_blk))
        pr = self._problem(spec, True, False, batch, t_first)
        _capi.check(self._lib.dtc_rdm_block_sums(
            self._ctx, ctypes.byref(pr), ctypes.byref(self._noise(spec)), ctypes.c_uint64(seed),
            ctypes.c_int64(traj_offset), ctypes.c_int32(n_traj),
            starts.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), ctypes.c_int32(n_blk),
            ctypes.c_int32(k), _capi.as_dptr(rho.view(np.float64)), _capi.as_dptr(pur)))
        return {"rho_sum": rho, "purity": pur, "blocks": blk}

    # -- sharded state (dtc_shard_*; driver: sharded.py) ----------------
    def shard_set_basis(self, spec: SweepSpec, shard, state_ptr: int, seed: int = 0x5EED0001,
                        traj: int = 0):
        """Prepare the (noisy-prep) product state in device buffer ``state_ptr``."""
        _capi.check(self._lib.dtc_shard_set_basis(
            self._ctx, ctypes.byref(self._problem(spec)), ctypes.byref(self._noise(spec)),
            ctypes.byref(shard), ctypes.c_uint64(seed), ctypes.c_int64(traj),
            ctypes.c_void_p(state_ptr)))

    def shard_step(self, spec: SweepSpec, shard, period: int, pre_mask: int, diag: bool,
                   post_mask: int, src_ptr: int, dst_ptr: int, want_obs: bool = False,
                   seed: int = 0x5EED0001, traj: int = 0, inst: int = 0):
        """dst = K_{period+1}[post] . D^diag . K_period[pre] . src on every shard held;
        returns obs [n_shards][1 + n_local] (or None)."""
        obs = np.zeros((shard.n_shards, 1 + shard.n_local)) if want_obs else None
        _capi.check(self._lib.dtc_shard_step(
            self._ctx, ctypes.byref(self._problem(spec)), ctypes.byref(self._noise(spec)),
            ctypes.byref(shard), ctypes.c_uint64(seed), ctypes.c_int64(traj),
            ctypes.c_int32(inst), ctypes.c_int32(period), ctypes.c_uint64(pre_mask),
            ctypes.c_int32(int(bool(diag))), ctypes.c_uint64(post_mask),
            ctypes.c_void_p(src_ptr), ctypes.c_void_p(dst_ptr), _capi.as_dptr(obs)))
        return obs

    def shard_step_async(self, spec: SweepSpec, shard, period: int, pre_mask: int, diag: bool,
                         post_mask: int, src_ptr: int, dst_ptr: int, obs_ptr: int | None = None,
                         seed: int = 0x5EED0001, traj: int = 0, inst: int = 0):
        """shard_step enqueued on the engine stream without waiting; obs_ptr
        (device, [n_shards][1 + n_local] doubles) receives the observables."""
        _capi.check(self._lib.dtc_shard_step_async(
            self._ctx, ctypes.byref(self._problem(spec)), ctypes.byref(self._noise(spec)),
            ctypes.byref(shard), ctypes.c_uint64(seed), ctypes.c_int64(traj),
            ctypes.c_int32(inst), ctypes.c_int32(period), ctypes.c_uint64(pre_mask),
            ctypes.c_int32(int(bool(diag))), ctypes.c_uint64(post_mask),
            ctypes.c_void_p(src_ptr), ctypes.c_void_p(dst_ptr),
            ctypes.c_void_p(obs_ptr) if obs_ptr else None))

    def shard_kick_slice(self, spec: SweepSpec, shard, period: int, pre_mask: int,
                         chunk_bits: int, slice_bits: int, slice_: int, state_ptr: int,
                         seed: int = 0x5EED0001, traj: int = 0):
        """K_period on the local bits pre_mask of slice `slice_` of every chunk
        (top chunk_bits local bits; the next slice_bits number the slices) of
        every shard held, in place, asynchronously (one launch)."""
        _capi.check(self._lib.dtc_shard_kick_slice(
            self._ctx, ctypes.byref(self._problem(spec)), ctypes.byref(self._noise(spec)),
            ctypes.byref(shard), ctypes.c_uint64(seed), ctypes.c_int64(traj),
            ctypes.c_int32(period), ctypes.c_uint64(pre_mask), ctypes.c_int32(chunk_bits),
            ctypes.c_int32(slice_bits), ctypes.c_int32(slice_), ctypes.c_void_p(state_ptr)))

    def release_buffers(self, drop_prefix: bool = True):
        """Free the engine's batch work buffers (dtc_release_buffers) and, by
        default, the forward prefix (dtc_prefix_release) -- all the engine's
        large device memory, e.g. before one 256 GiB sharded state; the next
        call re-allocates what it needs."""
        if drop_prefix:
            _capi.check(self._lib.dtc_prefix_release(self._ctx))
        _capi.check(self._lib.dtc_release_buffers(self._ctx))

    def shard_exchange_slice(self, shard, slice_bits: int, slice_: int, state_ptr: int):
        """Virtual ranks (every shard in ``state_ptr``): the all-to-all of slice
        ``slice_`` in place -- piece (shard r, chunk c) <-> (shard c, chunk r) --
        asynchronously on the engine stream (one launch)."""
        _capi.check(self._lib.dtc_shard_exchange_slice(
            self._ctx, ctypes.byref(shard), ctypes.c_int32(slice_bits), ctypes.c_int32(slice_),
            ctypes.c_void_p(state_ptr)))

    def shard_kick_exchange_slice(self, spec: SweepSpec, shard, period: int, pre_mask: int,
                                  slice_bits: int, slice_: int, state_ptr: int,
                                  seed: int = 0x5EED0001, traj: int = 0):
        """Virtual ranks: ``shard_kick_slice`` (chunk bits = n_global) and
        ``shard_exchange_slice`` of slice ``slice_`` as one step -- the last
        site group's kick pass stores each piece at its partner's place
        (dtc_shard_kick_exchange_slice), so the exchange moves no bytes of its
        own."""
        _capi.check(self._lib.dtc_shard_kick_exchange_slice(
            self._ctx, ctypes.byref(self._problem(spec)), ctypes.byref(self._noise(spec)),
            ctypes.byref(shard), ctypes.c_uint64(seed), ctypes.c_int64(traj),
            ctypes.c_int32(period), ctypes.c_uint64(pre_mask), ctypes.c_int32(slice_bits),
            ctypes.c_int32(slice_), ctypes.c_void_p(state_ptr)))

    # -- the echo on a sharded state: layer k of chain t in place of `period` --
    def shard_echo_step(self, spec: SweepSpec, shard, t: int, k: int, pre_mask: int, diag: bool,
                        post_mask: int, src_ptr: int, dst_ptr: int | None,
                        want_obs: bool = False, seed: int = 0x5EED0001, traj: int = 0,
                        inst: int = 0):
        """dst = L_{k+1}[post] . (D*)^diag . L_k[pre] . src on every shard held
        (dtc_shard_echo_step: L_0 undoes the forward layer that ran ahead, L_k
        is the inverse kick K'_k of chain t); returns obs or None.  ``dst_ptr``
        None: the chain's measure-only end (needs ``want_obs``)."""
        obs = np.zeros((shard.n_shards, 1 + shard.n_local)) if want_obs else None
        _capi.check(self._lib.dtc_shard_echo_step(
            self._ctx, ctypes.byref(self._problem(spec)), ctypes.byref(self._noise(spec)),
            ctypes.byref(shard), ctypes.c_uint64(seed), ctypes.c_int64(traj),
            ctypes.c_int32(inst), ctypes.c_int32(t), ctypes.c_int32(k),
            ctypes.c_uint64(pre_mask), ctypes.c_int32(int(bool(diag))),
            ctypes.c_uint64(post_mask), ctypes.c_void_p(src_ptr),
            ctypes.c_void_p(dst_ptr) if dst_ptr else None, _capi.as_dptr(obs)))
        return obs

    def shard_echo_step_async(self, spec: SweepSpec, shard, t: int, k: int, pre_mask: int,
                              diag: bool, post_mask: int, src_ptr: int, dst_ptr: int | None,
                              obs_ptr: int | None = None, seed: int = 0x5EED0001,
                              traj: int = 0, inst: int = 0):
        """shard_echo_step enqueued on the engine stream without waiting
        (dtc_shard_echo_step_async); obs_ptr is a device array."""
        _capi.check(self._lib.dtc_shard_echo_step_async(
            self._ctx, ctypes.byref(self._problem(spec)), ctypes.byref(self._noise(spec)),
            ctypes.byref(shard), ctypes.c_uint64(seed), ctypes.c_int64(traj),
            ctypes.c_int32(inst), ctypes.c_int32(t), ctypes.c_int32(k),
            ctypes.c_uint64(pre_mask), ctypes.c_int32(int(bool(diag))),
            ctypes.c_uint64(post_mask), ctypes.c_void_p(src_ptr),
            ctypes.c_void_p(dst_ptr) if dst_ptr else None,
            ctypes.c_void_p(obs_ptr) if obs_ptr else None))

    def shard_echo_kick_slice(self, spec: SweepSpec, shard, t: int, k: int, pre_mask: int,
                              chunk_bits: int, slice_bits: int, slice_: int, state_ptr: int,
                              seed: int = 0x5EED0001, traj: int = 0):
        """``shard_kick_slice`` with layer k of chain t (dtc_shard_echo_kick_slice)."""
        _capi.check(self._lib.dtc_shard_echo_kick_slice(
            self._ctx, ctypes.byref(self._problem(spec)), ctypes.byref(self._noise(spec)),
            ctypes.byref(shard), ctypes.c_uint64(seed), ctypes.c_int64(traj),
            ctypes.c_int32(t), ctypes.c_int32(k), ctypes.c_uint64(pre_mask),
            ctypes.c_int32(chunk_bits), ctypes.c_int32(slice_bits), ctypes.c_int32(slice_),
            ctypes.c_void_p(state_ptr)))

    def shard_echo_kick_exchange_slice(self, spec: SweepSpec, shard, t: int, k: int,
                                       pre_mask: int, slice_bits: int, slice_: int,
                                       state_ptr: int, seed: int = 0x5EED0001, traj: int = 0):
        """``shard_kick_exchange_slice`` with layer k of chain t
        (dtc_shard_echo_kick_exchange_slice)."""
        _capi.check(self._lib.dtc_shard_echo_kick_exchange_slice(
            self._ctx, ctypes.byref(self._problem(spec)), ctypes.byref(self._noise(spec)),
            ctypes.byref(shard), ctypes.c_uint64(seed), ctypes.c_int64(traj),
            ctypes.c_int32(t), ctypes.c_int32(k), ctypes.c_uint64(pre_mask),
            ctypes.c_int32(slice_bits), ctypes.c_int32(slice_), ctypes.c_void_p(state_ptr)))

    def stream_handle(self) -> int:
        """The engine's hipStream_t (for torch.cuda.ExternalStream)."""
        h = ctypes.c_void_p()
        _capi.check(self._lib.dtc_get_stream(self._ctx, ctypes.byref(h)))
        return int(h.value or 0)

    def synchronize(self):
        _capi.check(self._lib.dtc_synchronize(self._ctx))

    # -- profiling -------------------------------------------------------
    def set_profiling(self, on: bool):
        _capi.check(self._lib.dtc_set_profiling(self._ctx, int(on)))

    def reset_stats(self):
        _capi.check(self._lib.dtc_reset_stats(self._ctx))

    def kernel_stats(self):
        out = {}
        for k in range(_capi.KERNEL_KINDS):
            n = ctypes.c_int64()
            ms = ctypes.c_double()
            by = ctypes.c_double()
            _capi.check(self._lib.dtc_kernel_stats(self._ctx, k, ctypes.byref(n),
                                                   ctypes.byref(ms), ctypes.byref(by)))
            out[k] = {"launches": n.value, "total_ms": ms.value, "bytes": by.value}
        return out

    def lightcone_counts(self):
        """Light-cone ends launched since the engine opened, by kernel
        (dtc_lightcone_counts): 8-site window, 10-site generic, 10-site C2 form,
        12-site C2 form."""
        c = (ctypes.c_int64 * 4)()
        _capi.check(self._lib.dtc_lightcone_counts(self._ctx, c))
        return {"lc8": c[0], "lcw": c[1], "lcw2": c[2], "lcw3": c[3]}

    def schedule_counts(self):
        """Batch schedules built since the engine opened (dtc_schedule_counts):
        echo chains folded into a dual pass, device-noise batches whose forward
        ran a layer ahead, device-noise batches run with K-D forward passes
        (a chain did not fold, or DTC_NO_RUNAHEAD=1), and batches run with the
        13 / 7 site split of L = 20."""
        c = (ctypes.c_int64 * 4)()
        _capi.check(self._lib.dtc_schedule_counts(self._ctx, c))
        return {"folded": c[0], "device_runahead": c[1], "device_kd": c[2], "split13": c[3]}

    def wavefront_count(self):
        """Wavefront passes launched since the engine opened
        (dtc_wavefront_count; 0 with DTC_NO_WAVEFRONT=1)."""
        c = ctypes.c_int64()
        _capi.check(self._lib.dtc_wavefront_count(self._ctx, ctypes.byref(c)))
        return int(c.value)

    def device_info(self):
        name = ctypes.create_string_buffer(256)
        ncu = ctypes.c_int32()
        mem = ctypes.c_double()
        _capi.check(self._lib.dtc_device_info(self._ctx, name, 256, ctypes.byref(ncu),
                                              ctypes.byref(mem)))
        return {"name": name.value.decode(), "n_cu": ncu.value, "hbm_bytes": mem.value}


def spec_n_sub(polarization: str) -> int:
    return n_sub_of(polarization)
