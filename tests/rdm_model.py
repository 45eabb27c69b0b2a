"""The oracle side of the reduced-density-matrix tests (test infrastructure
only): rho of a host state by numpy reshape and matmul, the rows of one noisy
trajectory from the C oracle's states (tests/sample_model.trajectory_states),
and the depolarizing channel's exact rho_A by partial trace of the density
matrix of oracle.dm_oracle, stepped as tests/correlation_model.exact_channel
steps it."""
import numpy as np

from oracle import dm_oracle
from tests import correlation_model as cm
from tests import sample_model as sm

EPS = sm.EPS  # the project's standing figure for engine against oracle

# the trajectory-mean test (tests/test_rdm_cpu.py): the configuration of the
# correlators' channel test; every summand has modulus <= 1: bound 5 / sqrt(n)
CHANNEL = cm.CHANNEL
CHANNEL_WINDOWS = [(0,), (3,), (0, 1), (1, 3), (0, 1, 2), (0, 1, 2, 3)]

PAULI = {"I": np.eye(2, dtype=np.complex128),
         "X": np.array([[0, 1], [1, 0]], dtype=np.complex128),
         "Y": np.array([[0, -1j], [1j, 0]], dtype=np.complex128),
         "Z": np.array([[1, 0], [0, -1]], dtype=np.complex128)}


def _axes(L, sites):
    """Axes of a [2] * L array (axis a = bit L - 1 - a) with the window's sites
    first, most significant row bit (the last site) leading, then the rest."""
    front = [L - 1 - s for s in reversed(sites)]
    return front + [a for a in range(L) if a not in front]


def state_rdm(psi, L, sites):
    """rho [d][d] of the window: bit m of a row index is the bit of sites[m]."""
    sites = [int(s) for s in sites]
    d = 1 << len(sites)
    M = np.asarray(psi, dtype=np.complex128).reshape((2,) * L).transpose(_axes(L, sites))
    M = M.reshape(d, -1)
    return M @ M.conj().T


def matrix_rdm(rho, L, sites):
    """The same window of a full density matrix [2^L][2^L] by partial trace."""
    sites = [int(s) for s in sites]
    d = 1 << len(sites)
    ax = _axes(L, sites)
    R = np.asarray(rho, dtype=np.complex128).reshape((2,) * (2 * L))
    R = R.transpose(ax + [L + a for a in ax]).reshape(d, -1, d, (1 << L) // d)
    return np.einsum("acbc->ab", R)


def window_operator(letters):
    """kron(O_{s_{k-1}}, ..., O_{s_0}) for letters[m] on the window's m-th site."""
    op = np.ones((1, 1), dtype=np.complex128)
    for c in letters:
        op = np.kron(PAULI[c], op)
    return op


def trajectory_rows(spec, inst, traj, seed, windows):
    """[T][n_win][d][d] of one trajectory (windows of one size)."""
    d = 1 << len(windows[0])
    out = np.zeros((spec.T, len(windows), d, d), dtype=np.complex128)
    for t, psi in sm.trajectory_states(spec, inst, traj, seed):
        for w, sites in enumerate(windows):
            out[t, w] = state_rdm(psi, spec.L, sites)
    return out


def exact_channel(spec, windows, inst=0):
    """{sites: [T][d][d]} of the exact depolarizing channel: the density matrix
    of the vacuum stepped period by period (as correlation_model.exact_channel),
    partially traced to each window."""
    L, T = spec.L, spec.T
    assert spec.init_mask == 0 and spec.t_offset == 0
    rho0 = np.zeros((1 << L, 1 << L), dtype=np.complex128)
    rho0[0, 0] = 1.0
    rho = dm_oracle.DM(L, rho0)
    out = {tuple(w): np.zeros((T, 1 << len(w), 1 << len(w)), dtype=np.complex128)
           for w in windows}
    for t in range(T):
        if t > 0:
            dm_oracle._period(rho, 0, L, dm_oracle.kick_gates_from_table(spec.kick[t - 1]),
                              spec.hs[inst], spec.phis[inst], spec.p)
        full = rho.matrix()
        for w in out:
            out[w][t] = matrix_rdm(full, L, w)
    return out


def standard_windows(L):
    """The windows every GPU parity shape uses, grouped by size k."""
    return {
        4: [(0, 1, 2, 3), (L - 4, L - 3, L - 2, L - 1),
            (3, 7, L - 2, L - 1) if L >= 11 else (0, 2, L - 2, L - 1)],
        1: [(0,), (L - 1,)],
        2: [(1, 2), (0, L - 1)],
        3: [(0, L // 2, L - 1)],
    }
