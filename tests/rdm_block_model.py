"""A numpy restatement of the block density-matrix kernels' index algebra
(csrc/dtc_rdm_block.h; test infrastructure only): the kernel's row bits of a
block, the amplitude of a (row, column) pair, and the amplitudes one load
instruction of the Gram kernel reads."""
import numpy as np

PANEL = CHUNK = 64
THREADS = 512          # the Gram kernel's workgroup
REGS = 4096 // THREADS


def geometry(start, k, L_eff):
    """(ae, ke, m): the kernel works on ke = max(k, 6) row bits from position ae;
    a five-site block takes the bit above it as pad, or the bit below where the
    state has none above."""
    ke, ae = max(k, 6), start
    if ke > k and start + ke > L_eff:
        ae = start - 1
    return ae, ke, min(ae, 6)


def amp_index(ae, ke, r, c):
    r = np.asarray(r, dtype=np.int64)
    c = np.asarray(c, dtype=np.int64)
    return ((c >> ae) << (ae + ke)) | (r << ae) | (c & ((1 << ae) - 1))


def local_row(v, m):
    return (v >> m) & (PANEL - 1)


def local_col(v, m):
    return (v & ((1 << m) - 1)) | ((v >> (m + 6)) << m)


def staged_loads(start, k, L_eff, panel, chunk):
    """[REGS * THREADS / 64][64]: the amplitudes each load instruction (one
    register of one wave) reads of row panel `panel`, column chunk `chunk`."""
    ae, ke, m = geometry(start, k, L_eff)
    t = np.arange(THREADS)
    out = []
    for j in range(REGS):
        v = t | (j << 9)
        x = amp_index(ae, ke, panel * PANEL + local_row(v, m), chunk * CHUNK + local_col(v, m))
        out.append(x.reshape(THREADS // 64, 64))
    return np.concatenate(out)
