"""Shared test helpers (random disorder, statistics)."""
import numpy as np


def random_disorder(rng, L, n_inst=1):
    hs = rng.uniform(-np.pi, np.pi, (n_inst, L))
    phis = rng.uniform(-1.5 * np.pi, -0.5 * np.pi, (n_inst, max(L - 1, 1)))
    return hs, phis


def shot_sigma(a, shots=1024):
    """Std of a (n0 - n1)/shots estimate with expectation a."""
    return np.sqrt(np.clip(1.0 - np.asarray(a) ** 2, 1e-4, None) / shots)


def chi2_per_dof(x, y, sx, sy):
    r = (np.asarray(x) - np.asarray(y)) / np.sqrt(np.asarray(sx) ** 2 + np.asarray(sy) ** 2)
    return float(np.mean(r ** 2)), float(np.max(np.abs(r)))


def harsh_device(pkg, L):
    """A device-like noise model with strong damping (the device tests')."""
    return pkg.DeviceNoise(p_gate=np.full(L, 0.02), t1_us=np.linspace(1.5, 3.0, L),
                           t2_us=np.linspace(1.0, 4.0, L), gate_ns=120.0, anc_factor=0.9,
                           readout_p01=0.02, readout_p10=0.035)


def implied_launch_counts(pkg, out_dir, args, n_groups, x_basis, measured_x):
    """The launches by profiling kind that the tools/schedule_check.cpp dump of a
    forward sweep (mode=energy / mode=sample, ``args``) implies for one batch:
    a stored pass with a diagonal is a lo pass, one without a hi pass, one that
    stores nothing a final pass; one reduce per reduce range of a measuring
    pass.  Behind every launch that leaves a time's state (t_state), with
    ``x_basis``: the basis change, one kick-only pass per site group, and with
    ``measured_x`` its reduce."""
    import subprocess

    from tests.test_schedule_cpu import PART_XPRE, PART_Z, build, parse

    r = subprocess.run([build(out_dir, []), *args], capture_output=True, text=True, check=True)
    sched = parse(r.stdout)
    c = pkg._capi
    n = {c.KERNEL_LO_PASS: 0, c.KERNEL_HI_PASS: 0, c.KERNEL_FINAL_PASS: 0, c.KERNEL_REDUCE: 0}
    for l in sched:
        kind = (c.KERNEL_FINAL_PASS if l["no_store"]
                else c.KERNEL_LO_PASS if l["ps"]["diag"] != "0" else c.KERNEL_HI_PASS)
        n[kind] += 1
        n[c.KERNEL_REDUCE] += bool(l["parts"] & PART_Z) + bool(l["parts"] & PART_XPRE)
        if "t_state" in l and x_basis:
            n[c.KERNEL_HI_PASS] += n_groups
            n[c.KERNEL_REDUCE] += bool(measured_x)
    return n, sum("t_state" in l for l in sched)
