"""The inputs of tests/test_gpu_wavefront_inputs.py: the L = 20 sweeps that take
the wavefront interior (csrc/dtc_wavefront.hip) away from the one point the other
wavefront files run it at -- one disorder instance, a scalar g, the probe on
site 10.

tests/test_wavefront_inputs_cpu.py dumps the schedule of every probe site with
tools/schedule_check.cpp and asserts that the cases below reach every wavefront
pass shape and every table-set key of that census; the GPU file runs them and
takes its launch counts from the same dumps.  A planner change that moves a
shape or a key out of these cases shows on the CPU first."""
from collections import namedtuple

L = 20
P_NOISE = 0.05

# name: the test id.  kick: "x" (RX kicks from the vacuum), "y" (RY kicks from the
# Neel state) or "xy_cycle" (RX for five periods, RY for the next five; the
# vacuum).  n_traj: per instance.  g_list: per-period g, linspace(0.84, 1.0,
# T - 1 + t_offset), else the scalar of the kind.  oracle: the states (instance
# * n_traj + trajectory) whose rows the C oracle checks.
Case = namedtuple("Case", "name probe T t_offset kick n_inst n_traj g_list oracle")


def _case(name, probe, T, t_offset, kick, n_inst=1, n_traj=8, g_list=False, oracle=(0, 7)):
    return Case(name, probe, T, t_offset, kick, n_inst, n_traj, g_list, tuple(oracle))


# Moved probes, one octet each.  Probes 0 .. 4 have no light-cone end and give
# tile 1 its trailing kick-less diagonal after 1, 3 and 4 kick steps (all three
# at probe 4, under RY kicks; every case but probe 5's runs at least one of
# them); (4, 12, 1) and (5, 11, 1) between them reach the whole census, the
# others are the sites where the tiles' geometry changes: the first site, the
# one both tiles hold (11), the column group's first (12) and the last.
PROBE_CASES = [
    _case("probe0-T8-x", 0, 8, 0, "x"),
    _case("probe4-T12-off1-y", 4, 12, 1, "y"),
    _case("probe5-T11-off1-x", 5, 11, 1, "x"),
    _case("probe11-T12-y", 11, 12, 0, "y"),
    _case("probe12-T10-x", 12, 10, 0, "x"),
    _case("probe19-T12-y", 19, 12, 0, "y"),
]

# Several disorder instances in one call: 2 x 12 states (the second octet
# straddles the instance edge at 11 | 12) and 3 x 3 (one octet holds three
# instances).
INSTANCE_CASES = [
    _case("inst2x12-probe4-T10-off1-x", 4, 10, 1, "x", n_inst=2, n_traj=12,
          oracle=(7, 8, 11, 12, 15, 16, 23)),
    _case("inst3x3-T11-y", 10, 11, 0, "y", n_inst=3, n_traj=3, oracle=(2, 3, 7, 8)),
]

# A kick row of its own per period.
G_LIST_CASES = [
    _case("glist-T12-x", 10, 12, 0, "x", g_list=True),
    _case("glist-probe17-T12-off1-y", 17, 12, 1, "y", g_list=True),
]

# Both kick families in one sweep: every interior run spans the RX | RY edge
# between periods 5 and 6, so the plain interior runs.
FALLBACK_CASES = [
    _case("xy_cycle-T12", 10, 12, 0, "xy_cycle", n_traj=9, oracle=(0, 7, 8)),
]

CASES = PROBE_CASES + INSTANCE_CASES + G_LIST_CASES + FALLBACK_CASES

# The census of tests/test_wavefront_inputs_cpu.py: every probe site, T = 8 .. 12,
# t_offset 0 / 1, the default layer cap.
CENSUS_PROBES = range(L)
CENSUS_T = range(8, 13)
CENSUS_T_OFFSETS = (0, 1)


def sched_args(case):
    """The tools/schedule_check.cpp arguments of a case's schedule (the tool's
    xy_cycle5 pattern is the package's xy_cycle polarization)."""
    kick = "xy_cycle5" if case.kick == "xy_cycle" else case.kick
    return ["L=%d" % L, "T=%d" % case.T, "t_offset=%d" % case.t_offset, "probe=%d" % case.probe,
            "kick=%s" % kick]


def wf_shapes(sched):
    """The wavefront pass shapes (tile, kick steps, trailing kick-less diagonal)
    of a parsed dump (tests/test_schedule_cpu.parse)."""
    return {(l["wf"][1], l["wf"][0], (l["wf"][2] >> l["wf"][0]) & 1)
            for l in sched if l["wf"][0]}


def wf_keys(dump):
    """The table-set keys of a dump."""
    return {ln.split()[2] for ln in dump.splitlines() if ln.startswith("wf_set ")}


def launch_counts(dump):
    """What one batch of a dump's schedule launches: wavefront passes, and the
    light-cone ends as DtcEngine.lightcone_counts tells them apart (the two
    10-site kernels are one form to the schedule)."""
    tally = [ln for ln in dump.splitlines() if ln.startswith("tally ")]
    assert len(tally) == 1
    t = {k: int(v) for k, v in (tok.split("=") for tok in tally[0].split()[1:])}
    return {"wf": t["wf0"] + t["wf1"], "lc8": t["lc8"], "lc10": t["lc10"], "lc12": t["lc12"]}
