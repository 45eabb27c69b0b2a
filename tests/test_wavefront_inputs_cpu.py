"""The census behind tests/test_gpu_wavefront_inputs.py, on the CPU:
tools/schedule_check.cpp dumps the L = 20 schedule of every probe site 0 .. 19 at
T = 8 .. 12 with t_offset 0 and 1 (the default layer cap, RX kicks; RY kicks for
a few, since the kick family must not change a schedule), and the wavefront
launches of all of them give

  * the pass shapes (tile, kick steps, trailing kick-less diagonal), which pick
    the code path of dtc_wf_pass, and
  * the table-set keys (wf_table_set in csrc/dtc_schedule.h: which fields and
    bonds each step's diagonal holds), which pick the tables it reads.

The case table of tests/wavefront_cases.py must reach every one of them -- the
GPU file runs exactly those cases -- and the census size is pinned, so a planner
change that adds a shape or a key fails here until a case reaches it.  The real
xy_cycle kicks (five RX periods, five RY periods) must plan no wavefront pass at
all: every interior run of a chain long enough spans the RX | RY edge."""
import subprocess

import pytest

from tests import wavefront_cases as wc
from tests.test_schedule_cpu import WF_SHAPE, build, parse

N_SHAPES, N_KEYS = 12, 19
# RY dumps: the two cases that cover the census, a column-group probe, the default
Y_POINTS = [(4, 12, 1), (5, 11, 1), (17, 12, 1), (10, 11, 0)]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return build(tmp_path_factory.mktemp("wf_inputs"), [])


def _dump(exe, args):
    r = subprocess.run([exe, *args], capture_output=True, text=True)
    assert r.returncode == 0, (args, r.stdout[-400:], r.stderr[-400:])
    return r.stdout


def _point(exe, probe, T, t_offset, kick="x"):
    dump = _dump(exe, ["L=20", "probe=%d" % probe, "T=%d" % T, "t_offset=%d" % t_offset,
                       "kick=%s" % kick])
    return wc.wf_shapes(parse(dump)), wc.wf_keys(dump)


@pytest.fixture(scope="module")
def census(exe):
    """{(probe, T, t_offset): (shapes, keys)} of the RX dumps."""
    return {(probe, T, off): _point(exe, probe, T, off)
            for probe in wc.CENSUS_PROBES for T in wc.CENSUS_T for off in wc.CENSUS_T_OFFSETS}


def _union(census):
    shapes, keys = set(), set()
    for s, k in census.values():
        shapes |= s
        keys |= k
    return shapes, keys


def test_census_size_is_pinned(census):
    shapes, keys = _union(census)
    print("shapes:", sorted(shapes))
    for k in sorted(keys):
        print("key:", k)
    assert len(shapes) == N_SHAPES and len(keys) == N_KEYS
    # both tiles, every step count the planner gives them, the trailing diagonal on
    # tile 1 after 1, 3 and 4 kick steps
    assert {(t, s) for t, s, _ in shapes} == {(0, 1), (0, 2), (0, 3), (0, 4), (1, 2), (1, 3), (1, 4)}
    assert {s for t, s, tr in shapes if t == 0 and tr} == {1, 3, 4}
    # a first kick step without a diagonal
    assert any(k.startswith("1c||") for k in keys) and any(k.startswith("0c||") for k in keys)


def test_kick_family_does_not_change_the_schedule(exe, census):
    for point in Y_POINTS:
        assert _point(exe, *point, kick="y") == census[point], point


def test_case_table_reaches_the_census(exe, census):
    """The counterpart of test_octet_case_list_is_complete: the probe cases of the
    GPU file run every shape and every key; the two cases the table is built
    around do so alone."""
    shapes, keys = _union(census)
    got_s, got_k = set(), set()
    for c in wc.PROBE_CASES:
        assert c.kick in ("x", "y") and c.n_inst == 1 and not c.g_list
        s, k = _point(exe, c.probe, c.T, c.t_offset, c.kick)
        if (c.probe, c.T, c.t_offset) in census:
            assert (s, k) == census[(c.probe, c.T, c.t_offset)], c.name
        got_s |= s
        got_k |= k
    assert shapes - got_s == set() and keys - got_k == set()
    two_s, two_k = _union({p: census[p] for p in [(4, 12, 1), (5, 11, 1)]})
    assert two_s == shapes and two_k == keys
    points = {(c.probe, c.T, c.t_offset) for c in wc.PROBE_CASES}
    assert {(4, 12, 1), (5, 11, 1)} <= points
    # RY runs tile 1's trailing diagonal too
    assert any(t == 0 and tr for c in wc.PROBE_CASES if c.kick == "y"
               for t, _, tr in census[(c.probe, c.T, c.t_offset)][0])


def test_every_case_plans_wavefront_passes_but_the_fallback(exe):
    for c in wc.CASES:
        n = wc.launch_counts(_dump(exe, wc.sched_args(c)))["wf"]
        assert (n == 0) == (c in wc.FALLBACK_CASES), (c.name, n)


@pytest.mark.parametrize("t_offset", [0, 1])
@pytest.mark.parametrize("T", range(10, 17))
def test_xy_cycle_plans_no_wavefront_pass(exe, T, t_offset):
    """RX for five periods, RY for the next five (kicks.period_gate_specs): the
    sweep passes wavefront_applies, since every row is RX or RY, and wf_replace
    must turn down every run ("one kick family per pass").  The same sweep with
    one family plans passes from T = 11 (T = 10 with t_offset 1) on."""
    args = ["L=20", "T=%d" % T, "t_offset=%d" % t_offset]
    sched = parse(_dump(exe, args + ["kick=xy_cycle5"]))
    assert sched and not any(l["shape"] == WF_SHAPE or l["wf"][0] for l in sched)
    one = parse(_dump(exe, args + ["kick=x"]))
    assert len(one) <= len(sched)
    if T + t_offset >= 11:
        assert any(l["shape"] == WF_SHAPE for l in one) and len(one) < len(sched)


def test_xy_cycle5_rows_are_the_packages(pkg):
    """What the tool's xy_cycle5 pattern stands for (RY on the rows r with
    (r / 5) odd): kicks.period_gate_specs puts RX and RY on those rows."""
    from importlib import import_module

    kicks = import_module(pkg.__name__ + ".kicks")
    for r in range(23):
        assert kicks.period_gate_specs("xy_cycle", 0.97, r)[0][0] == ("ry" if (r // 5) % 2 else "rx")
