"""make_plan (csrc/dtc_schedule.h) against the plan table of tests/plan_table.py,
through the host-only dtc_plan_groups: the GPU parity tests pick their L by the
plan it runs (9-site and 4-site column groups, three groups, one tile), so the
planner must not move an L onto another plan unnoticed."""
import pytest

from tests.plan_table import PLAN, plan_id


def test_table_covers_every_batched_size():
    assert sorted(PLAN) == list(range(1, 26))
    for L, sizes in PLAN.items():
        assert sum(sizes) == L
        # the low group holds 9..12 sites, a column group 9, 8 or 4
        if len(sizes) > 1:
            assert 9 <= sizes[0] <= 12 and set(sizes[1:]) <= {9, 8, 4}, L


@pytest.mark.parametrize("L", sorted(PLAN), ids=plan_id)
def test_plan_groups_match_table(pkg, L):
    """dtc_plan_groups orders the column groups by increasing size (the sharded
    steps' order), the sweeps by decreasing size: the sizes as a multiset."""
    masks = pkg._capi.plan_groups(L)
    acc = 0
    for m in masks:
        assert acc & m == 0
        acc |= m
    assert acc == (1 << L) - 1
    sizes = [bin(m).count("1") for m in masks]
    assert sorted(sizes) == sorted(PLAN[L]), (L, sizes)
    # the low group is the first mask and holds the low sites
    assert masks[0] == (1 << PLAN[L][0]) - 1
