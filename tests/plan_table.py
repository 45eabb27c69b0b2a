"""The site-group plan of every state size the batched engine runs (make_plan in
csrc/dtc_schedule.h): the low group's sites first, then the column groups'.

tests/test_plan_table_cpu.py pins the planner to this table; the GPU parity
files take their ids from it, so that a planner change which moves a test's L
onto another plan shows there first."""

PLAN = {L: (L,) for L in range(1, 13)}
PLAN.update({
    13: (9, 4),
    14: (10, 4),
    15: (11, 4),
    16: (12, 4),
    17: (9, 8),
    18: (10, 8),
    19: (11, 8),
    20: (12, 8),
    21: (12, 9),
    22: (10, 8, 4),
    23: (11, 8, 4),
    24: (12, 8, 4),
    25: (12, 9, 4),
})


def plan_id(L: int) -> str:
    """'L17:9+8' -- the plan as it stands in a test id."""
    return "L%d:%s" % (L, "+".join(str(a) for a in PLAN[L]))
