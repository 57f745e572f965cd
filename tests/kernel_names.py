"""The names of the scoring-pass instances, as smpc_debug_last_pass_kernel (and rocprofv3's kernel
trace) spells them: one speller per kernel template and one table from horizon to the lane pass's
row.  The tests pin the instance a tick must run by name; every expected name is written down here
or in the test, none is computed the way the library selects (smpc_inst.h: lane_select).

The lane pass has nine template arguments,
    smpc_pass_lane<FULL, OBST, MANY, NCH, RR, GA, QUADS, TC, DEP>
given by keyword; what is not named is the plain row of a 64-step tick (PLAIN).  lane(56) starts
from the plain row of a 56-step tick (PLAIN_ROW) instead, and the keywords change that one."""

# FULL: T == 64 * NCH (no step mask); OBST: ObstaclesCritic scored; MANY: the grouped launch;
# NCH: chunks of 64 steps; RR: the re-read form; GA: GoalAngle scored (a near-goal tick);
# QUADS: noise read in quads of steps; TC: compile-time horizon (0: run time); DEP: the deployed list
LANE_ARGS = ("full", "obst", "many", "nch", "rr", "ga", "quads", "tc", "dep")
PLAIN = dict(full=True, obst=True, many=False, nch=1, rr=False, ga=False, quads=True, tc=0, dep=False)

# horizon -> what the plain row (the five critics, a cruise tick, one context) changes of PLAIN
PLAIN_ROW = {
    64: dict(),
    56: dict(full=False, tc=56),
    40: dict(full=False),
    30: dict(full=False, quads=False),
    128: dict(nch=2, rr=True),
}
# the same without ObstaclesCritic: below 64 steps the ragged instance
NO_OBST_ROW = {
    64: dict(obst=False),
    56: dict(full=False, obst=False, quads=False),
    40: dict(full=False, obst=False, quads=False),
    30: dict(full=False, obst=False, quads=False),
}


def spell(name, args):
    return name + "<" + ", ".join(str(a).lower() if isinstance(a, bool) else str(a) for a in args) + ">"


def _lane_args(horizon, diff, table=PLAIN_ROW):
    unknown = set(diff) - set(LANE_ARGS)
    assert not unknown, f"not a template argument of the lane pass: {sorted(unknown)}"
    row = {**PLAIN, **table[horizon], **diff}
    return tuple(row[a] for a in LANE_ARGS)


def lane(horizon=64, **diff):
    return spell("smpc_pass_lane", _lane_args(horizon, diff))


def lane_pow(horizon=64, **diff):
    """The instances for a cost_power other than 1."""
    return spell("smpc_pass_lane_pow", _lane_args(horizon, diff))


def lane_nh(horizon=64, **diff):
    """The instances without a vy stream (DiffDrive, Ackermann)."""
    return spell("smpc_pass_lane_nh", _lane_args(horizon, diff))


def wave(r, mode, full, many=False):
    """smpc_pass<R, MODE, FULL>: R chunks of 64 steps, FULL: T == 64 R; many: the grouped launch."""
    return spell("smpc_pass_many" if many else "smpc_pass", (r, mode, full))


def wave_at(T, mode, many=False):
    """wave() for a horizon: R = 1, 2, 4 up to 64, 128, 256 steps."""
    r = 1 if T <= 64 else 2 if T <= 128 else 4
    return wave(r, mode, T == 64 * r, many)


def stats(r, full, many=False):
    """smpc_pass_stats<R, FULL>: the wave pass keeping every critic's term (a breakdown)."""
    return spell("smpc_pass_stats_many" if many else "smpc_pass_stats", (r, full))


# the plain rows, spelled: horizon -> kernel
LANE_ROW = {T: lane(T) for T in PLAIN_ROW}
LANE_ROW_NO_OBST = {T: spell("smpc_pass_lane", _lane_args(T, {}, NO_OBST_ROW)) for T in NO_OBST_ROW}
LANE_NH_ROW = {T: lane_nh(T) for T in (64, 56, 40)}
LANE_POW_ROW = {T: lane_pow(T) for T in (64, 56, 40, 30)}
