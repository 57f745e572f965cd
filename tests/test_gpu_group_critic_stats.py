"""Critic statistics for a fleet: smpc_group_critic_breakdown gives every member of an smpc_group what
smpc_critic_breakdown gives an identical context outside any group, the group staying a group.

The yardstick everywhere is the LONE TWIN: a second context, never grouped, created and configured
identically (config, seed or set_noise, costmap, critics, footprint, limits, tick history).  Its
breakdown is compared with np.array_equal on per_rollout and field by field on the struct: no
tolerance.  tests/test_gpu_critic_stats*.py hold the twin to the oracle and to float64.

Shapes are the smallest at which the grouped kernels can go wrong: a block of the pass is 16
rollouts, so 72, 200 and 130 end in a half block and 72 / 200 / 256 / 1000 need 5, 13, 16 and 63 blocks
of one launch (a block beyond a member's grid must leave, and nW must be the member's own); path
lengths 40 to 60 give each member its own LDS carve-up; 400, 16 390 and 32 769 rollouts are 1, 2 and 3
slices of the reduction (a block beyond a member's slices must leave)."""
import ctypes as C

import numpy as np
import pytest

from mpcholonavigation_amd import _abi as A
from mpcholonavigation_amd.synthetic import make_noise, make_scenario, wall_beside_path
from mpcholonavigation_amd.tick import Tick, default_config
from tests.footprint_scenes import (critics_of, fleet_of, list_critics, moved_along, round_with_twins, setup, wall_member,
                                    wall_pair)
from tests.harness import FIVE, OUT_FIELDS, close, copy_of, mod, moved, shifted  # noqa: F401
from tests.helpers import configure
from tests.stats_scenes import CONTROL, NO_FURTHEST, ORDER, critics, mask_of, scene

pytestmark = pytest.mark.gpu

STRUCT_FIELDS = ("scored_mask", "fail_flag", "batch", "best_rollout", "best_cost", "effective_samples")
ROW_FIELDS = ("sum", "min", "max", "weighted", "at_best")


def same_stats(a, b, label):
    """Two breakdowns: equal, not close."""
    for f in STRUCT_FIELDS:
        assert getattr(a, f) == getattr(b, f), (label, f, getattr(a, f), getattr(b, f))
    for f in ROW_FIELDS:
        assert np.array_equal(getattr(a, f), getattr(b, f)), (label, f, getattr(a, f), getattr(b, f))
    assert (a.per_rollout is None) == (b.per_rollout is None), label
    if a.per_rollout is not None:
        assert a.per_rollout.shape == b.per_rollout.shape and np.array_equal(a.per_rollout, b.per_rollout), label


def against_twins(grp, twins, ticks, us, label, take=None):
    """One grouped breakdown against the twins' single calls, member by member.  -> the group's results"""
    res = grp.critic_stats(ticks, us, take=take, per_rollout=True)
    for i, tw in enumerate(twins):
        if take is not None and not take[i]:
            assert res[i] is None
            continue
        try:
            ref = tw.critic_stats(ticks[i], us[i], per_rollout=True)
        except Exception as e:      # the twin refuses: the member's entry is the same refusal
            assert isinstance(res[i], type(e)) and res[i].code == e.code and str(res[i]) == str(e), (label, i, res[i], e)
            continue
        assert not isinstance(res[i], Exception), (label, i, res[i])
        same_stats(res[i], ref, f"{label} member {i}")
    return res


def pair(mod, B, T, cr, seed, P=60, origin=(0.0, 0.0), temperature=0.3, gamma=0.015, footprint=False, near_goal=False,
         cfg_kw=None, limits=None):
    """(member, twin, tick, u0): two contexts with the same everything on the wall scene at `origin`."""
    cfg = default_config(batch_size=B, time_steps=T, temperature=temperature, gamma=gamma)
    cfg = copy_of(cfg, **(cfg_kw or {}))
    scn = make_scenario(T, seed=seed, path_points=P, near_goal=near_goal)
    scn.cells = wall_beside_path(scn)
    ox, oy = origin
    scn.origin_x, scn.origin_y = ox, oy
    t = scn.tick
    tick = Tick(ox + t.pose_x, oy + t.pose_y, 0.0 if near_goal else 0.2, t.speed,
                (ox + t.path_x.astype(np.float64)).astype(np.float32), (oy + t.path_y.astype(np.float64)).astype(np.float32),
                t.path_yaw, float(np.float32(ox + t.goal_x)), float(np.float32(oy + t.goal_y)), goal_checker_xy_tolerance=0.25)
    noise = make_noise(B, T, std=(cfg.vx_std, cfg.vy_std, cfg.wz_std), seed=900 + seed)
    out = []
    for _ in range(2):
        g = setup(mod.Smpc(cfg), scn, cr, noise, footprint)
        if limits:
            g.set_acceleration_limits(*limits)
        out.append(g)
    return out[0], out[1], tick, scn.u0


def grouped(mod, pairs):
    members, twins, ticks, us = (list(x) for x in zip(*pairs))
    return mod.SmpcGroup(members), members, twins, ticks, us


# ---- 1. heterogeneous members, the ragged instance ----------------------------------------------------

def test_heterogeneous_members_equal_their_twins(mod):
    """T = 56.  The deployed nine as written (CostCritic's footprint) on two members, the five with
    ObstaclesCritic on two, one member near the goal, one with all twelve critics at cost_power 2; batch
    sizes, path lengths, map origins, temperatures, gammas and noise all their own."""
    T = 56
    pairs = [
        pair(mod, 72, T, list_critics("deployed"), 60, 40, (0.0, 0.0), 0.3, 0.015, footprint=True),
        pair(mod, 200, T, critics_of(FIVE), 61, 47, (-3.7, 5.5), 0.1, 0.03),
        pair(mod, 256, T, list_critics("deployed"), 62, 53, (12.25, -1.05), 1.0, 0.0, footprint=True),
        pair(mod, 1000, T, critics_of(FIVE), 63, 60, (1.6, 0.4), 0.3, 0.1),
        pair(mod, 136, T, list_critics("deployed", False), 64, near_goal=True),
        pair(mod, 200, T, critics(ORDER, 2), 65, 50, (2.0, -2.0), 0.5, 0.02),
    ]
    grp, members, twins, ticks, us = grouped(mod, pairs)
    res = against_twins(grp, twins, ticks, us, "heterogeneous")
    bit = {n: 1 << k for k, n in enumerate(ORDER)}
    # (the deployed list's PathAlign stands down here: 56 steps do not reach its offset_from_furthest of 20 points)
    assert res[0].scored_mask & bit["cost"] and res[0].scored_mask & bit["path_follow"] and not res[0].fail_flag
    assert res[1].scored_mask & bit["obstacles"] and not res[1].scored_mask & bit["cost"]
    assert res[4].scored_mask & bit["goal_angle"] and not res[4].scored_mask & bit["path_align"]
    assert res[5].scored_mask & bit["velocity_deadband"] and res[5].scored_mask & bit["path_align_legacy"]
    assert res[5].scored_mask & bit["path_align"] and res[5].per_rollout[ORDER.index("path_align")].any()
    # the footprint and the wall decide: some rollouts collide on the members beside it, not all
    assert all(r.per_rollout.any(axis=1).sum() >= 3 for r in res)
    cnt = grp.breakdown_counts()
    print(f"[group critic stats] heterogeneous: masks {[hex(r.scored_mask) for r in res]}, effective samples "
          f"{[round(r.effective_samples, 2) for r in res]}, counts {cnt}")
    assert (cnt.batched_members, cnt.single_members) == (6, 0)
    st = grp.stats()
    assert (st.batched_launches, st.single_ticks) == (0, 0)
    grp.close()
    close(*members, *twins)


# ---- 2. the whole-horizon instance; a lane-flag member on device noise ---------------------------------

def test_whole_horizon_with_a_lane_member_on_device_noise(mod):
    """T = 64, members 192 and 130 x 64.  The 192 member is a SMPC_FLAG_LANE_PER_ROLLOUT context that
    drew with the device RNG and is asked before any tick: the draw filled the group-major tensors only,
    so the [B, T] copy the stats pass reads is made inside the grouped call (ensure_row_major)."""
    T = 64
    cfg, scn, _ = scene(4, T, "wall")
    cfg_l = copy_of(cfg, batch_size=192, flags=cfg.flags | A.SMPC_FLAG_LANE_PER_ROLLOUT)
    lane = []
    for _ in range(2):
        g = mod.Smpc(cfg_l)
        configure(g, scn, critics=critics(FIVE, 1))
        g.seed(7)
        lane.append(g)
    grp, members, twins, ticks, us = grouped(mod, [(lane[0], lane[1], scn.tick, scn.u0),
                                                   pair(mod, 130, T, list_critics("deployed"), 70, 45, footprint=True)])
    res = against_twins(grp, twins, ticks, us, "whole horizon")
    assert res[0].per_rollout[ORDER.index("obstacles")].any() and res[0].per_rollout[CONTROL].any()
    cnt = grp.breakdown_counts()
    assert (cnt.batched_members, cnt.single_members) == (2, 0)
    # the lane member's tick afterwards is its twin's: the breakdown left it alone
    rg = grp.optimize(ticks, us)
    rt = twins[0].optimize(ticks[0], us[0])
    assert np.array_equal(rg[0][0], rt[0]) and rg[0][1].pass_kind == rt[1].pass_kind == 1
    grp.close()
    close(*members, *twins)


# ---- 3. across the slices of the reduction ---------------------------------------------------------------

def test_members_of_one_two_and_three_slices(mod):
    """T = 15, batches 400, 16 390 and 32 769: 1, 2 and 3 slices in one reduction launch of three slices
    per member — the blocks beyond a member's slices must leave.  The best rollout of the 32 769 member is
    steered into its last slice (alone there: the ragged slice of one rollout), as
    test_gpu_critic_stats_reach.py::test_best_rollout_steered_across_the_slices does."""
    T = 15
    cfg, scn, _ = scene(4, T, "wall")
    pairs = []
    for B, seed in ((400, 3), (16390, 5), (32769, 7)):
        two = []
        for _ in range(2):
            g = mod.Smpc(copy_of(cfg, batch_size=B))
            configure(g, scn, critics=critics(ORDER, 1))
            g.seed(seed)
            two.append(g)
        if B == 32769:
            st0 = two[1].critic_stats(scn.tick, scn.u0)
            b = st0.best_rollout
            assert b != B - 1
            swapped = [n.copy() for n in two[1].get_noise()]
            for n in swapped:
                n[[b, B - 1]] = n[[B - 1, b]]
            for g in two:
                g.set_noise(*swapped)
        pairs.append((two[0], two[1], scn.tick, scn.u0))
    grp, members, twins, ticks, us = grouped(mod, pairs)
    res = against_twins(grp, twins, ticks, us, "slices")
    assert res[2].best_rollout == 32768 and res[2].best_cost == st0.best_cost
    assert np.array_equal(res[2].at_best, res[2].per_rollout[:, 32768])
    for r in res:
        assert np.array_equal(r.min, r.per_rollout.min(axis=1)) and np.array_equal(r.max, r.per_rollout.max(axis=1))
    assert grp.breakdown_counts().batched_members == 3
    grp.close()
    close(*members, *twins)


# ---- 4. routes ---------------------------------------------------------------------------------------------

def test_routes_in_one_group(mod):
    """One group at T = 56 whose members each take another route of the single call: closed in (every
    rollout collides: fail_flag 1, the rows of the re-score), fail_flag_in (the control row only), both
    collision critics with a footprint (refused with the single call's code and message, the others
    unaffected), acceleration limits, DiffDrive, a critic list that needs no furthest point."""
    T = 56
    closed = wall_member(mod, 200, T, "deployed", True, closed_in=True)
    t = closed[2].tick
    retry = pair(mod, 72, T, list_critics("deployed"), 80, footprint=True)
    retry_tick = Tick(*(getattr(retry[2], f) for f in ("pose_x", "pose_y", "pose_yaw", "speed", "path_x", "path_y", "path_yaw",
                                                        "goal_x", "goal_y")), fail_flag_in=True)
    both = critics_of(ORDER, footprint=("cost", "obstacles"))
    diff_kw = dict(motion_model=A.SMPC_MODEL_DIFF_DRIVE, vy_max=0.0, vy_std=0.0)
    pairs = [
        (closed[0], closed[1], t, closed[2].u0),
        (retry[0], retry[1], retry_tick, retry[3]),
        pair(mod, 136, T, both, 81, footprint=True),
        pair(mod, 200, T, list_critics("deployed"), 82, 47, footprint=True, limits=(0.6, -0.8, 0.5, 1.2)),
        pair(mod, 256, T, critics_of(FIVE), 83, 53, cfg_kw=diff_kw),
        pair(mod, 72, T, critics_of(NO_FURTHEST), 84),
    ]
    grp, members, twins, ticks, us = grouped(mod, pairs)
    res = against_twins(grp, twins, ticks, us, "routes")
    assert res[0].fail_flag and res[0].scored_mask == mask_of(("constraint", "cost"))
    assert res[1].fail_flag and res[1].scored_mask == 1 << CONTROL and not res[1].per_rollout[:CONTROL].any()
    assert isinstance(res[2], mod.SmpcError) and res[2].code == A.SMPC_ERR_UNSUPPORTED and "consider_footprint" in str(res[2])
    assert not res[3].fail_flag and not res[4].fail_flag
    assert not res[5].scored_mask & sum(1 << ORDER.index(n) for n in ("path_align", "path_follow", "path_angle"))
    # limits decide something: the limited member's rows are not those of the same member without limits
    free = pair(mod, 200, T, list_critics("deployed"), 82, 47, footprint=True)
    st_free = free[1].critic_stats(free[2], free[3], per_rollout=True)
    assert not np.array_equal(st_free.per_rollout, res[3].per_rollout)
    close(free[0], free[1])
    cnt = grp.breakdown_counts()
    assert (cnt.batched_members, cnt.single_members) == (5, 0), cnt      # (the refused member rode nothing)
    # twice: the same bits, and still the twins'
    again = against_twins(grp, twins, ticks, us, "routes, again")
    for a, b in zip(res, again):
        if not isinstance(a, Exception):
            same_stats(a, b, "routes twice")
    grp.close()
    close(*members, *twins)


def test_a_member_that_is_not_taken_is_not_touched(mod):
    """take = (1, 0, 1) through the C-ABI itself: the entries of the member left out keep the sentinel
    they were filled with, its tick input and control sequence are not read (null pointers), and its
    next tick is its twin's."""
    T = 56
    pairs = [pair(mod, 72, T, list_critics("deployed"), 90, 41, footprint=True),
             pair(mod, 200, T, critics_of(FIVE), 91, 50),
             pair(mod, 136, T, list_critics("deployed"), 92, 59, footprint=True)]
    grp, members, twins, ticks, us = grouped(mod, pairs)
    n = 3
    lib = grp.lib
    ins = (A.SmpcTickIn * n)()
    ubuf = [np.ascontiguousarray(u, np.float32) for u in us]
    for i in (0, 2):
        ins[i] = ticks[i].c
    uptr = (C.c_void_p * n)(ubuf[0].ctypes.data, None, ubuf[2].ctypes.data)
    st = (A.SmpcCriticStats * n)()
    C.memset(st, 0xAB, C.sizeof(st))
    status = (C.c_int32 * n)(-77, -77, -77)
    rows = [np.full((A.SMPC_STATS_ROWS, m.B), -5.0, np.float32) for m in members]
    rptr = (C.c_void_p * n)(*[r.ctypes.data for r in rows])
    take = (C.c_uint8 * n)(1, 0, 1)
    rc = lib.smpc_group_critic_breakdown(grp.h, ins, uptr, take, st, rptr, status)
    assert rc == 0 and list(status) == [0, -77, 0]
    assert bytes(st[1]) == b"\xab" * C.sizeof(A.SmpcCriticStats) and np.all(rows[1] == -5.0)
    for i in (0, 2):
        ref = twins[i].critic_stats(ticks[i], us[i], per_rollout=True)
        assert np.array_equal(rows[i], ref.per_rollout) and st[i].best_rollout == ref.best_rollout
        assert st[i].scored_mask == ref.scored_mask and st[i].best_cost == np.float32(ref.best_cost)
    assert not lib.smpc_last_error(members[1].h)
    cnt = grp.breakdown_counts()
    assert (cnt.batched_members, cnt.single_members) == (2, 0)
    # the wrapper's face of the same, then a round: every member's tick is its twin's
    against_twins(grp, twins, ticks, us, "take", take=(False, True, True))
    res = grp.optimize(ticks, us)
    for i in range(n):
        ut, ot = twins[i].optimize(ticks[i], us[i])
        assert np.array_equal(res[i][0], ut) and res[i][1].min_cost == ot.min_cost, i
    # nobody taken, null arrays: refused
    none = (C.c_uint8 * n)(0, 0, 0)
    assert lib.smpc_group_critic_breakdown(grp.h, ins, uptr, none, st, rptr, status) == A.SMPC_ERR_INVALID
    assert lib.smpc_group_critic_breakdown(grp.h, ins, uptr, take, st, None, None) == A.SMPC_ERR_INVALID
    grp.close()
    close(*members, *twins)


def test_a_long_horizon_pair_is_scored_one_by_one(mod):
    """T = 100: no grouped instance (as smpc_pass_many) — inside the same call, one by one, equal to the
    twins, counted under single_members."""
    T = 100
    pairs = [pair(mod, 72, T, list_critics("deployed"), 95, 44, footprint=True), pair(mod, 130, T, critics(ORDER, 1), 96, 57)]
    grp, members, twins, ticks, us = grouped(mod, pairs)
    against_twins(grp, twins, ticks, us, "T = 100")
    cnt = grp.breakdown_counts()
    assert (cnt.batched_members, cnt.single_members) == (0, 2)
    res = grp.optimize(ticks, us)
    for i in range(2):
        ut, _ = twins[i].optimize(ticks[i], us[i])
        assert np.array_equal(res[i][0], ut), i
    grp.close()
    close(*members, *twins)


# ---- 5. no side effect ---------------------------------------------------------------------------------------

def fleet_loop(mod, with_breakdown, rounds=6):
    T = 56
    pairs = [pair(mod, 72, T, list_critics("deployed"), 60, 40, (0.0, 0.0), 0.3, 0.015, footprint=True),
             pair(mod, 200, T, critics_of(FIVE), 61, 47, (-3.7, 5.5), 0.1, 0.03),
             pair(mod, 256, T, list_critics("deployed"), 62, 53, (12.25, -1.05), 1.0, 0.0, footprint=True,
                  limits=(0.6, -0.8, 0.5, 1.2))]
    grp, members, twins, ticks0, us = grouped(mod, pairs)
    close(*twins)
    log, stats = [], []
    for k in range(rounds):
        ticks = [moved(t, 0.015 * k) for t in ticks0]
        if with_breakdown:
            a = grp.critic_stats(ticks, us, per_rollout=True)
            b = grp.critic_stats(ticks, us, per_rollout=True)
            for i, (x, y) in enumerate(zip(a, b)):
                same_stats(x, y, f"round {k} member {i}: two consecutive breakdowns")
            stats.append(a)
        res = grp.optimize(ticks, us)
        s = grp.stats()
        log.append(([u.copy() for u, _ in res], [tuple(getattr(o, f) for f in OUT_FIELDS) for _, o in res],
                    [m.get_costs() for m in members], (s.batched_launches, s.single_ticks)))
        us = [shifted(u) for u, _ in res]
    grp.close()
    close(*members)
    return log, stats


@pytest.mark.parametrize("no_bar", [False, True], ids=["bar", "SMPC_NO_BAR_TICK"])
def test_breakdowns_leave_the_rounds_as_they_are(mod, monkeypatch, no_bar):
    """Six rounds with the pose advancing and u shifted, plain and with a grouped breakdown (two, in
    fact) in front of every round: u, every non-timing field of smpc_tick_out, the costs and
    smpc_group_stats bit for bit.  Both ways of handing the tick blocks over."""
    if no_bar:
        monkeypatch.setenv("SMPC_NO_BAR_TICK", "1")
    plain, _ = fleet_loop(mod, False)
    probed, stats = fleet_loop(mod, True)
    assert any(p == 1 for r in plain[1:] for p in (o[OUT_FIELDS.index("passes")] for o in r[1])), "no round speculated"
    assert plain[-1][3][0] > 0, "no round rode a batched launch"
    for k, (a, b) in enumerate(zip(plain, probed)):
        for i in range(3):
            assert np.array_equal(a[0][i], b[0][i]), f"round {k} member {i}: u"
            assert a[1][i] == b[1][i], f"round {k} member {i}: {dict(zip(OUT_FIELDS, a[1][i]))} != {dict(zip(OUT_FIELDS, b[1][i]))}"
            assert np.array_equal(a[2][i], b[2][i]), f"round {k} member {i}: costs"
        assert a[3] == b[3], f"round {k}: smpc_group_stats {a[3]} != {b[3]}"
    # the breakdowns followed the loop: they are not one answer six times
    assert not np.array_equal(stats[0][0].per_rollout, stats[-1][0].per_rollout)


def test_a_breakdown_after_an_abandoned_round_is_clean(mod):
    """A round abandoned on a refused plan (1 025 points on one member), then a breakdown: the twins'
    bits.  The same plan in the breakdown itself: that member's entry is the single call's refusal, the
    others have their statistics."""
    T = 56
    pairs = [pair(mod, 72, T, list_critics("deployed"), 60, 40, footprint=True), pair(mod, 200, T, critics_of(FIVE), 61, 47),
             pair(mod, 136, T, list_critics("deployed"), 62, 53, footprint=True)]
    grp, members, twins, ticks, us = grouped(mod, pairs)
    for _ in range(3):      # into the steady state: the rounds ride batched launches
        res = grp.optimize(ticks, us)
        for i in range(3):
            twins[i].optimize(ticks[i], us[i])
    t = ticks[2]
    n = 1025
    long_plan = Tick(t.pose_x, t.pose_y, t.pose_yaw, t.speed, (t.pose_x + 0.01 * np.arange(n)).astype(np.float32),
                     np.full(n, t.pose_y, np.float32), np.zeros(n, np.float32), t.goal_x, t.goal_y)
    with pytest.raises(mod.SmpcError):
        grp.optimize([ticks[0], ticks[1], long_plan], us)
    against_twins(grp, twins, ticks, us, "after an abandoned round")
    res = against_twins(grp, twins, [ticks[0], ticks[1], long_plan], us, "a refused plan in the breakdown")
    assert isinstance(res[2], mod.SmpcError) and not isinstance(res[0], Exception) and not isinstance(res[1], Exception)
    grp.close()
    close(*members, *twins)


# ---- 6. the host face --------------------------------------------------------------------------------------

def test_fleet_host_statistics_equal_the_twins_and_leave_the_loop_alone():
    """FleetOptimizer.critic_stats against Optimizer.critic_stats of ungrouped twin optimizers, in front
    of every round of a ten-tick closed loop: the statistics are the twins' bit for bit, and the Twists
    of the fleet's rounds are those of a second set of twins that were never asked — the breakdowns
    moved nothing.  One member is left out of the statistics on odd ticks."""
    trio = [wall_pair(256 if i else 72, 56, seed=500 + i) for i in range(3)]
    members, twins, scn = [p[0] for p in trio], [p[1] for p in trio], trio[0][2]
    fleet = fleet_of(members)
    for k in range(10):
        ticks = [moved_along(scn.tick, k)] * 3
        take = None if k % 2 == 0 else (True, False, True)
        res = fleet.critic_stats(ticks, take=take, per_rollout=(k < 2))
        for i in range(3):
            if take is not None and not take[i]:
                assert res[i] is None
                continue
            # (the twin's own breakdown leaves its loop alone: test_gpu_critic_stats.py holds that)
            same_stats(res[i], twins[i].critic_stats(ticks[i], per_rollout=(k < 2)), f"host tick {k} member {i}")
            assert res[i].scored("CostCritic") and res[i].scored("ControlCost") and res[i].batch == (256 if i else 72)
        round_with_twins(fleet, members, twins, ticks, f"host round {k}")
    # ungrouped in between (a round of the members' own eval_control leaves the fleet so): the call regroups
    fleet.run_rounds([moved_along(scn.tick, 10)] * 3, 1, alone=True)
    for t in twins:
        t.eval_control(moved_along(scn.tick, 10))
    res = fleet.critic_stats([moved_along(scn.tick, 11)] * 3)
    for i in range(3):
        same_stats(res[i], twins[i].critic_stats(moved_along(scn.tick, 11)), f"host after ungroup member {i}")
    round_with_twins(fleet, members, twins, [moved_along(scn.tick, 11)] * 3, "host round after ungroup")
    # a member that was shut down: SMPC_ERR_STATE in its entry, the others have theirs
    members[1].close()
    res = fleet.critic_stats([moved_along(scn.tick, 12)] * 3)
    assert isinstance(res[1], Exception) and res[1].code == A.SMPC_ERR_STATE
    for i in (0, 2):
        same_stats(res[i], twins[i].critic_stats(moved_along(scn.tick, 12)), f"host with a member gone, member {i}")
    fleet.close()
    close(members[0], members[2], *twins)


def test_a_member_on_several_trips_of_a_grid_smaller_than_the_launch(mod, monkeypatch):
    """Where nW is used: a wave's next rollout is nW further on, so with one rollout per wave — every
    shape above — it is never added.  Here member 0 is made under SMPC_MAX_BLOCKS_PER_CU=1 (read when a
    context is created; its twin likewise): 9 000 rollouts on a grid of one block per CU, several trips,
    beside a member of 20 000 on as many blocks per CU as its instance holds.  Where that is more than
    one, the launch is wider than member 0's own grid and only the member's own nW scores it right;
    where it is one (the R = 1 instances on gfx950 today), both grids are the cap and the
    case holds the several trips of two members in one launch to their twins."""
    T = 15
    cfg, scn, _ = scene(4, T, "wall")
    pairs = []
    for B, seed, knob in ((9000, 11, "1"), (20000, 12, None)):
        if knob:
            monkeypatch.setenv("SMPC_MAX_BLOCKS_PER_CU", knob)
        else:
            monkeypatch.delenv("SMPC_MAX_BLOCKS_PER_CU", raising=False)
        two = []
        for _ in range(2):
            g = mod.Smpc(copy_of(cfg, batch_size=B))
            configure(g, scn, critics=critics(ORDER, 1))
            g.seed(seed)
            two.append(g)
        pairs.append((two[0], two[1], scn.tick, scn.u0))
    grp, members, twins, ticks, us = grouped(mod, pairs)
    res = against_twins(grp, twins, ticks, us, "several trips")
    assert all(r.per_rollout[CONTROL].all() for r in res)        # every rollout was scored
    assert grp.breakdown_counts().batched_members == 2
    grp.close()
    close(*members, *twins)
