"""Trajectory validation in the host optimizer and the fleet (Optimizer::setTrajectoryValidation,
FleetOptimizer's one grouped validation per round).

The scenes are the fleet host's (tests/footprint_scenes.py: the wall scene, the deployed critic
list).  A result is made to collide without changing the tick: a moving obstacle with collision_cost
and repulsion_weight 0 scores nothing — the twin without it ticks to the same bits — and with a
radius that covers the robot the mean's first pose is inside it whatever the controls are."""
import numpy as np
import pytest

from mpcholonavigation_amd import _abi as A
from tests.footprint_scenes import THROWN, fleet_of, moved_along, wall_pair
from tests.harness import close

pytestmark = pytest.mark.gpu

MESSAGE = "Optimizer fail to compute path"       # ref src/optimizer.cpp:166-183


def covering_disc(scn, T, far=False):
    xy = np.zeros((1, T, 2), np.float32)
    xy[0, :, 0] = scn.tick.pose_x + (30.0 if far else 0.0)
    xy[0, :, 1] = scn.tick.pose_y
    return xy, np.array([0.5], np.float32)


def free_disc(h, scn, far=False):
    h.set_moving_obstacles(*covering_disc(scn, h.T, far), collision_cost=0.0, repulsion_weight=0.0)


def test_off_and_valid_equal_the_twin_bit_for_bit():
    on, twin, scn, _ = wall_pair(seed=700)
    off, _, _, _ = wall_pair(seed=700)
    for h in (on, off, twin):
        free_disc(h, scn, far=True)
    on.set_trajectory_validation(True, consider_footprint=True)
    off.set_trajectory_validation(True)
    off.set_trajectory_validation(False)
    assert off.last_validation().run == 0 and off.last_validation().valid
    for k in range(4):
        tick = moved_along(scn.tick, k)
        (ta, oa), (tb, ob), (tc, oc) = on.eval_control(tick), off.eval_control(tick), twin.eval_control(tick)
        assert np.array_equal(ta, tc) and np.array_equal(tb, tc), k
        assert np.array_equal(on.get_control_sequence(), twin.get_control_sequence()), k
        assert np.array_equal(off.get_control_sequence(), twin.get_control_sequence()), k
        assert (oa.non_colliding, oa.min_cost, oa.sum_w) == (oc.non_colliding, oc.min_cost, oc.sum_w), k
    v = on.last_validation()
    assert v.valid and v.checked == 40 and (v.run, v.invalid) == (4, 0)
    assert off.last_validation().run == 0
    close(on, off, twin)


@pytest.mark.parametrize("limit", [0, 2])
def test_an_invalid_result_resets_retries_and_throws_the_references_message(limit):
    h, twin, scn, _ = wall_pair(seed=701, retry_attempt_limit=limit)
    for o in (h, twin):
        free_disc(o, scn)
    h.set_trajectory_validation(True, collision_lookahead_time=1.0)
    tw, out = twin.eval_control(scn.tick)          # the tick itself is fine: nothing collides with the costmap
    assert out.fail_flag == 0
    with pytest.raises(RuntimeError) as e:
        h.eval_control(scn.tick)
    assert MESSAGE in str(e.value)
    v = h.last_validation()
    assert not v.valid and (v.cause, v.first_bad, v.disc, v.checked) == (A.SMPC_VALIDATION_CAUSE_DISC, 0, 0, 20)
    assert (v.run, v.invalid) == (limit + 1, limit + 1)      # the first result and every retry's
    assert h.last_tick().fail_flag == 0                      # no tick failed: the validator refused them
    assert not np.any(h.get_control_sequence())              # the last reset's
    # validation off again: the object goes on like a fresh twin after the same reset
    h.set_trajectory_validation(False)
    twin.reset()
    assert np.array_equal(h.eval_control(scn.tick)[0], twin.eval_control(scn.tick)[0])
    close(h, twin)


def test_setting_is_refused_and_kept_across_reset():
    h, twin, scn, _ = wall_pair(seed=702, retry_attempt_limit=0)
    for bad in (0.0, -2.0, float("nan"), float("inf")):
        with pytest.raises(RuntimeError):
            h.set_trajectory_validation(True, collision_lookahead_time=bad)
    h.eval_control(scn.tick)
    assert h.last_validation().run == 0                      # a refused setting switched nothing on
    h.set_trajectory_validation(True)
    h.reset()
    free_disc(h, scn)
    with pytest.raises(RuntimeError):
        h.eval_control(scn.tick)
    assert h.last_validation().run == 1
    close(h, twin)


def test_fleet_one_grouped_validation_per_round_and_an_invalid_member_retries_alone():
    trio = [wall_pair(seed=710 + i, retry_attempt_limit=1) for i in range(3)]
    members, twins, scn = [p[0] for p in trio], [p[1] for p in trio], trio[0][2]
    for i, (m, t) in enumerate(zip(members, twins)):
        for o in (m, t):
            free_disc(o, scn, far=i != 1)                    # member 1 stands inside its disc
    fleet = fleet_of(members)
    fleet.set_trajectory_validation(True, collision_lookahead_time=1.5)
    rounds = 3
    for k in range(rounds):
        before = fleet.validation_counts()
        retries = fleet.stats().retries
        tick = moved_along(scn.tick, k)
        res = fleet.eval_control([tick] * 3)
        after = fleet.validation_counts()
        # the round's one call for the three, and member 1's retry alone
        assert (after.launches - before.launches, after.members - before.members) == (2, 4), k
        assert fleet.stats().retries - retries == 1, k
        assert res[1].status == THROWN and MESSAGE in res[1].error, k
        for i in (0, 2):
            tw, out = twins[i].eval_control(tick)
            assert res[i].status == 0 and np.array_equal(res[i].twist, tw), (k, i)
            assert np.array_equal(members[i].get_control_sequence(), twins[i].get_control_sequence()), (k, i)
            assert (res[i].out.non_colliding, res[i].out.min_cost) == (out.non_colliding, out.min_cost), (k, i)
    v = fleet.last_validation()
    assert (v[0].run, v[0].invalid) == (rounds, 0) and (v[2].run, v[2].invalid) == (rounds, 0)
    assert (v[1].run, v[1].invalid) == (2 * rounds, 2 * rounds) and v[1].cause == A.SMPC_VALIDATION_CAUSE_DISC
    # validation off: no further call
    fleet.set_trajectory_validation(False)
    before = fleet.validation_counts()
    res = fleet.eval_control([moved_along(scn.tick, rounds)] * 3)
    assert fleet.validation_counts().launches == before.launches and res[1].status == 0
    fleet.close()
    close(*members, *twins)
