"""The fleet host: sortham::FleetOptimizer (host/fleet.hpp, sortham_fleet_* of include/smpc_host.h)
ticks N sortham::Optimizer objects through one smpc_group_optimize_some call and runs the reference's
evalControl around it per member; smpc_group_optimize_some itself (SmpcGroup.optimize(take=...)).

The yardstick of every case is the "twin": a second Optimizer with the same configuration and the
same noise, driven by its own eval_control with the same inputs.  Grouped ticks equal lone ticks in
bits (test_gpu_group_wave.py) and the host code is the members' own, so a member equals its twin in
bits: Twist, control sequence, optimized trajectory, the tick's integers, min_cost and sum_w.

Members are built as test_gpu_group_wave.py builds them (tests/footprint_scenes.py: the wall scene,
the deployed critic list with consider_footprint, the 0.5 x 0.36 m rectangle) at 256 x 56 — 16
blocks of one launch — and one fleet at 192 x 64, the whole-horizon instance.  Controller frequency
20 Hz = 1 / model_dt: the control sequence is shifted after every tick.

The counters: a member that rides the batched launch and whose tick reports more than one pass was
scored again on its own (a missed furthest-point prediction), which smpc_group_stats counts as a
single tick; so a round adds to single_ticks the members that do not ride plus the riders with
passes > 1, exactly."""
import os

import numpy as np
import pytest

from mpcholonavigation_amd import _abi as A
from mpcholonavigation_amd.synthetic import make_noise, make_scenario
from mpcholonavigation_amd.tick import Tick, default_config, default_critics
from tests.footprint_scenes import (CIRCUMSCRIBED, FOOTPRINT, FREQ, INTS, LAYER_SCALING, NOT_TAKEN, THROWN, classes, dress,
                                    fleet_of, host, list_critics, moved_along, round_with_twins, same, setup, wall_case,
                                    wall_pair)
from tests.harness import DEPLOYED, FIVE, close, shifted
from tests.helpers import rel_err

pytestmark = pytest.mark.gpu


# ---- 1. closed loop, equal bits ------------------------------------------------------------------

@pytest.mark.parametrize("B,T", [(256, 56), (192, 64)])
def test_closed_loop_every_member_equals_its_twin(B, T):
    trio = [wall_pair(B, T, seed=500 + i) for i in range(3)]
    members, twins, scn = [p[0] for p in trio], [p[1] for p in trio], trio[0][2]
    fleet = fleet_of(members)
    assert all(m.get_constraints()[1] for m in members)          # shifting on
    log = []
    for k in range(8):
        res, d_single, d_batched = round_with_twins(fleet, members, twins, [moved_along(scn.tick, k)] * 3, f"{B}x{T} round {k}")
        passes = [r.out.passes for r in res]
        log.append((passes, d_single, d_batched))
        assert all(r.out.pass_kind == 0 for r in res), k
        if k == 0:
            assert (d_single, d_batched) == (3, 0)               # no prediction yet: each alone
        if k >= 2:
            # one batched launch, and a single tick only for a member whose prediction missed
            assert d_batched == 1 and d_single == sum(p > 1 for p in passes), log
    print(f"[fleet] {B}x{T} closed loop (passes, single ticks, batched launches) per round: {log}")
    assert any(d_single == 0 for _, d_single, _ in log[2:]), log
    # the footprint walk decided: some rollouts collided, not all
    assert 0 < res[0].out.non_colliding < B
    assert fleet.stats().retries == 0
    fleet.close()
    close(*members, *twins)


# ---- 2. against the oracle ---------------------------------------------------------------------------

def test_closed_loop_against_the_reference_host_logic_on_the_oracle():
    """The bar of test_gpu_host_optimizer.py's closed loops: Twist rel_err < 2e-4, fail_flag and the
    furthest point equal, the oracle's control sequence re-synchronised every round."""
    from oracle.loader import OracleOptimizer
    B, T = 256, 56
    members, oracles = [], []
    for i in range(3):
        cfg, scn, _ = wall_case(B, T)
        noise = make_noise(B, T, std=(cfg.vx_std, cfg.vy_std, cfg.wz_std), seed=500 + i)
        cr = list_critics("deployed")
        members.append(host(cfg, scn, cr, DEPLOYED, noise))
        o = OracleOptimizer(cfg, cr, FREQ)
        o.set_costmap(scn.cells, scn.origin_x, scn.origin_y, scn.resolution, inscribed_radius=scn.inscribed_radius,
                      cost_scaling_factor=scn.cost_scaling_factor, inflation_radius=scn.inflation_radius)
        xy = np.ascontiguousarray(FOOTPRINT, np.float64)
        assert o.lib.smpc_oracle_set_footprint(o.core, xy.ctypes.data, len(xy), CIRCUMSCRIBED, LAYER_SCALING) == 0
        o.set_noise(*noise)
        oracles.append(o)
    fleet = fleet_of(members)
    for k in range(8):
        tick = moved_along(scn.tick, k)
        res = fleet.eval_control([tick] * 3)
        for i, (m, o) in enumerate(zip(members, oracles)):
            tw_o, out_o = o.eval_control(tick)
            r = res[i]
            e = rel_err(r.twist, tw_o)
            print(f"[fleet oracle] round {k} member {i}: twist rel err {e:.2e}, non-colliding {r.out.non_colliding} / "
                  f"{out_o.non_colliding}")
            assert r.status == 0 and r.out.fail_flag == out_o.fail_flag == 0
            assert r.out.furthest_reached_path_point == out_o.furthest_reached_path_point
            assert e < 2e-4, (k, i, r.twist, tw_o)
            o.set_control_sequence(m.get_control_sequence())
    fleet.close()
    close(*members, *oracles)


# ---- 3. take -----------------------------------------------------------------------------------------

def test_a_member_left_out_is_untouched_and_goes_on_as_its_twin():
    trio = [wall_pair(seed=510 + i) for i in range(3)]
    members, twins, scn = [p[0] for p in trio], [p[1] for p in trio], trio[0][2]
    members[1].set_speed_limit(80.0, True)
    twins[1].set_speed_limit(80.0, True)
    fleet = fleet_of(members)
    for k in range(8):
        take = [1, 0, 1] if k in (2, 3) else [1, 1, 1]           # rounds 3 and 4 without member 1
        u, c = members[1].get_control_sequence(), members[1].get_constraints()[0]
        ticks = [moved_along(scn.tick, k)] * 3
        if not take[1]:
            ticks[1] = None                                       # not looked at
        res, _, _ = round_with_twins(fleet, members, twins, ticks, f"take round {k}", take=take)
        if not take[1]:
            assert res[1].twist is None and res[1].out is None
            assert np.array_equal(members[1].get_control_sequence(), u)
            assert np.array_equal(members[1].get_constraints()[0], c)
    # nobody taken: a no-op
    state = [m.get_control_sequence() for m in members]
    before = fleet.stats()
    res = fleet.eval_control([None] * 3, take=[0, 0, 0])
    assert [r.status for r in res] == [NOT_TAKEN] * 3
    after = fleet.stats()
    assert (after.batched_launches, after.single_ticks, after.retries) == (before.batched_launches, before.single_ticks, before.retries)
    assert all(np.array_equal(m.get_control_sequence(), s) for m, s in zip(members, state))
    round_with_twins(fleet, members, twins, [moved_along(scn.tick, 8)] * 3, "after the empty round")
    fleet.close()
    close(*members, *twins)


# ---- 4. a failing member ------------------------------------------------------------------------------

@pytest.mark.parametrize("retry", [0, 1, 3])
def test_a_member_that_cannot_plan_throws_alone(retry):
    """Member 1 stands on an all-lethal map with the five critics: every rollout collides, fallback()
    resets and retries retry_attempt_limit times alone with the fail flag sticky, then throws
    (optimizer.cpp:166-183) — that member's status; its neighbours' round is their twins'."""
    B, T = 256, 56
    pairs = [wall_pair(seed=520), None, wall_pair(seed=522)]
    cfg = default_config(batch_size=B, time_steps=T)
    bad_scn = make_scenario(T, all_lethal=True)
    noise = make_noise(B, T, seed=521)
    pairs[1] = tuple(host(cfg, bad_scn, default_critics(), FIVE, noise, footprint=False, retry_attempt_limit=retry)
                     for _ in range(2))
    members, twins, scn = [p[0] for p in pairs], [p[1] for p in pairs], pairs[0][2]
    fleet = fleet_of(members)
    for k in range(2):
        ticks = [moved_along(scn.tick, k), bad_scn.tick, moved_along(scn.tick, k)]
        res = fleet.eval_control(ticks)
        assert res[1].status == THROWN and "Optimizer fail to compute path" in res[1].error, (res[1].status, res[1].error)
        with pytest.raises(RuntimeError, match="Optimizer fail to compute path"):
            twins[1].eval_control(bad_scn.tick)
        # fallback() ended in reset(); the last tick either ran is the last retry
        assert not members[1].get_control_sequence().any() and not twins[1].get_control_sequence().any()
        lm, lt = members[1].last_tick(), twins[1].last_tick()
        for f in INTS + ("passes", "min_cost", "sum_w"):
            assert getattr(lm, f) == getattr(lt, f) == getattr(res[1].out, f), (k, f)
        assert lm.fail_flag == 1 and lm.non_colliding == 0
        assert fleet.stats().retries == (k + 1) * retry           # the counter was cleared by the throw
        for i in (0, 2):
            tw_t, out_t = twins[i].eval_control(ticks[i])
            same(members[i], twins[i], res[i], tw_t, out_t, f"retry {retry} round {k} member {i}")
    fleet.close()
    close(*members, *twins)


# ---- 5. members that do not ride -------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["ackermann", "visualize", "two_iterations"])
def test_a_member_without_a_batched_instance_is_ticked_alone_inside_the_round(kind):
    kw = {"ackermann": dict(cfg_kw={"motion_model": A.SMPC_MODEL_ACKERMANN, "vy_max": 0.0, "vy_std": 0.0},
                            motion_model="Ackermann"),
          "visualize": dict(visualize=True),
          "two_iterations": dict(cfg_kw={"iteration_count": 2})}[kind]
    trio = [wall_pair(seed=530), wall_pair(seed=531), wall_pair(seed=532, **kw)]
    members, twins, scn = [p[0] for p in trio], [p[1] for p in trio], trio[0][2]
    fleet = fleet_of(members)
    for k in range(4):
        res, d_single, d_batched = round_with_twins(fleet, members, twins, [scn.tick] * 3, f"{kind} round {k}")
        riders = [r.out.passes for r in res[:2]]
        print(f"[fleet] {kind} round {k}: passes {[r.out.passes for r in res]}, single +{d_single}, batched +{d_batched}")
        if k >= 2:
            assert d_batched == 1 and d_single == 1 + sum(p > 1 for p in riders), (k, riders, d_single, d_batched)
    fleet.close()
    close(*members, *twins)


def test_a_lane_member_next_to_two_deployed_ones():
    """2 048 x 56.  The member created with SMPC_FLAG_LANE_PER_ROLLOUT (the five critics, the open scene)
    scores on the lane pass: the deployed pair's instance is not its own, so it does not ride their
    launch; as a group's only lane member it keeps the one-member launch of the grouped lane instance
    that smpc_group_optimize has always given it, which neither counter counts (a missed prediction
    re-scores it alone: then it is a single tick).  Its twin is created with SMPC_NO_HALF_BLOCKS, as in
    test_gpu_group_wave.py: a group's lane members launch full-size blocks."""
    B, T = 2048, 56
    pairs = [wall_pair(B, T, seed=540), wall_pair(B, T, seed=541)]
    cfg = default_config(batch_size=B, time_steps=T, flags=A.SMPC_FLAG_LANE_PER_ROLLOUT)
    lane_scn = make_scenario(T, seed=60, path_points=40)
    noise = make_noise(B, T, seed=542)
    lane = host(cfg, lane_scn, default_critics(), FIVE, noise, footprint=False)
    os.environ["SMPC_NO_HALF_BLOCKS"] = "1"      # (read when a context is created)
    try:
        lane_twin = host(cfg, lane_scn, default_critics(), FIVE, noise, footprint=False)
    finally:
        del os.environ["SMPC_NO_HALF_BLOCKS"]
    members, twins, scn = [pairs[0][0], pairs[1][0], lane], [pairs[0][1], pairs[1][1], lane_twin], pairs[0][2]
    fleet = fleet_of(members)
    for k in range(4):
        ticks = [scn.tick, scn.tick, lane_scn.tick]
        res, d_single, d_batched = round_with_twins(fleet, members, twins, ticks, f"lane round {k}")
        passes = [r.out.passes for r in res]
        print(f"[fleet] lane round {k}: passes {passes}, kinds {[r.out.pass_kind for r in res]}, single +{d_single}, "
              f"batched +{d_batched}")
        if not os.environ.get("SMPC_PASS"):      # (the developer override picks the pass)
            assert [r.out.pass_kind for r in res] == [0, 0, 1]
        if k >= 2:
            assert d_batched == 1 and d_single == sum(p > 1 for p in passes), (k, passes, d_single, d_batched)
    fleet.close()
    close(*members, *twins)


# ---- 6. member calls between rounds ------------------------------------------------------------------------

def test_members_are_used_through_their_own_handles_between_rounds():
    """set_speed_limit on one member, reset() on another, initialize() again with another batch size on
    the third (a context rebuild: the fleet drops its group before the old context goes and regroups
    at the next round) — everybody stays its twin, and batched launches resume."""
    B, T = 256, 56
    trio = [wall_pair(B, T, seed=550 + i) for i in range(3)]
    members, twins, scn = [p[0] for p in trio], [p[1] for p in trio], trio[0][2]
    fleet = fleet_of(members)
    k = 0

    def rounds(n, label):
        nonlocal k
        for _ in range(n):
            out = round_with_twins(fleet, members, twins, [moved_along(scn.tick, k)] * 3, f"{label} round {k}")
            k += 1
        return out

    rounds(3, "start")
    for x in (members[0], twins[0]):
        x.set_speed_limit(50.0, True)
    res, _, _ = rounds(1, "speed limit")
    assert abs(members[0].get_constraints()[0][0] - 0.25) < 1e-3 and members[1].get_constraints()[0][0] == np.float32(0.5)
    for x in (members[1], twins[1]):
        x.reset()
    assert not members[1].get_control_sequence().any()
    rounds(1, "reset")
    B2 = 200
    cfg2 = default_config(batch_size=B2, time_steps=T)
    noise2 = make_noise(B2, T, std=(cfg2.vx_std, cfg2.vy_std, cfg2.wz_std), seed=559)
    for x in (members[2], twins[2]):
        x.initialize(cfg2, list_critics("deployed"), FREQ, critics=classes(DEPLOYED),
                     cost_scaling_factor=scn.cost_scaling_factor, inflation_radius=scn.inflation_radius)
        dress(x, scn, noise2, footprint=False)                  # (the footprint survives initialize())
    launches = fleet.stats().batched_launches                    # (summed over the fleet's groups: not lost)
    assert launches >= 2
    for _ in range(3):
        res, d_single, d_batched = rounds(1, "rebuilt")
    assert d_batched == 1 and d_single == sum(r.out.passes > 1 for r in res)
    assert fleet.stats().batched_launches > launches
    fleet.close()
    close(*members, *twins)


def test_a_member_shut_down_cannot_be_taken_and_the_others_go_on():
    trio = [wall_pair(seed=560 + i) for i in range(3)]
    members, twins, scn = [p[0] for p in trio], [p[1] for p in trio], trio[0][2]
    fleet = fleet_of(members)
    from mpcholonavigation_amd.host_optimizer import FleetError, FleetOptimizer
    with pytest.raises(FleetError) as e:                         # already in a fleet
        FleetOptimizer(members[:2])
    assert e.value.code == A.SMPC_ERR_STATE and "in a fleet already" in str(e.value)
    with pytest.raises(FleetError) as e:
        FleetOptimizer([twins[0], twins[0]])
    assert e.value.code == A.SMPC_ERR_INVALID and "listed twice" in str(e.value)
    # the group's own rule, with its message: one horizon per group
    other = wall_pair(192, 64, seed=569)
    with pytest.raises(FleetError) as e:
        FleetOptimizer([twins[0], other[0]])
    assert e.value.code == A.SMPC_ERR_INVALID and "share the device and time_steps" in str(e.value)
    # a member whose initialize() threw has no context: not initialised
    with pytest.raises(RuntimeError, match="is not one of the registered"):
        other[1].initialize(other[3], list_critics("deployed"), FREQ, critics=["ObstacleCritic"])
    with pytest.raises(FleetError) as e:
        FleetOptimizer([other[1]])
    assert e.value.code == A.SMPC_ERR_STATE and "not initialised" in str(e.value)
    FleetOptimizer([twins[0], twins[1]]).close()                 # (a refused creation left nobody in a fleet)
    close(*other[:2])
    round_with_twins(fleet, members, twins, [scn.tick] * 3, "before")
    members[1].close()                                           # destroyed while a member
    with pytest.raises(FleetError) as e:
        fleet.eval_control([scn.tick] * 3)
    assert e.value.code == A.SMPC_ERR_STATE and "member 1" in str(e.value)
    for k in range(1, 4):
        res, d_single, d_batched = round_with_twins(fleet, members, twins, [scn.tick, None, scn.tick], f"without 1, {k}",
                                                    take=[1, 0, 1])
    assert d_batched == 1
    # a member whose initialize() threw has no context until it is initialised again: it cannot be
    # taken, the fleet goes on without it, and takes it up again afterwards
    cfg = trio[2][3]
    for x in (members[2], twins[2]):
        with pytest.raises(RuntimeError, match="is not one of the registered"):
            x.initialize(cfg, list_critics("deployed"), FREQ, critics=["ObstacleCritic"])
    with pytest.raises(FleetError) as e:
        fleet.eval_control([scn.tick, None, scn.tick], take=[1, 0, 1])
    assert e.value.code == A.SMPC_ERR_STATE and "member 2" in str(e.value)
    round_with_twins(fleet, members, twins, [scn.tick, None, None], "without 1 and 2", take=[1, 0, 0])
    noise = make_noise(cfg.batch_size, cfg.time_steps, std=(cfg.vx_std, cfg.vy_std, cfg.wz_std), seed=562)
    for x in (members[2], twins[2]):
        x.initialize(cfg, list_critics("deployed"), FREQ, critics=classes(DEPLOYED),
                     cost_scaling_factor=scn.cost_scaling_factor, inflation_radius=scn.inflation_radius)
        dress(x, scn, noise, footprint=False)
    for k in range(3):
        res, d_single, d_batched = round_with_twins(fleet, members, twins, [scn.tick, None, scn.tick], f"2 is back, {k}",
                                                    take=[1, 0, 1])
    assert d_batched == 1
    fleet.close()
    close(members[0], members[2], *twins)


# ---- 7. regenerate_noises -------------------------------------------------------------------------------

def test_regenerate_noises_members_draw_their_twins_epochs():
    """Device RNG, the twin's seed: every tick is followed by the draw of the next epoch
    (smpc_redraw_noise_async on the group's stream), round by round the twin's sequence."""
    trio = [wall_pair(seed=0, supply_noise=False, regenerate_noises=True, noise_seed=70 + i) for i in range(3)]
    members, twins, scn = [p[0] for p in trio], [p[1] for p in trio], trio[0][2]
    fleet = fleet_of(members)
    costs = []
    for k in range(6):
        res, _, _ = round_with_twins(fleet, members, twins, [moved_along(scn.tick, k)] * 3, f"regenerate round {k}")
        costs.append(res[0].out.min_cost)
    assert len(set(costs)) == len(costs)                         # a new epoch every round
    fleet.close()
    close(*members, *twins)


# ---- 8. smpc_group_optimize_some directly ---------------------------------------------------------------

def test_the_subset_call_on_a_group():
    """take=None (smpc_group_optimize, now a call of the subset entry) against a full take on a second
    group: equal bits and counters.  Then a round without member 1: its costs stay, and its next tick
    equals the tick of a lone twin that was not called either."""
    from mpcholonavigation_amd import optimizer as mod
    B, T = 256, 56
    sets = [[], [], []]                                          # group A, group B, lone twins
    for i in range(3):
        cfg, scn, _ = wall_case(B, T)
        noise = make_noise(B, T, std=(cfg.vx_std, cfg.vy_std, cfg.wz_std), seed=580 + i)
        for s in sets:
            s.append(setup(mod.Smpc(cfg), scn, list_critics("deployed"), noise))
    ga, gb = mod.SmpcGroup(sets[0]), mod.SmpcGroup(sets[1])
    us = [scn.u0] * 3
    for k in range(6):
        ticks = [moved_along(scn.tick, k)] * 3
        skip = k == 3
        take = [1, 0, 1] if skip else [1, 1, 1]
        costs = sets[1][1].get_costs()
        ra = ga.optimize(ticks, us) if not skip else ga.optimize(ticks, us, take=take)
        rb = gb.optimize([t if on else None for t, on in zip(ticks, take)], [u if on else None for u, on in zip(us, take)],
                         take=take)
        new_us = list(us)
        for i in range(3):
            if not take[i]:
                assert ra[i] is None and rb[i] is None
                assert np.array_equal(sets[1][1].get_costs(), costs)
                continue
            ut, ot = sets[2][i].optimize(ticks[i], us[i])
            for (u, o), label in ((ra[i], "take=None"), (rb[i], "take")):
                assert np.array_equal(u, ut), (k, i, label)
                for f in INTS + ("min_cost", "sum_w"):
                    assert getattr(o, f) == getattr(ot, f), (k, i, label, f)
            assert ra[i][1].passes == rb[i][1].passes
            assert np.array_equal(sets[0][i].get_costs(), sets[2][i].get_costs()), (k, i)
            assert np.array_equal(sets[1][i].get_costs(), sets[2][i].get_costs()), (k, i)
            new_us[i] = shifted(ut)
        us = new_us
        sa, sb = ga.stats(), gb.stats()
        assert (sa.batched_launches, sa.single_ticks) == (sb.batched_launches, sb.single_ticks), k
    assert sa.batched_launches >= 3
    # nobody taken: nothing happens, null pointers allowed
    assert gb.optimize([None] * 3, [None] * 3, take=[0, 0, 0]) == [None] * 3
    sc = gb.stats()
    assert (sc.batched_launches, sc.single_ticks) == (sb.batched_launches, sb.single_ticks)
    ga.close()
    gb.close()
    close(*sets[0], *sets[1], *sets[2])


# ---- 9. the abandoned round -----------------------------------------------------------------------------

def test_a_round_that_fails_as_a_whole_moves_nobody_and_the_next_one_is_the_twins():
    """Member 1 comes with a plan of 1 025 points (SMPC_ERR_UNSUPPORTED: the path lives in LDS): the
    round returns the error, no member's control sequence or constraints moved, and the next round,
    with a valid plan, is the round of twins that were not called in between."""
    from mpcholonavigation_amd.host_optimizer import FleetError
    trio = [wall_pair(seed=590 + i) for i in range(3)]
    members, twins, scn = [p[0] for p in trio], [p[1] for p in trio], trio[0][2]
    fleet = fleet_of(members)
    for k in range(3):
        round_with_twins(fleet, members, twins, [moved_along(scn.tick, k)] * 3, f"before round {k}")
    t = moved_along(scn.tick, 3)
    n = 1025
    px = (t.pose_x + 0.002 * np.arange(n)).astype(np.float32)
    long = Tick(t.pose_x, t.pose_y, t.pose_yaw, t.speed, px, np.full(n, t.path_y[0], np.float32), np.zeros(n, np.float32),
                float(px[-1]), float(t.path_y[0]))
    state = [(m.get_control_sequence(), m.get_constraints()[0], m.get_optimized_trajectory()) for m in members]
    stats = fleet.stats()
    with pytest.raises(FleetError) as e:
        fleet.eval_control([t, long, t])
    assert e.value.code == A.SMPC_ERR_UNSUPPORTED, str(e.value)
    print(f"[fleet] abandoned round: {e.value}")
    # lastError() names the call and the member whose context met the error, then the library's own text
    text = str(e.value).split("] ", 1)[1]
    assert text.startswith("smpc_group_optimize_some: member 1: ") and "SMPC_MAX_PATH" in text, text
    for m, (u, c, _) in zip(members, state):
        assert np.array_equal(m.get_control_sequence(), u) and np.array_equal(m.get_constraints()[0], c)
    assert fleet.stats().retries == stats.retries
    for k in range(3, 6):
        res, d_single, d_batched = round_with_twins(fleet, members, twins, [moved_along(scn.tick, k)] * 3, f"after round {k}")
    assert d_batched == 1
    fleet.close()
    close(*members, *twins)
