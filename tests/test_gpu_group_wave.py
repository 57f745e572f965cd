"""Fleet ticks on the wave pass: smpc_group_optimize batches members whose own plan chose the
wave-per-rollout pass in MODE 0, 3 or 4 (T <= 64) — the deployed critic list with consider_footprint
as the YAML is written, the same in point mode, the five critics in a context created without the
lane flag — into one launch of smpc_pass_many<1, MODE, FULL> per distinct instance.

Which instance runs (by name), every grouped member bit for bit against an identically configured
context ticked alone, parity with the CPU oracle, every kind of second pass, what does not ride, a
mixed group of lane and wave members, and the group's counters (smpc_group_stats).

Scenes, lists and footprint: tests/footprint_scenes.py.  The bar against the oracle is the one of
tests/test_gpu_footprint_lean.py: assert_parity with max_flips=3, fail_flag and non_colliding exact.
The shapes are the smallest that exercise what can go wrong: a block is 16 rollouts, so 72, 200 and
136 end in a half block, and 72 / 200 / 256 / 1000 need 5, 13, 16 and 63 blocks of one launch.

A lone context's wave-pass geometry (grid, carve-up) does not depend on whether it is grouped, so the
lone twins here are created without any knob; only the lane members of the mixed group get
SMPC_NO_HALF_BLOCKS, as the grouped lane tests do.

Not here: a stale tick block (SMPC_DEBUG_STALE_TICK, test_gpu_parity.py::
test_a_stale_tick_block_fails_the_tick_and_the_context_recovers).  The knob withholds the hand-over a
context makes by itself in prepare_tick; a grouped tick's blocks are handed over by the group, in one
pass over all riding members, which does not consult it.  The guard itself is the same code on both
routes: block 0 of a member's share of smpc_pass_many echoes the number it read, the reduction hands
it on, fetch_out compares."""
import os

import numpy as np
import pytest

from mpcholonavigation_amd import _abi as A
from mpcholonavigation_amd.synthetic import make_noise, make_scenario, wall_beside_path
from mpcholonavigation_amd.tick import Tick, default_config, default_critics
from tests.footprint_scenes import list_critics, oracle_tick, same_bits, setup, wall_case, wall_member
from tests.harness import close, last_kernel, mod, moved, shifted  # noqa: F401
from tests.helpers import assert_parity, configure
from tests.kernel_names import wave

pytestmark = pytest.mark.gpu


def row(T, mode, many=True):
    """The grouped row of a horizon of at most 64 steps (many=False: a member ticked alone)."""
    return wave(1, mode, T == 64, many)


# ---- 1. the instance, by name ----------------------------------------------------------------

@pytest.mark.parametrize("which,footprint,B,T,mode", [
    ("deployed", True, 256, 56, 4), ("deployed", True, 192, 64, 4), ("deployed", False, 256, 56, 3),
    ("five", False, 256, 64, 0), ("five", False, 256, 30, 0)])
def test_members_without_the_lane_flag_ride_the_grouped_row(mod, which, footprint, B, T, mode):
    """Three members, the same tick four times: the first has no furthest-point prediction (each member
    is ticked alone, on its own instance), from the third on the group's launch is the grouped row."""
    members = []
    for i in range(3):
        g, spare, scn = wall_member(mod, B, T, which, footprint, noise_seed=500 + i)
        spare.close()
        members.append(g)
    grp = mod.SmpcGroup(members)
    before = grp.stats()
    assert (before.batched_launches, before.single_ticks) == (0, 0)
    seen = []
    for k in range(4):
        res = grp.optimize([scn.tick] * 3, [scn.u0] * 3)
        st = grp.stats()
        seen.append((last_kernel(members[0]), [o.passes for _, o in res], st.batched_launches, st.single_ticks))
        print(f"[group wave] {which} fp {footprint} {B}x{T} tick {k}: {seen[-1]}")
        assert all(o.pass_kind == 0 for _, o in res), k
        if k == 0:
            assert seen[0][0] == row(T, mode, many=False) and st.batched_launches == 0 and st.single_ticks == 3
        if k >= 2:
            assert seen[k][0] == row(T, mode), seen
            assert seen[k][1] == [1, 1, 1], seen
            assert seen[k][2] > seen[k - 1][2] and seen[k][3] == seen[k - 1][3], seen
    grp.close()
    close(*members)


# ---- 2. bit for bit against each member alone --------------------------------------------------

def test_every_member_equals_its_lone_twin_over_a_closed_loop(mod):
    """Four members that share the horizon and the critic list (the deployed list as written) and
    nothing else: batch sizes 72, 200, 256, 1000 — 5, 13, 16 and 63 blocks of one launch, two of them
    ending in a half block — path lengths 40 to 60 (their own LDS carve-up), map origins,
    temperatures, gammas, noise.  Five ticks with the pose advancing and the control sequence shifted."""
    T = 56
    spec = [(72, 40, (0.0, 0.0), 0.3, 0.015), (200, 47, (-3.7, 5.5), 0.1, 0.03), (256, 53, (12.25, -1.05), 1.0, 0.0),
            (1000, 60, (1.6, 0.4), 0.3, 0.1)]
    members, twins, ticks0, us = [], [], [], []
    for i, (B, P, (ox, oy), temp, gamma) in enumerate(spec):
        cfg = default_config(batch_size=B, time_steps=T, temperature=temp, gamma=gamma)
        scn = make_scenario(T, seed=60 + i, path_points=P)
        scn.cells = wall_beside_path(scn)
        scn.origin_x, scn.origin_y = ox, oy
        t = scn.tick
        ticks0.append(Tick(ox + t.pose_x, oy + t.pose_y, t.pose_yaw, t.speed,
                           (ox + t.path_x.astype(np.float64)).astype(np.float32),
                           (oy + t.path_y.astype(np.float64)).astype(np.float32), t.path_yaw,
                           float(np.float32(ox + t.goal_x)), float(np.float32(oy + t.goal_y))))
        noise = make_noise(B, T, std=(cfg.vx_std, cfg.vy_std, cfg.wz_std), seed=900 + i)
        for lst in (members, twins):
            lst.append(setup(mod.Smpc(cfg), scn, list_critics("deployed"), noise))
        us.append(scn.u0)
    grp = mod.SmpcGroup(members)
    passes, left = [], []
    for k in range(5):
        ticks = [moved(t, 0.015 * k) for t in ticks0]
        res = grp.optimize(ticks, us)
        for i in range(4):
            rt = twins[i].optimize(ticks[i], us[i])
            same_bits(members[i], twins[i], res[i], rt, f"tick {k} member {i} (B {spec[i][0]})")
            assert res[i][1].pass_kind == 0
        us = [shifted(u) for u, _ in res]
        passes.append([o.passes for _, o in res])
        left.append([o.non_colliding for _, o in res])
    # the footprint walk ran and decided: every member had ticks on which some rollouts collided, not all
    for i in range(4):
        assert any(0 < row_[i] < spec[i][0] for row_ in left), (i, left)
    st = grp.stats()
    print(f"[group wave] closed loop: passes per member, per tick {passes}; batched launches {st.batched_launches}, "
          f"single ticks {st.single_ticks}")
    # after the first tick (no prediction yet) a member scores twice only where its prediction missed
    later = [p for r in passes[1:] for p in r]
    assert sum(p == 1 for p in later) >= len(later) - 4 - 2, passes      # (tick 1 has no drift estimate yet)
    assert all(p == 1 for p in passes[-1]), passes
    assert st.batched_launches >= 3
    grp.close()
    close(*members, *twins)


# ---- 3. parity with the oracle ------------------------------------------------------------------

@pytest.mark.parametrize("T,shapes", [(56, (72, 200)), (64, (136,))])
def test_grouped_members_against_the_oracle(mod, T, shapes):
    """Both lists at every shape in one group (the five critics with ObstaclesCritic's footprint run
    MODE 4 too: one launch), at T = 56 with a near-goal member of each list.  The oracle's tick is
    the scene's first (footprint_scenes.oracle_tick); the group is given it twice — alone, then
    batched — and the batched result is the one held to the oracle."""
    cases = [(which, B, False) for which in ("deployed", "five") for B in shapes]
    if T == 56:
        cases += [("deployed", 72, True), ("five", 72, True)]
    members, scns = [], []
    for which, B, near in cases:
        on = oracle_tick(which, B, T, near_goal=near)
        assert 0 < on.out.non_colliding < B, (which, B, near)
        if not near:
            off = oracle_tick(which, B, T, footprint=False)
            assert on.out.non_colliding < off.out.non_colliding, (which, B)
        cfg, scn, noise = wall_case(B, T, near_goal=near)
        members.append(setup(mod.Smpc(cfg), scn, list_critics(which), noise))
        scns.append(scn)
    grp = mod.SmpcGroup(members)
    ticks, us = [s.tick for s in scns], [s.u0 for s in scns]
    grp.optimize(ticks, us)
    before = grp.stats()
    res = grp.optimize(ticks, us)
    after = grp.stats()
    assert after.batched_launches == before.batched_launches + 1 and after.single_ticks == before.single_ticks
    assert last_kernel(members[0]) == row(T, 4)
    for (which, B, near), g, (u, out) in zip(cases, members, res):
        ref = oracle_tick(which, B, T, near_goal=near)
        label = f"grouped {which} {B}x{T}{' near goal' if near else ''}"
        assert out.passes == 1 and out.pass_kind == 0, label
        assert out.fail_flag == ref.out.fail_flag and out.non_colliding == ref.out.non_colliding, label
        assert_parity(u, out, ref.u, ref.out, g.get_costs(), ref.costs, max_flips=3, label=label)
    grp.close()
    close(*members)


# ---- 4. second passes ----------------------------------------------------------------------------

def test_a_missed_prediction_rescores_that_member_alone(mod):
    """A plan with twice the spacing halves the index of every endpoint's nearest point: member 1's
    prediction misses on the third tick.  It is scored again on its own; the others are not."""
    trio = [wall_member(mod, 256, 56, noise_seed=700 + i) for i in range(3)]
    members, twins, scn = [m for m, _, _ in trio], [t for _, t, _ in trio], trio[0][2]
    grp = mod.SmpcGroup(members)
    t = scn.tick
    px = (t.pose_x + 0.1 * np.arange(len(t.path_x))).astype(np.float32)
    jumped = Tick(t.pose_x, t.pose_y, t.pose_yaw, t.speed, px, t.path_y, t.path_yaw, float(px[-1]), t.goal_y)
    for k in range(3):
        ticks = [jumped if (k == 2 and i == 1) else t for i in range(3)]
        before = grp.stats()
        res = grp.optimize(ticks, [scn.u0] * 3)
        after = grp.stats()
        for i in range(3):
            same_bits(members[i], twins[i], res[i], twins[i].optimize(ticks[i], scn.u0), f"tick {k} member {i}")
    assert [o.passes for _, o in res] == [1, 2, 1]
    assert after.batched_launches == before.batched_launches + 1 and after.single_ticks == before.single_ticks + 1
    grp.close()
    close(*members, *twins)


def test_a_member_whose_rollouts_all_collide_and_one_that_starts_failed(mod):
    """Member 0 stands between two walls under its outline (wall_case closed_in): fail_flag 1, no
    rollout left, re-scored as alone.  Member 2 comes with fail_flag_in on the third tick: not
    eligible, ticked alone.  Member 1 and 3 ride on."""
    quad = [wall_member(mod, 256, 56, noise_seed=800 + i, closed_in=(i == 0)) for i in range(4)]
    members, twins, scns = [q[0] for q in quad], [q[1] for q in quad], [q[2] for q in quad]
    grp = mod.SmpcGroup(members)
    for k in range(3):
        ticks = [s.tick for s in scns]
        if k == 2:
            t = scns[2].tick
            ticks[2] = Tick(t.pose_x, t.pose_y, t.pose_yaw, t.speed, t.path_x, t.path_y, t.path_yaw, t.goal_x, t.goal_y,
                            fail_flag_in=True)
        before = grp.stats()
        res = grp.optimize(ticks, [s.u0 for s in scns])
        after = grp.stats()
        for i in range(4):
            same_bits(members[i], twins[i], res[i], twins[i].optimize(ticks[i], scns[i].u0), f"tick {k} member {i}")
        assert res[0][1].fail_flag == 1 and res[0][1].non_colliding == 0, k
    # the last tick: members 0, 1, 3 in the launch, 0 re-scored behind it, 2 alone
    assert after.batched_launches == before.batched_launches + 1 and after.single_ticks == before.single_ticks + 2
    assert res[2][1].fail_flag == 1 and res[1][1].passes == 1 and res[3][1].passes == 1
    grp.close()
    close(*members, *twins)


# ---- 5. what does not ride ---------------------------------------------------------------------------

def test_a_long_horizon_is_ticked_alone(mod):
    """T = 100 runs smpc_pass<2, 4, false>: no grouped row.  (Its own group: a group shares T.)"""
    pair = [wall_member(mod, 128, 100, noise_seed=300 + i) for i in range(2)]
    members, twins, scn = [p[0] for p in pair], [p[1] for p in pair], pair[0][2]
    grp = mod.SmpcGroup(members)
    for k in range(3):
        res = grp.optimize([scn.tick] * 2, [scn.u0] * 2)
        for i in range(2):
            same_bits(members[i], twins[i], res[i], twins[i].optimize(scn.tick, scn.u0), f"T 100 tick {k} member {i}")
        assert last_kernel(members[0]) == "smpc_pass<2, 4, false>"
    st = grp.stats()
    assert (st.batched_launches, st.single_ticks) == (0, 6)
    grp.close()
    close(*members, *twins)


def test_members_without_a_grouped_row_are_ticked_alone_next_to_the_launch(mod):
    """Two members as deployed ride the launch; next to them a cost_power of 2 (general pass), a
    context that stores trajectories (general pass) and an Ackermann model (its constraint launch
    behind the reduction) are ticked alone on every tick, and counted."""
    B, T = 256, 56
    power = list_critics("deployed")
    power.path_follow.cost_power = 2
    acker = {"motion_model": A.SMPC_MODEL_ACKERMANN, "vy_max": 0.0, "vy_std": 0.0}
    quint = [wall_member(mod, B, T, noise_seed=400), wall_member(mod, B, T, noise_seed=401),
             wall_member(mod, B, T, noise_seed=402, critics=power),
             wall_member(mod, B, T, noise_seed=403, cfg_kw={"flags": A.SMPC_FLAG_STORE_TRAJECTORIES}),
             wall_member(mod, B, T, noise_seed=404, cfg_kw=acker)]
    members, twins, scn = [q[0] for q in quint], [q[1] for q in quint], quint[0][2]
    us = [scn.u0.copy() for _ in range(5)]
    us[4][1] = 0.0
    grp = mod.SmpcGroup(members)
    for k in range(4):
        before = grp.stats()
        res = grp.optimize([scn.tick] * 5, us)
        after, kernel = grp.stats(), last_kernel(members[0])      # (before the twins launch theirs)
        for i in range(5):
            same_bits(members[i], twins[i], res[i], twins[i].optimize(scn.tick, us[i]), f"tick {k} member {i}")
        if k >= 2:
            assert after.single_ticks == before.single_ticks + 3 and after.batched_launches == before.batched_launches + 1
            assert res[0][1].passes == 1 and res[1][1].passes == 1
            assert kernel == row(T, 4)      # the launch goes out behind the members that are ticked alone
    grp.close()
    close(*members, *twins)


def test_lane_members_and_wave_members_in_one_group(mod):
    """Two five-critic members with the lane flag and two deployed-list members without: the lane
    pair rides its grouped lane instance as it always did, the wave pair the grouped wave row — two
    scoring launches, one reduction — and every member equals its lone twin.  (The lone lane twins
    are created with SMPC_NO_HALF_BLOCKS, as in test_gpu_properties.py: a group's lane members always
    launch full-size blocks.)"""
    T = 56
    members, twins, ticks, us = [], [], [], []
    for i in range(2):
        cfg = default_config(batch_size=2048, time_steps=T, flags=A.SMPC_FLAG_LANE_PER_ROLLOUT)
        scn = make_scenario(T, seed=60 + i, path_points=40 + 5 * i)
        noise = make_noise(2048, T, seed=900 + i)
        os.environ["SMPC_NO_HALF_BLOCKS"] = "1"      # (read when a context is created)
        try:
            twin = mod.Smpc(cfg)
        finally:
            del os.environ["SMPC_NO_HALF_BLOCKS"]
        for lst, g in ((members, mod.Smpc(cfg)), (twins, twin)):
            configure(g, scn, critics=default_critics(), noise=noise)
            lst.append(g)
        ticks.append(scn.tick)
        us.append(scn.u0)
    for i in range(2):
        m, t, scn = wall_member(mod, 200 + 56 * i, T, noise_seed=600 + i)
        members.append(m)
        twins.append(t)
        ticks.append(scn.tick)
        us.append(scn.u0)
    grp = mod.SmpcGroup(members)
    for k in range(4):
        before = grp.stats()
        res = grp.optimize(ticks, us)
        after = grp.stats()
        for i in range(4):
            same_bits(members[i], twins[i], res[i], twins[i].optimize(ticks[i], us[i]), f"mixed tick {k} member {i}")
        kinds = [o.pass_kind for _, o in res]
        if not os.environ.get("SMPC_PASS"):      # (the developer override picks the pass)
            assert kinds == [1, 1, 0, 0], kinds
    if not os.environ.get("SMPC_PASS"):
        assert [o.passes for _, o in res] == [1, 1, 1, 1]
        assert after.batched_launches == before.batched_launches + 2 and after.single_ticks == before.single_ticks
    grp.close()
    close(*members, *twins)
