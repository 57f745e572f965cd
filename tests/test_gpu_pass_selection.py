"""Which scoring-pass instance a tick runs, pinned by name.

For a fixed list of tick shapes: the exact string of smpc_debug_last_pass_kernel() (the instance
as rocprofv3 spells it, every template argument written out) and smpc_tick_out.pass_kind
(0 wave per rollout, 1 lane per rollout, 2 split horizon).  The expected strings were recorded
from the library before the host code that chooses and launches the instances was gathered into
one table per kernel family and one decision; they are not derived from the code under test.

The list reaches every row of the three instance tables that a tick can reach:
  smpc_pass_lane   18 rows, all reached (plain, whole quads, TC = 56, ragged, GoalAngle, deployed
                   list, re-read with one and two chunks, and the grouped forms)
  smpc_pass_split   3 rows, all reached
  smpc_pass        24 rows, all reached (MODE 1, furthest only, through smpc_shard_furthest)
"""
import numpy as np
import pytest

from mpcholonavigation_amd.synthetic import make_noise, make_scenario
from mpcholonavigation_amd.tick import Tick, default_config
from tests.harness import (DEPLOYED, FIVE, LANE, NO_OBST, Smpc,  # noqa: F401
                           create_with_env, critics_of, last_kernel, shifted)
from tests.helpers import configure, make_case
from tests.kernel_names import lane, wave

pytestmark = pytest.mark.gpu


# (id, batch, horizon, config flags, critic names, cost_power, near the goal, environment) -> (pass_kind, kernel)
F, Tr = False, True
TICKS = [
    # lane, plain: the five critics, with and without ObstaclesCritic
    ("lane-64", 2048, 64, LANE, FIVE, 1, F, {}, 1, lane()),
    ("lane-56", 2048, 56, LANE, FIVE, 1, F, {}, 1, lane(56)),
    ("lane-40", 2048, 40, LANE, FIVE, 1, F, {}, 1, lane(full=False)),
    ("lane-30", 2048, 30, LANE, FIVE, 1, F, {}, 1, lane(full=False, quads=False)),
    ("lane-64-no-obst", 2048, 64, LANE, NO_OBST, 1, F, {}, 1, lane(obst=False)),
    ("lane-56-no-obst", 2048, 56, LANE, NO_OBST, 1, F, {}, 1, lane(full=False, obst=False, quads=False)),
    ("lane-40-no-obst", 2048, 40, LANE, NO_OBST, 1, F, {}, 1, lane(full=False, obst=False, quads=False)),
    ("lane-30-no-obst", 2048, 30, LANE, NO_OBST, 1, F, {}, 1, lane(full=False, obst=False, quads=False)),
    ("lane-64-by-size", 61440, 64, 0, FIVE, 1, F, {}, 1, lane()),
    # lane, GoalAngle: a near-goal tick
    ("lane-ga-64", 2048, 64, LANE, FIVE, 1, Tr, {}, 1, lane(ga=True)),
    ("lane-ga-40", 2048, 40, LANE, FIVE, 1, Tr, {}, 1, lane(full=False, ga=True, quads=False)),
    # lane, deployed list: a cruise tick
    ("lane-dep-64", 2048, 64, LANE, DEPLOYED, 1, F, {}, 1, lane(dep=True)),
    ("lane-dep-56", 2048, 56, LANE, DEPLOYED, 1, F, {}, 1, lane(56, dep=True)),
    # lane, re-read
    ("lane-rr-128", 2048, 128, LANE, FIVE, 1, F, {}, 1, lane(128)),
    ("lane-rr-64", 2048, 64, LANE, FIVE, 1, F, {"SMPC_LANE_REREAD": "1"}, 1, lane(rr=True)),
    # split
    ("split-4-full", 16384, 64, 0, FIVE, 1, F, {}, 2, "smpc_pass_split<4, true>"),
    ("split-4-masked", 20000, 60, 0, FIVE, 1, F, {}, 2, "smpc_pass_split<4, false>"),
    ("split-2-full", 4096, 64, 0, FIVE, 1, F, {"SMPC_PASS": "split", "SMPC_SPLIT_NSEG": "2"}, 2, "smpc_pass_split<2, true>"),
    # wave: MODE 0 (the five, cost_power 1), 2 (general), 3 (lean with the deployed list's additive forms)
    ("wave-0-30", 1000, 30, 0, FIVE, 1, F, {}, 0, wave(1, 0, F)),
    ("wave-0-64", 1000, 64, 0, FIVE, 1, F, {}, 0, wave(1, 0, Tr)),
    ("wave-0-100", 1000, 100, 0, FIVE, 1, F, {}, 0, wave(2, 0, F)),
    ("wave-0-128", 1000, 128, 0, FIVE, 1, F, {}, 0, wave(2, 0, Tr)),
    ("wave-0-200", 500, 200, 0, FIVE, 1, F, {}, 0, wave(4, 0, F)),
    ("wave-0-256", 500, 256, 0, FIVE, 1, F, {}, 0, wave(4, 0, Tr)),
    ("wave-2-30", 1000, 30, 0, FIVE, 2, F, {}, 0, wave(1, 2, F)),
    ("wave-2-64", 1000, 64, 0, FIVE, 2, F, {}, 0, wave(1, 2, Tr)),
    ("wave-2-100", 1000, 100, 0, FIVE, 2, F, {}, 0, wave(2, 2, F)),
    ("wave-2-128", 1000, 128, 0, FIVE, 2, F, {}, 0, wave(2, 2, Tr)),
    ("wave-2-200", 500, 200, 0, FIVE, 2, F, {}, 0, wave(4, 2, F)),
    ("wave-2-256", 500, 256, 0, FIVE, 2, F, {}, 0, wave(4, 2, Tr)),
    ("wave-3-56", 2000, 56, 0, DEPLOYED, 1, F, {}, 0, wave(1, 3, F)),
    ("wave-3-64", 1000, 64, 0, DEPLOYED, 1, F, {}, 0, wave(1, 3, Tr)),
    ("wave-3-100", 1000, 100, 0, DEPLOYED, 1, F, {}, 0, wave(2, 3, F)),
    ("wave-3-128", 1000, 128, 0, DEPLOYED, 1, F, {}, 0, wave(2, 3, Tr)),
    ("wave-3-200", 500, 200, 0, DEPLOYED, 1, F, {}, 0, wave(4, 3, F)),
    ("wave-3-256", 500, 256, 0, DEPLOYED, 1, F, {}, 0, wave(4, 3, Tr)),
    # a lane-pass context whose tick the lane pass does not take: the wave pass
    ("wave-ga-128", 2048, 128, LANE, FIVE, 1, Tr, {}, 0, wave(2, 3, Tr)),
    ("wave-power-2-lane-ctx", 2048, 64, LANE, FIVE, 2, F, {}, 0, wave(1, 2, Tr)),
]


def make_ctx(Smpc, monkeypatch, B, T, flags, names, power, near, env):
    cfg, scn, noise = make_case(B, T, near_goal=near)
    cfg.flags |= flags
    g = create_with_env(Smpc, monkeypatch, cfg, env)
    configure(g, scn, critics=critics_of(names, power), noise=noise)
    return g, scn


@pytest.mark.parametrize("case", TICKS, ids=[c[0] for c in TICKS])
def test_tick_runs_the_pinned_instance(Smpc, monkeypatch, case):
    name, B, T, flags, names, power, near, env, kind, kernel = case
    g, scn = make_ctx(Smpc, monkeypatch, B, T, flags, names, power, near, env)
    u = scn.u0
    for k in range(2):       # the first tick without a furthest-point prediction, the second speculated
        u, out = g.optimize(scn.tick, u)
        print(f"[selection] {name} tick {k}: pass_kind {out.pass_kind} kernel {last_kernel(g)}")
        assert (out.pass_kind, last_kernel(g)) == (kind, kernel), (name, k)
    g.close()


@pytest.mark.parametrize("T,r,full", [(30, 1, F), (64, 1, Tr), (100, 2, F), (128, 2, Tr), (200, 4, F), (256, 4, Tr)])
def test_furthest_only_pass_runs_the_pinned_instance(Smpc, monkeypatch, T, r, full):
    """MODE 1 of the wave pass scores nothing and finds the furthest reached path point: a tick
    launches it in front of its first scoring pass; the step-wise sharded API launches it alone."""
    import torch
    g, scn = make_ctx(Smpc, monkeypatch, 500, T, 0, FIVE, 1, F, {})
    t_f = torch.zeros(8, dtype=torch.float32, device="cuda")
    g.set_stream(torch.cuda.current_stream().cuda_stream)
    g.shard_begin(scn.tick, scn.u0)
    g.shard_furthest(t_f.data_ptr())
    torch.cuda.synchronize()
    print(f"[selection] furthest only T {T}: kernel {last_kernel(g)}")
    assert last_kernel(g) == wave(r, 1, full)
    assert float(t_f[0]) > 0.0
    g.close()


# (id, batch, horizon, critic names) -> kernel of a member scored alone, kernel of the batched launch
GROUPS = [
    ("group-64", 2048, 64, FIVE, lane(), lane(many=True)),
    ("group-56", 2048, 56, FIVE, lane(56), lane(full=False, many=True, quads=False)),
    ("group-64-no-obst", 2048, 64, NO_OBST, lane(obst=False), lane(obst=False, many=True)),
    ("group-40-no-obst", 2048, 40, NO_OBST, lane(full=False, obst=False, quads=False), lane(full=False, obst=False, many=True, quads=False)),
    ("group-dep-64", 4096, 64, DEPLOYED, lane(dep=True), lane(many=True, dep=True)),
    ("group-dep-56", 4096, 56, DEPLOYED, lane(56, dep=True), lane(full=False, many=True, tc=56, dep=True)),
]


@pytest.mark.parametrize("case", GROUPS, ids=[c[0] for c in GROUPS])
def test_group_runs_the_pinned_instance(Smpc, case):
    """smpc_group_optimize: the batched launch's instance.  The first tick has no furthest-point
    prediction and a missed prediction re-scores a member alone, after the batched launch: the
    kernel launched last is then that member's own instance."""
    from mpcholonavigation_amd.optimizer import SmpcGroup
    name, B, T, names, alone, kernel = case
    n = 3
    members, scns = [], []
    for i in range(n):
        cfg = default_config(batch_size=B, time_steps=T, flags=LANE)
        scn = make_scenario(T, seed=70 + i)
        g = Smpc(cfg)
        configure(g, scn, critics=critics_of(names), noise=make_noise(B, T, seed=950 + i))
        members.append(g)
        scns.append(scn)
    grp = SmpcGroup(members)
    us = [scn.u0 for scn in scns]
    seen = []
    for k in range(5):
        res = grp.optimize([scn.tick for scn in scns], us)
        us = [shifted(u) for u, _ in res]
        assert all(o.pass_kind == 1 for _, o in res)
        seen.append(last_kernel(members[0]))
    print(f"[selection] {name}: kernel launched last, per tick: {seen}")
    assert seen[0] == alone, name
    assert kernel in seen[1:] and set(seen) == {alone, kernel}, name
    grp.close()
    for g in members:
        g.close()


# a tick whose flags are stripped after the launch was planned (fail_flag_in: the retry after
# fallback() scores nothing, critic_manager.cpp:70-73) runs what the stripped flags have an instance for
DOWNGRADES = [
    ("reread-128-to-wave", 2048, 128, LANE, {}, 1, lane(128), 0, wave(2, 0, Tr)),
    ("reread-64-to-wave", 2048, 64, LANE, {"SMPC_LANE_REREAD": "1"}, 1, lane(rr=True), 0, wave(1, 0, Tr)),
    ("split-to-lane", 16384, 64, 0, {}, 2, "smpc_pass_split<4, true>", 1, lane(obst=False)),
    ("split-masked-to-lane", 20000, 60, 0, {}, 2, "smpc_pass_split<4, false>", 1, lane(full=False, obst=False, quads=False)),
    ("lane-56-stays-lane", 2048, 56, LANE, {}, 1, lane(56), 1, lane(full=False, obst=False, quads=False)),
]


@pytest.mark.parametrize("case", DOWNGRADES, ids=[c[0] for c in DOWNGRADES])
def test_stripped_tick_runs_the_pinned_instance(Smpc, monkeypatch, case):
    name, B, T, flags, env, kind, kernel, kind_stripped, kernel_stripped = case
    g, scn = make_ctx(Smpc, monkeypatch, B, T, flags, FIVE, 1, F, env)
    u, out = g.optimize(scn.tick, scn.u0)
    print(f"[selection] {name}: pass_kind {out.pass_kind} kernel {last_kernel(g)}")
    assert (out.pass_kind, last_kernel(g)) == (kind, kernel), name
    t = scn.tick
    t2 = Tick(t.pose_x, t.pose_y, t.pose_yaw, t.speed, t.path_x, t.path_y, t.path_yaw, t.goal_x, t.goal_y,
              fail_flag_in=True)
    u, out = g.optimize(t2, np.zeros_like(scn.u0))
    print(f"[selection] {name} stripped: pass_kind {out.pass_kind} kernel {last_kernel(g)}")
    assert out.fail_flag == 1
    assert (out.pass_kind, last_kernel(g)) == (kind_stripped, kernel_stripped), name
    g.close()
