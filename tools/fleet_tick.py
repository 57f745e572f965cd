#!/usr/bin/env python3
"""Developer tool: round time of a fleet at the deployed configuration through smpc_group_optimize.

N members, each the deployed critic list as written (robot_bringup/config/nav2_params.yaml: nine
critics, CostCritic consider_footprint on, a 0.5 x 0.36 m rectangle) at 2 000 rollouts x 56 steps,
no lane flag, own noise; one round = one smpc_group_optimize call = one tick of every member, closed
loop (each member continues from its own shifted control sequence).  Wall time per round over
blocks of rounds, every block printed, and — in the same process, in turn with the group's blocks — the
tick of one such context alone (smpc_optimize), so that the round can be set against N single ticks.

    fleet_tick.py [--scene open|wall] [--members 1,2,4,8,16] [--blocks 5] [--rounds 200] [--label TEXT] [BxT]

open: the make_scenario map (no obstacle near the path: no step wants the footprint walk);
wall: an inflated wall 0.35 m beside the path (synthetic.wall_beside_path: the walk runs).
One JSON line per N on stdout (block times in us, median, spread = max - min over the blocks, the
group's counters where the library has smpc_group_stats).  Two builds are compared by running this
tool from either tree in alternating processes; --label names the build in the line."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from mpcholonavigation_amd.optimizer import Smpc, SmpcGroup
from mpcholonavigation_amd.synthetic import make_scenario, wall_beside_path
from mpcholonavigation_amd.tick import default_config, default_critics

DEPLOYED = ("constraint", "cost", "goal", "goal_angle", "path_align", "path_follow", "path_angle",
            "prefer_forward", "twirling")
ALL = ("obstacles", "path_align", "path_follow", "goal_angle", "prefer_forward", "cost", "goal", "constraint",
       "twirling", "path_angle", "velocity_deadband")
FOOTPRINT = np.array([[0.25, 0.18], [0.25, -0.18], [-0.25, -0.18], [-0.25, 0.18]])


def option(args, name, default):
    if name in args:
        i = args.index(name)
        v = args[i + 1]
        del args[i:i + 2]
        return v
    return default


def member(B, T, scn, seed):
    cr = default_critics()
    for n in ALL:
        getattr(cr, n).enabled = 1 if n in DEPLOYED else 0
    cr.cost.consider_footprint = 1
    g = Smpc(default_config(batch_size=B, time_steps=T))
    g.set_critics(cr)
    g.set_costmap(scn.cells, scn.origin_x, scn.origin_y, scn.resolution)
    g.set_footprint(FOOTPRINT, circumscribed_radius=float(np.hypot(0.25, 0.18)), layer_cost_scaling_factor=10.0)
    g.seed(seed)
    return g


def shifted(u):
    return np.concatenate([u[:, 1:], u[:, -1:]], axis=1)


def main():
    args = sys.argv[1:]
    scene = option(args, "--scene", "open")
    counts = [int(v) for v in option(args, "--members", "1,2,4,8,16").split(",")]
    blocks, rounds = int(option(args, "--blocks", "5")), int(option(args, "--rounds", "200"))
    label = option(args, "--label", "")
    B, T = (int(v) for v in (args[0] if args else "2000x56").split("x"))
    if scene not in ("open", "wall"):
        sys.exit("--scene open|wall")
    scn = make_scenario(T)
    if scene == "wall":
        scn.cells = wall_beside_path(scn)

    lone = member(B, T, scn, 999)
    state = {"u": scn.u0}

    def lone_block(n):
        t0 = time.perf_counter()
        for _ in range(n):
            un, out = lone.optimize(scn.tick, state["u"])
            state["u"] = shifted(un)
        return (time.perf_counter() - t0) / n * 1e6, out

    lone_block(30)
    for N in counts:
        members = [member(B, T, scn, 1 + i) for i in range(N)]
        grp = SmpcGroup(members)
        ticks, us = [scn.tick] * N, [scn.u0] * N

        def block(n):
            nonlocal us
            t0 = time.perf_counter()
            for _ in range(n):
                res = grp.optimize(ticks, us)
                us = [shifted(u) for u, _ in res]
            return (time.perf_counter() - t0) / n * 1e6, res

        block(30)
        group_us, lone_us = [], []
        for _ in range(blocks):      # the group's blocks and the lone context's take turns
            us_round, res = block(rounds)
            group_us.append(us_round)
            lone_us.append(lone_block(rounds)[0])
        line = {"label": label, "scene": scene, "B": B, "T": T, "members": N, "rounds_per_block": rounds,
                "round_us_blocks": [round(v, 2) for v in group_us], "round_us_median": round(float(np.median(group_us)), 2),
                "round_us_spread": round(max(group_us) - min(group_us), 2),
                "single_tick_us_blocks": [round(v, 2) for v in lone_us],
                "single_tick_us_median": round(float(np.median(lone_us)), 2),
                "round_over_n_single": round(float(np.median(group_us)) / (N * float(np.median(lone_us))), 3),
                "passes": [int(o.passes) for _, o in res], "pass_kind": [int(o.pass_kind) for _, o in res],
                "non_colliding": [int(o.non_colliding) for _, o in res]}
        if hasattr(grp, "stats"):
            st = grp.stats()
            line["batched_launches"], line["single_ticks"] = int(st.batched_launches), int(st.single_ticks)
        print(json.dumps(line), flush=True)
        grp.close()
        for g in members:
            g.close()
    lone.close()


if __name__ == "__main__":
    main()
