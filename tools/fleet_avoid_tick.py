#!/usr/bin/env python3
"""Developer tool: what mutual avoidance (FleetOptimizer::setMutualAvoidance) costs per fleet round.

    tools/fleet_avoid_tick.py [--members 2,16] [--blocks 5] [--rounds 200] [--warmup 30] [BxT]

N members as tools/fleet_host_tick.py builds them (the deployed critic list as written, 2 000 x 56,
own device noise) in one sortham::FleetOptimizer, every member on the scene's own tick as that tool has
them: with avoidance on every member then has all the others on top of it, so every term of the
kernel is live — its most expensive case — and the round's grouping is the one of the figures there.  Blocks of rounds from the compiled loop
(sortham_fleet_run_rounds) take turns in one process behind a warm-up: avoidance off — the round as
it is without the feature — on, N - 1 discs per member, and on by the per-member route.  Per round
with avoidance on, on top of the round: per member the table built on the host (N - 1 trajectories
integrated); then
  on             ONE smpc_group_set_moving_obstacles for the fleet (every table checked and laid out
                 in the group's pinned staging buffer, ONE asynchronous upload on the group's stream)
                 and ONE smpc_moving_cost_rm_many launch behind the hand-over, the member as a grid
                 dimension;
  on_per_member  a second fleet of N members of its own, built the same way and created under
                 SMPC_FLEET_AVOID=per_member: per member Optimizer::setMovingObstacles and
                 smpc_set_moving_obstacles (its own staging copy, upload and event) and one
                 smpc_moving_cost launch ahead of the grouped pass — the route before the grouped one.
One JSON line per N: us per round, median and spread over the blocks, and what the grouped route's
counters (FleetOptimizer.moving_launches) added per round in the last block of each."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from mpcholonavigation_amd.host_optimizer import FleetOptimizer
from mpcholonavigation_amd.synthetic import make_scenario
from tools.fleet_host_tick import host_member, summary
from tools.fleet_tick import option

ROBOT_RADIUS = 0.2


def measure(N, B, T, blocks, rounds, warmup):
    scn = make_scenario(T)
    hosts = [host_member(B, T, scn, 1 + i) for i in range(N)]
    fleet = FleetOptimizer(hosts)
    # the per-member route: members of its own (a context is in one fleet), the knob read at creation
    hosts_pm = [host_member(B, T, scn, 1 + i) for i in range(N)]
    os.environ["SMPC_FLEET_AVOID"] = "per_member"
    fleet_pm = FleetOptimizer(hosts_pm)
    del os.environ["SMPC_FLEET_AVOID"]
    ticks = [scn.tick] * N
    OFF, ON, PER_MEMBER = "off", "on", "on_per_member"

    def block(which, n):
        f = fleet_pm if which == PER_MEMBER else fleet
        f.set_mutual_avoidance(None if which == OFF else [ROBOT_RADIUS] * N)
        f.run_rounds(ticks, 2)          # (the switch itself, and a regroup if there was one: not timed)
        before, moving_before = f.stats(), f.moving_launches()
        t0 = time.perf_counter()
        res = f.run_rounds(ticks, n)
        us = (time.perf_counter() - t0) / n * 1e6
        after, moving_after = f.stats(), f.moving_launches()
        return us, res, {"batched_launches": after.batched_launches - before.batched_launches,
                         "single_ticks": after.single_ticks - before.single_ticks,
                         "grouped_moving_launches_per_round": (moving_after.grouped_launches - moving_before.grouped_launches) / n,
                         "table_uploads_per_round": (moving_after.table_uploads - moving_before.table_uploads) / n}

    for which in (OFF, ON, PER_MEMBER):
        block(which, warmup)
    off_us, on_us, pm_us, last = [], [], [], {}
    for _ in range(blocks):
        for which, acc in ((OFF, off_us), (ON, on_us), (PER_MEMBER, pm_us)):
            us, r, counts = block(which, rounds)
            acc.append(us)
            last[which] = counts
            if which == ON:
                res = r
    reach = []
    for h in hosts:
        try:
            reach.append(float((h.moving_obstacle_costs()[0] > 0).mean()))
        except RuntimeError:      # (its last tick was a retry with fail_flag_in: it scored nothing)
            pass
    reach = float(np.mean(reach)) if reach else float("nan")
    line = {"B": B, "T": T, "members": N, "rounds_per_block": rounds, "off_us": summary(off_us), "on_us": summary(on_us),
            "on_per_member_us": summary(pm_us),
            "on_minus_off_us": round(float(np.median(on_us) - np.median(off_us)), 2),
            "per_member_us": round(float(np.median(on_us) - np.median(off_us)) / N, 2),
            "on_per_member_minus_on_us": round(float(np.median(pm_us) - np.median(on_us)), 2),
            "last_block": last,
            "share_of_rollouts_within_reach": round(reach, 3), "status": [int(r.status) for r in res], "fail_flag": [int(r.out.fail_flag) for r in res],
            "retries": fleet.stats().retries}
    fleet.close()
    fleet_pm.close()
    for h in hosts + hosts_pm:
        h.close()
    return line


def main():
    args = sys.argv[1:]
    counts = [int(v) for v in option(args, "--members", "2,16").split(",")]
    blocks, rounds = int(option(args, "--blocks", "5")), int(option(args, "--rounds", "200"))
    warmup = int(option(args, "--warmup", "30"))
    B, T = (int(v) for v in (args[0] if args else "2000x56").split("x"))
    for N in counts:
        print(json.dumps(measure(N, B, T, blocks, rounds, warmup)), flush=True)


if __name__ == "__main__":
    main()
