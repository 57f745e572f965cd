#!/usr/bin/env python3
"""Developer tool: round time of a fleet at the deployed configuration through the fleet host.

N members as tools/fleet_tick.py builds them (the deployed critic list as written: nine critics,
CostCritic consider_footprint on, a 0.5 x 0.36 m rectangle, 2 000 rollouts x 56 steps, own device
noise), here as sortham::Optimizer objects in a sortham::FleetOptimizer.  Three variants take turns
in one process, block after block:

  (a) alone  — every member's own evalControl, one after the other, on its ungrouped context
               (sortham_fleet_run_rounds with alone = 1): what a caller without the fleet runs;
  (b) fleet  — the fleet round (sortham_fleet_run_rounds): one smpc_group_optimize_some call and the
               reference's evalControl around it per member; the same compiled loop as (a);
  (c) raw    — smpc_group_optimize on N bare contexts from the Python loop of tools/fleet_tick.py
               (no fallback, filter, Twist; the shift in numpy).

    fleet_host_tick.py [--scene open|wall|both] [--members 1,2,4,8,16] [--blocks 5] [--rounds 200]
                       [--warmup 30] [--out DIR] [BxT]

One JSON line per scene and N on stdout (block times in us per round, median, spread = max - min over
the blocks); with --out, the lines in DIR/fleet_host.jsonl and the table in DIR/fleet_host_table.txt.
(b) - (c) per member is the host's share: fallback, filter, Twist, shift and the plan copy of the C
face, against a caller that does none of it."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from mpcholonavigation_amd.host_optimizer import FleetOptimizer, Optimizer
from mpcholonavigation_amd.optimizer import SmpcGroup
from mpcholonavigation_amd.synthetic import make_scenario, wall_beside_path
from mpcholonavigation_amd.tick import default_config, default_critics
from tools.fleet_tick import ALL, DEPLOYED, FOOTPRINT, member, option, shifted

CLASSES = ["".join(w.capitalize() for w in n.split("_")) + "Critic" for n in DEPLOYED]


def host_member(B, T, scn, seed):
    cr = default_critics()
    for n in ALL:
        getattr(cr, n).enabled = 1 if n in DEPLOYED else 0
    cr.cost.consider_footprint = 1
    h = Optimizer(default_config(batch_size=B, time_steps=T), cr, 20.0, critics=CLASSES, noise_seed=seed)
    h.set_costmap(scn.cells, scn.origin_x, scn.origin_y, scn.resolution)
    h.set_footprint(FOOTPRINT, circumscribed_radius=float(np.hypot(0.25, 0.18)), layer_cost_scaling_factor=10.0)
    return h


def summary(v):
    return {"blocks": [round(x, 2) for x in v], "median": round(float(np.median(v)), 2), "spread": round(max(v) - min(v), 2)}


def measure(scene, N, B, T, blocks, rounds, warmup):
    scn = make_scenario(T)
    if scene == "wall":
        scn.cells = wall_beside_path(scn)
    hosts = [host_member(B, T, scn, 1 + i) for i in range(N)]
    fleet = FleetOptimizer(hosts)
    raws = [member(B, T, scn, 1 + i) for i in range(N)]
    grp = SmpcGroup(raws)
    ticks = [scn.tick] * N
    state = {"us": [scn.u0] * N}

    def timed(f, n):
        t0 = time.perf_counter()
        res = f(n)
        return (time.perf_counter() - t0) / n * 1e6, res

    def alone(n):
        return fleet.run_rounds(ticks, n, alone=True)

    def grouped(n):
        return fleet.run_rounds(ticks, n)

    def raw(n):
        for _ in range(n):
            res = grp.optimize(ticks, state["us"])
            state["us"] = [shifted(u) for u, _ in res]
        return res

    for f in (alone, grouped, raw):
        f(warmup)
    a, b, c = [], [], []
    for _ in range(blocks):
        a.append(timed(alone, rounds)[0])
        grouped(2)                      # (the fleet forms its group again: not in the timed block)
        before = fleet.stats()
        us_b, res = timed(grouped, rounds)
        after = fleet.stats()
        b.append(us_b)
        c.append(timed(raw, rounds)[0])
    line = {"scene": scene, "B": B, "T": T, "members": N, "rounds_per_block": rounds,
            "alone_us": summary(a), "fleet_us": summary(b), "raw_group_us": summary(c),
            "fleet_minus_alone_us": round(float(np.median(b) - np.median(a)), 2),
            "host_share_us_per_member": round(float(np.median(b) - np.median(c)) / N, 2),
            "last_fleet_block": {"batched_launches": after.batched_launches - before.batched_launches,
                                 "single_ticks": after.single_ticks - before.single_ticks,
                                 "retries": after.retries - before.retries},
            "status": [int(r.status) for r in res], "passes": [int(r.out.passes) for r in res],
            "non_colliding": [int(r.out.non_colliding) for r in res]}
    fleet.close()
    grp.close()
    for x in hosts + raws:
        x.close()
    return line


def table(lines):
    out = []
    for scene in dict.fromkeys(ln["scene"] for ln in lines):
        rows = [ln for ln in lines if ln["scene"] == scene]
        out.append(f"scene {scene}, {rows[0]['B']} x {rows[0]['T']}; us per round, median (spread) over "
                   f"{len(rows[0]['alone_us']['blocks'])} blocks of {rows[0]['rounds_per_block']} rounds")
        out.append("  N | (a) members alone | (b) fleet round | (c) raw group round | (a) - (b), over the larger spread | "
                   "(b) - (c) per member | last (b) block: batched launches / single ticks")
        for ln in rows:
            a, b, c = ln["alone_us"], ln["fleet_us"], ln["raw_group_us"]
            gain = a["median"] - b["median"]
            big = max(a["spread"], b["spread"], 1e-9)
            lb = ln["last_fleet_block"]
            out.append(f" {ln['members']:2d} | {a['median']:8.1f} ({a['spread']:5.1f}) | {b['median']:8.1f} ({b['spread']:5.1f}) | "
                       f"{c['median']:8.1f} ({c['spread']:5.1f}) | {gain:8.1f} {gain / big:6.1f} | "
                       f"{ln['host_share_us_per_member']:6.2f} | {lb['batched_launches']} / {lb['single_ticks']}")
        out.append("")
    return "\n".join(out)


def main():
    args = sys.argv[1:]
    scene = option(args, "--scene", "both")
    counts = [int(v) for v in option(args, "--members", "1,2,4,8,16").split(",")]
    blocks, rounds = int(option(args, "--blocks", "5")), int(option(args, "--rounds", "200"))
    warmup = int(option(args, "--warmup", "30"))
    out_dir = option(args, "--out", "")
    B, T = (int(v) for v in (args[0] if args else "2000x56").split("x"))
    if scene not in ("open", "wall", "both"):
        sys.exit("--scene open|wall|both")
    lines = []
    for s in (("open", "wall") if scene == "both" else (scene,)):
        for N in counts:
            lines.append(measure(s, N, B, T, blocks, rounds, warmup))
            print(json.dumps(lines[-1]), flush=True)
    text = table(lines)
    print(text)
    if out_dir:
        os.makedirs(out_dir, exist_ok=True)
        with open(os.path.join(out_dir, "fleet_host.jsonl"), "w") as f:
            f.writelines(json.dumps(ln) + "\n" for ln in lines)
        with open(os.path.join(out_dir, "fleet_host_table.txt"), "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
