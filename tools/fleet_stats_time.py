#!/usr/bin/env python3
"""Developer tool: wall time of one smpc_group_critic_breakdown for a fleet at the deployed
configuration, against the same members' smpc_critic_breakdown one after the other.

N members, each the deployed critic list as written (robot_bringup/config/nav2_params.yaml: nine
critics, CostCritic consider_footprint on, a 0.5 x 0.36 m rectangle) at 2 000 rollouts x 56 steps,
own noise, grouped; and N identically made contexts that are in no group (the route a fleet host had
before: ungroup, one call per robot — here without even the ungrouping).  Both are timed at the C-ABI
(ctypes, the argument arrays built once) in the same process, in turn: blocks of --block calls of the
grouped call and of one-by-one sweeps alternate until each has --calls of them; that is one repeat,
and the spread reported is the difference between the medians of --repeats repeats.

    fleet_stats_time.py [--scene open,wall] [--members 2,4,8,16] [--calls 60] [--block 10] [--repeats 2]
                        [--grouped-only] [BxT]

open: the make_scenario map (nothing near the path); wall: an inflated wall 0.35 m beside the path
(synthetic.wall_beside_path: the footprint walk runs).  One JSON line per scene and N on stdout, then a
table.  --grouped-only: only the grouped calls, for a kernel trace (rocprofv3 --kernel-trace --stats --
python tools/fleet_stats_time.py --grouped-only --members 16 --scene wall).  Needs an MI355X; the first
--warm calls of either route are not timed (clocks, allocations)."""
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from mpcholonavigation_amd import _abi as A
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


def flag(args, name):
    if name in args:
        args.remove(name)
        return True
    return False


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


def main():
    args = sys.argv[1:]
    scenes = option(args, "--scene", "open,wall").split(",")
    counts = [int(v) for v in option(args, "--members", "2,4,8,16").split(",")]
    calls, block = int(option(args, "--calls", "60")), int(option(args, "--block", "10"))
    repeats, warm = int(option(args, "--repeats", "2")), int(option(args, "--warm", "100"))
    grouped_only = flag(args, "--grouped-only")
    B, T = (int(v) for v in (args[0] if args else "2000x56").split("x"))
    rows = []
    for scene in scenes:
        if scene not in ("open", "wall"):
            sys.exit("--scene open|wall")
        scn = make_scenario(T)
        if scene == "wall":
            scn.cells = wall_beside_path(scn)
        for N in counts:
            members = [member(B, T, scn, 1 + i) for i in range(N)]
            twins = [] if grouped_only else [member(B, T, scn, 1 + i) for i in range(N)]
            grp = SmpcGroup(members)
            lib = grp.lib
            # a few rounds first: every member has a tick history and a shifted control sequence, as in a loop
            us = [scn.u0] * N
            for _ in range(4):
                res = grp.optimize([scn.tick] * N, us)
                for i, t in enumerate(twins):
                    t.optimize(scn.tick, us[i])
                us = [np.concatenate([u[:, 1:], u[:, -1:]], axis=1) for u, _ in res]
            ins = (A.SmpcTickIn * N)(*[scn.tick.c] * N)
            ubuf = np.ascontiguousarray(np.stack(us), np.float32)
            uptr = (C.c_void_p * N)(*[ubuf[i].ctypes.data for i in range(N)])
            st = (A.SmpcCriticStats * N)()
            st1 = (A.SmpcCriticStats * N)()
            status = (C.c_int32 * N)()
            one_in = C.byref(scn.tick.c)

            def grouped_call():
                rc = lib.smpc_group_critic_breakdown(grp.h, ins, uptr, None, st, None, status)
                assert rc == 0 and not any(status), (rc, list(status))

            def one_by_one():
                for i, t in enumerate(twins):
                    rc = lib.smpc_critic_breakdown(t.h, one_in, uptr[i], C.byref(st1[i]), None)
                    assert rc == 0, rc

            def timed(fn, n):
                out = []
                for _ in range(n):
                    t0 = time.perf_counter()
                    fn()
                    out.append((time.perf_counter() - t0) * 1e3)
                return out

            timed(grouped_call, warm)
            if not grouped_only:
                timed(one_by_one, max(warm // N, 10))
                for i in range(N):       # the two routes give the same statistics
                    assert bytes(st[i]) == bytes(st1[i]), f"member {i}: grouped and single statistics differ"
            med_g, med_s, all_g, all_s = [], [], [], []
            for _ in range(repeats):
                g_ms, s_ms = [], []
                while len(g_ms) < calls:
                    g_ms += timed(grouped_call, block)
                    if not grouped_only:
                        s_ms += timed(one_by_one, block)
                med_g.append(float(np.median(g_ms)))
                all_g += g_ms
                if s_ms:
                    med_s.append(float(np.median(s_ms)))
                    all_s += s_ms
            cnt = grp.breakdown_counts()
            line = {"scene": scene, "B": B, "T": T, "members": N, "calls_per_repeat": len(g_ms),
                    "grouped_ms_median": round(float(np.median(all_g)), 4), "grouped_ms_min": round(min(all_g), 4),
                    "grouped_ms_repeats": [round(v, 4) for v in med_g],
                    "grouped_ms_spread": round(max(med_g) - min(med_g), 4),
                    "batched_members": int(cnt.batched_members), "single_members": int(cnt.single_members),
                    "effective_samples": [round(float(s.effective_samples), 1) for s in st]}
            if all_s:
                line.update({"one_by_one_ms_median": round(float(np.median(all_s)), 4), "one_by_one_ms_min": round(min(all_s), 4),
                             "one_by_one_ms_repeats": [round(v, 4) for v in med_s],
                             "one_by_one_ms_spread": round(max(med_s) - min(med_s), 4),
                             "grouped_over_one_by_one": round(float(np.median(all_g)) / float(np.median(all_s)), 3)})
            print(json.dumps(line), flush=True)
            rows.append(line)
            grp.close()
            for g in members + twins:
                g.close()
    if not grouped_only:
        print(f"\n{'scene':6} {'N':>3} {'grouped ms':>11} {'(spread)':>9} {'one by one ms':>14} {'(spread)':>9} {'ratio':>6}")
        for r in rows:
            print(f"{r['scene']:6} {r['members']:>3} {r['grouped_ms_median']:>11.3f} {r['grouped_ms_spread']:>9.3f} "
                  f"{r['one_by_one_ms_median']:>14.3f} {r['one_by_one_ms_spread']:>9.3f} {r['grouped_over_one_by_one']:>6.3f}")


if __name__ == "__main__":
    main()
