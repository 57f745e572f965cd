#!/usr/bin/env python3
"""Developer tool: wall time of the trajectory validator at the deployed configuration.

  single  one smpc_validate_trajectory (with the footprint and 15 moving obstacles, lookahead 2 s) on a
          context at 2 000 rollouts x 56 steps with the deployed critic list, next to that context's
          smpc_optimize tick in the same process, blocks of the two alternating;
  group   one smpc_group_validate_trajectories for N grouped members against the same number of
          ungrouped twins' single calls one after the other, alternating likewise.

    validate_tick.py [--members 2,4,8,16] [--calls 60] [--block 10] [--repeats 2] [--warm 100] [BxT]

Timed at the C-ABI (ctypes, the argument arrays built once).  One JSON line per measurement on stdout,
then a table.  Needs an MI355X; the first --warm calls of either route are not timed."""
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from mpcholonavigation_amd import _abi as A
from mpcholonavigation_amd.optimizer import Smpc, SmpcGroup, validation_params
from mpcholonavigation_amd.synthetic import make_scenario, wall_beside_path
from mpcholonavigation_amd.tick import default_config, default_critics

DEPLOYED = ("constraint", "cost", "goal", "goal_angle", "path_align", "path_follow", "path_angle",
            "prefer_forward", "twirling")
ALL = ("obstacles", "path_align", "path_follow", "goal_angle", "prefer_forward", "cost", "goal", "constraint",
       "twirling", "path_angle", "velocity_deadband")
FOOTPRINT = np.array([[0.25, 0.18], [0.25, -0.18], [-0.25, -0.18], [-0.25, 0.18]])
DISCS = 15


def option(args, name, default):
    if name in args:
        i = args.index(name)
        v = args[i + 1]
        del args[i:i + 2]
        return v
    return default


def discs(scn, T, seed):
    """DISCS discs beside and ahead of the path, none of them on it: every one is checked at every pose."""
    rng = np.random.default_rng(seed)
    xy = np.zeros((DISCS, T, 2), np.float32)
    xy[:, :, 0] = (scn.tick.pose_x + rng.uniform(0.2, 2.0, DISCS))[:, None] + 0.005 * np.arange(T)[None, :]
    xy[:, :, 1] = (scn.tick.pose_y + rng.choice([-1.0, 1.0], DISCS) * rng.uniform(0.9, 1.6, DISCS))[:, None]
    return xy, np.full(DISCS, 0.4, np.float32)


def member(B, T, scn, seed):
    cr = default_critics()
    for n in ALL:
        getattr(cr, n).enabled = 1 if n in DEPLOYED else 0
    cr.cost.consider_footprint = 1
    g = Smpc(default_config(batch_size=B, time_steps=T))
    g.set_critics(cr)
    g.set_costmap(scn.cells, scn.origin_x, scn.origin_y, scn.resolution)
    g.set_footprint(FOOTPRINT, circumscribed_radius=float(np.hypot(0.25, 0.18)), layer_cost_scaling_factor=10.0)
    g.set_moving_obstacles(*discs(scn, T, seed))
    g.seed(seed)
    return g


def timed(fn, n):
    out = []
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def alternate(a, b, calls, block, repeats):
    """Blocks of a and b in turn.  -> (median a, spread of a's repeat medians, median b, spread of b's)."""
    med_a, med_b, all_a, all_b = [], [], [], []
    for _ in range(repeats):
        xa, xb = [], []
        while len(xa) < calls:
            xa += timed(a, block)
            xb += timed(b, block)
        med_a.append(float(np.median(xa)))
        med_b.append(float(np.median(xb)))
        all_a += xa
        all_b += xb
    return (float(np.median(all_a)), max(med_a) - min(med_a), float(np.median(all_b)), max(med_b) - min(med_b))


def main():
    args = sys.argv[1:]
    counts = [int(v) for v in option(args, "--members", "2,4,8,16").split(",")]
    calls, block = int(option(args, "--calls", "60")), int(option(args, "--block", "10"))
    repeats, warm = int(option(args, "--repeats", "2")), int(option(args, "--warm", "100"))
    B, T = (int(v) for v in (args[0] if args else "2000x56").split("x"))
    scn = make_scenario(T)
    scn.cells = wall_beside_path(scn)
    pose = (scn.tick.pose_x, scn.tick.pose_y, scn.tick.pose_yaw)
    rows = []

    # ---- the single call next to the tick ----
    g = member(B, T, scn, 1)
    lib = g.lib
    u = np.ascontiguousarray(scn.u0, np.float32)
    for _ in range(4):
        u, _ = g.optimize(scn.tick, u)
        u = np.ascontiguousarray(np.concatenate([u[:, 1:], u[:, -1:]], axis=1))
    p = validation_params(lib, consider_footprint=True)
    out, tout = A.SmpcValidation(), A.SmpcTickOut()
    ut = u.copy()

    def one_validation():
        rc = lib.smpc_validate_trajectory(g.h, C.byref(p), pose[0], pose[1], pose[2], u.ctypes.data, C.byref(out), None)
        assert rc == 0, rc

    def one_tick():
        ut[:] = u
        rc = lib.smpc_optimize(g.h, C.byref(scn.tick.c), ut.ctypes.data, C.byref(tout))
        assert rc == 0, rc

    timed(one_validation, warm)
    timed(one_tick, warm)
    v_ms, v_sp, t_ms, t_sp = alternate(one_validation, one_tick, calls, block, repeats)
    line = {"what": "single", "B": B, "T": T, "discs": DISCS, "footprint": True, "checked": int(out.checked),
            "valid": int(out.valid), "validate_ms_median": round(v_ms, 4), "validate_ms_spread": round(v_sp, 4),
            "tick_ms_median": round(t_ms, 4), "tick_ms_spread": round(t_sp, 4)}
    print(json.dumps(line), flush=True)
    rows.append(line)
    g.close()

    # ---- the group call against the twins' single calls ----
    for N in counts:
        members = [member(B, T, scn, 1 + i) for i in range(N)]
        twins = [member(B, T, scn, 1 + i) for i in range(N)]
        grp = SmpcGroup(members)
        params = (A.SmpcValidationParams * N)(*[p] * N)
        poses = (C.c_double * (3 * N))(*(list(pose) * N))
        ubuf = np.ascontiguousarray(np.stack([u] * N), np.float32)
        uptr = (C.c_void_p * N)(*[ubuf[i].ctypes.data for i in range(N)])
        outs, outs1 = (A.SmpcValidation * N)(), (A.SmpcValidation * N)()
        status = (C.c_int32 * N)()

        def grouped_call():
            rc = lib.smpc_group_validate_trajectories(grp.h, params, poses, uptr, None, outs, None, status)
            assert rc == 0 and not any(status), (rc, list(status))

        def one_by_one():
            for i, t in enumerate(twins):
                rc = lib.smpc_validate_trajectory(t.h, C.byref(p), pose[0], pose[1], pose[2], uptr[i], C.byref(outs1[i]), None)
                assert rc == 0, rc

        timed(grouped_call, warm)
        timed(one_by_one, max(warm // N, 10))
        for i in range(N):
            assert bytes(outs[i]) == bytes(outs1[i]), f"member {i}: grouped and single verdicts differ"
        g_ms, g_sp, s_ms, s_sp = alternate(grouped_call, one_by_one, calls, block, repeats)
        cnt = grp.validation_counts()
        line = {"what": "group", "B": B, "T": T, "members": N, "grouped_ms_median": round(g_ms, 4),
                "grouped_ms_spread": round(g_sp, 4), "one_by_one_ms_median": round(s_ms, 4),
                "one_by_one_ms_spread": round(s_sp, 4), "grouped_over_one_by_one": round(g_ms / s_ms, 3),
                "launches": int(cnt.launches), "members_carried": int(cnt.members)}
        print(json.dumps(line), flush=True)
        rows.append(line)
        grp.close()
        for m in members + twins:
            m.close()

    s = rows[0]
    print(f"\nsingle call {s['validate_ms_median']:.3f} ms (spread {s['validate_ms_spread']:.3f}), "
          f"tick {s['tick_ms_median']:.3f} ms (spread {s['tick_ms_spread']:.3f}) at {B} x {T}")
    print(f"{'N':>3} {'grouped ms':>11} {'(spread)':>9} {'one by one ms':>14} {'(spread)':>9} {'ratio':>6}")
    for r in rows[1:]:
        print(f"{r['members']:>3} {r['grouped_ms_median']:>11.3f} {r['grouped_ms_spread']:>9.3f} "
              f"{r['one_by_one_ms_median']:>14.3f} {r['one_by_one_ms_spread']:>9.3f} {r['grouped_over_one_by_one']:>6.3f}")


if __name__ == "__main__":
    main()
