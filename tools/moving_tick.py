#!/usr/bin/env python3
"""Developer tool: what the moving-obstacle term (smpc_set_moving_obstacles) costs per tick.

    tools/moving_tick.py [deployed:BxT:K | five:BxT:K ...]
                         (default: deployed:2000x56:15 five:65536x64:8 five:2097152x64:8)

Per configuration, in one process and behind the clock warm-up of bench.py (200 ms of the workload's
own ticks), iteration_count 1, stored noise from the device RNG, two contexts that differ in the
obstacles alone — none (the tick as it is without the feature) and K discs across the nominal path —
timed in turn, ROUNDS times over, so that a drift of the clocks meets both.  Figures: the whole call on
the device by HIP events (SMPC_FLAG_PROFILE; the term's launch lies inside it), the smpc_moving_cost
kernel alone by HIP events of its own, and the wall time of a tick with the events off.  The kernel
reads the noise once, 12 B T bytes with three tensors: its share of 8 TB/s is printed beside its time.
(A fleet round with mutual avoidance: tests/test_gpu_moving_obstacles.py drives one; its table upload
per member and round is host work this tool does not time.)"""
import ctypes
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from mpcholonavigation_amd import _abi as A
from mpcholonavigation_amd.optimizer import LIB_PATH, Smpc
from mpcholonavigation_amd.synthetic import make_scenario
from mpcholonavigation_amd.tick import default_config, default_critics

FIVE = ("obstacles", "path_align", "path_follow", "goal_angle", "prefer_forward")
DEPLOYED = ("constraint", "cost", "goal", "goal_angle", "path_align", "path_follow", "path_angle",
            "prefer_forward", "twirling")
ALL = ("obstacles", "path_align", "path_follow", "goal_angle", "prefer_forward", "cost", "goal", "constraint",
       "twirling", "path_angle", "velocity_deadband", "path_align_legacy")
HBM_BYTES_PER_S = 8.0e12
CLOCK_WARMUP_MS = 200.0
ROUNDS, WARM, TIMED = 3, 20, 60


def shift(u):
    return np.concatenate([u[:, 1:], u[:, -1:]], axis=1)


def kernel_name(g):
    f = g.lib.smpc_debug_last_pass_kernel
    f.restype, f.argtypes = ctypes.c_char_p, []
    return f().decode()


def moving_ms(g):
    f = g.lib.smpc_debug_moving_ms
    f.restype, f.argtypes = ctypes.c_int, [A._ctx, ctypes.POINTER(ctypes.c_float)]
    ms = ctypes.c_float(0)
    return float(ms.value) if f(g.h, ctypes.byref(ms)) == 0 else float("nan")


def discs(tick, T, dt, K, seed=3):
    """K discs that cross the nominal path ahead of the robot, each with a constant velocity."""
    rng = np.random.default_rng(seed)
    t = np.arange(1, T + 1) * dt
    xy = np.zeros((K, T, 2), np.float32)
    for k in range(K):
        a0, b0 = rng.uniform(0.2, 1.5), rng.uniform(-0.8, 0.8)
        va, vb = rng.uniform(-0.25, 0.25, 2)
        xy[k, :, 0] = tick.pose_x + a0 + va * t
        xy[k, :, 1] = tick.pose_y + b0 + vb * t
    return xy, rng.uniform(0.05, 0.2, K).astype(np.float32)


def make(names, B, T, K):
    cr = default_critics()
    for n in ALL:
        getattr(cr, n).enabled = 1 if n in names else 0
    scn = make_scenario(T)
    cfg = default_config(batch_size=B, time_steps=T, flags=A.SMPC_FLAG_PROFILE)
    g = Smpc(cfg)
    g.set_critics(cr)
    g.set_costmap(scn.cells, scn.origin_x, scn.origin_y, scn.resolution, inscribed_radius=scn.inscribed_radius,
                  cost_scaling_factor=scn.cost_scaling_factor, inflation_radius=scn.inflation_radius)
    g.seed(1234)
    if K:
        g.set_moving_obstacles(*discs(scn.tick, T, cfg.model_dt, K))
    return g, scn


def main():
    args = sys.argv[1:] or ["deployed:2000x56:15", "five:65536x64:8", "five:2097152x64:8"]
    print(f"library: {LIB_PATH}")
    for a in args:
        which, size, K = a.split(":")
        B, T = (int(v) for v in size.split("x"))
        K = int(K)
        names = DEPLOYED if which == "deployed" else FIVE
        ctxs = [("obstacles off", *make(names, B, T, 0)), ("obstacles on", *make(names, B, T, K))]
        us = {label: scn.u0 for label, _, scn in ctxs}
        t0 = time.perf_counter()      # the clock warm-up: the workload's own ticks
        while (time.perf_counter() - t0) * 1e3 < CLOCK_WARMUP_MS:
            for label, g, scn in ctxs:
                un, _ = g.optimize(scn.tick, us[label])
                us[label] = shift(un)
        res = {label: {"dev": [], "mov": [], "wall": []} for label, _, _ in ctxs}
        info = {}
        for _ in range(ROUNDS):
            for label, g, scn in ctxs:
                u = us[label]
                g.set_profile(True)
                for k in range(WARM + TIMED):
                    un, out = g.optimize(scn.tick, u)
                    u = shift(un)
                    if k >= WARM:
                        res[label]["dev"].append(out.device_ms)
                        if label == "obstacles on":
                            res[label]["mov"].append(moving_ms(g))
                info[label] = (out.pass_kind, kernel_name(g), out.passes)
                g.set_profile(False)
                t0 = time.perf_counter()
                for k in range(TIMED):
                    un, out = g.optimize(scn.tick, u)
                    u = shift(un)
                res[label]["wall"].append((time.perf_counter() - t0) / TIMED * 1e3)
                us[label] = u
        for label, g, _ in ctxs:
            r = res[label]
            line = (f"{which} {B}x{T} K={K} {label:13s}: device {float(np.median(r['dev'])) * 1e3:8.1f} us, "
                    f"tick {float(np.median(r['wall'])) * 1e3:8.1f} us (rounds {' '.join('%.1f' % (w * 1e3) for w in r['wall'])})")
            if r["mov"]:
                mov = float(np.median(r["mov"]))
                floor_ms = 12.0 * B * T / HBM_BYTES_PER_S * 1e3
                line += (f", smpc_moving_cost {mov * 1e3:8.1f} us = {100.0 * floor_ms / mov:5.1f} % of 12 B T / 8 TB/s "
                         f"({floor_ms * 1e3:.1f} us)")
            print(line + f", pass_kind {info[label][0]}, passes {info[label][2]}, {info[label][1]}", flush=True)
            g.close()


if __name__ == "__main__":
    main()
