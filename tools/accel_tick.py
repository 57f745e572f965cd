#!/usr/bin/env python3
"""Developer tool: what the acceleration limits (smpc_set_acceleration_limits) cost per tick.

    tools/accel_tick.py [deployed:BxT | five:BxT ...]
                        (default: deployed:2000x56 five:65536x64 five:2097152x64)

Per configuration, in one process and behind the clock warm-up of bench.py (200 ms of the workload's
own ticks), iteration_count 1, stored noise from the device RNG, two contexts that differ in the
limits alone — off (the tick as it is without the feature) and 3 / -3 / 3 / 3.5 — timed in turn,
ROUNDS times over, so that a drift of the clocks meets both.  Figures: the whole call on the device
by HIP events (SMPC_FLAG_PROFILE; the limiter's launch lies inside it), the limiter kernel alone by
HIP events of its own, and the wall time of a tick with the events off.  The limiter moves
24 B T bytes (three tensors in, three out): its share of 8 TB/s is printed beside its time."""
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
LIMITS = (3.0, -3.0, 3.0, 3.5)
HBM_BYTES_PER_S = 8.0e12
CLOCK_WARMUP_MS = 200.0
ROUNDS, WARM, TIMED = 3, 20, 60


def shift(u):
    return np.concatenate([u[:, 1:], u[:, -1:]], axis=1)


def kernel_name(g):
    f = g.lib.smpc_debug_last_pass_kernel
    f.restype, f.argtypes = ctypes.c_char_p, []
    return f().decode()


def limiter_ms(g):
    f = g.lib.smpc_debug_limit_ms
    f.restype, f.argtypes = ctypes.c_int, [A._ctx, ctypes.POINTER(ctypes.c_float)]
    ms = ctypes.c_float(0)
    return float(ms.value) if f(g.h, ctypes.byref(ms)) == 0 else float("nan")


def make(names, B, T, limits):
    cr = default_critics()
    for n in ALL:
        getattr(cr, n).enabled = 1 if n in names else 0
    scn = make_scenario(T)
    g = Smpc(default_config(batch_size=B, time_steps=T, flags=A.SMPC_FLAG_PROFILE))
    g.set_critics(cr)
    g.set_costmap(scn.cells, scn.origin_x, scn.origin_y, scn.resolution, inscribed_radius=scn.inscribed_radius,
                  cost_scaling_factor=scn.cost_scaling_factor, inflation_radius=scn.inflation_radius)
    g.seed(1234)
    if limits:
        g.set_acceleration_limits(*limits)
    return g, scn


def main():
    args = sys.argv[1:] or ["deployed:2000x56", "five:65536x64", "five:2097152x64"]
    print(f"library: {LIB_PATH}")
    for a in args:
        which, size = a.split(":")
        B, T = (int(v) for v in size.split("x"))
        names = DEPLOYED if which == "deployed" else FIVE
        ctxs = [("limits off", *make(names, B, T, None)), ("limits on", *make(names, B, T, LIMITS))]
        us = {label: scn.u0 for label, _, scn in ctxs}
        t0 = time.perf_counter()      # the clock warm-up: the workload's own ticks
        while (time.perf_counter() - t0) * 1e3 < CLOCK_WARMUP_MS:
            for label, g, scn in ctxs:
                un, _ = g.optimize(scn.tick, us[label])
                us[label] = shift(un)
        res = {label: {"dev": [], "lim": [], "wall": []} for label, _, _ in ctxs}
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
                        if label == "limits on":
                            res[label]["lim"].append(limiter_ms(g))
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
            line = (f"{which} {B}x{T} {label:10s}: device {float(np.median(r['dev'])) * 1e3:8.1f} us, "
                    f"tick {float(np.median(r['wall'])) * 1e3:8.1f} us (rounds {' '.join('%.1f' % (w * 1e3) for w in r['wall'])})")
            if r["lim"]:
                lim = float(np.median(r["lim"]))
                floor_ms = 24.0 * B * T / HBM_BYTES_PER_S * 1e3
                line += (f", limiter {lim * 1e3:8.1f} us = {100.0 * floor_ms / lim:5.1f} % of 24 B T / 8 TB/s "
                         f"({floor_ms * 1e3:.1f} us)")
            print(line + f", pass_kind {info[label][0]}, passes {info[label][2]}, {info[label][1]}", flush=True)
            g.close()


if __name__ == "__main__":
    main()
