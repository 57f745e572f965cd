#!/usr/bin/env python3
"""Developer tool: tick time of the north star's five critics with cost_power 2 against cost_power 1.

    tools/power_tick.py [BxT ...]          (default: 2097152x64 262144x64)

Per size, in one process and behind the clock warm-up of bench.py (200 ms of the workload's own
ticks), iteration_count 1, stored noise from the device RNG:
  power 1            the lean lane pass (smpc_pass_lane)
  power 2            the library's own route (from 61 440 rollouts: smpc_pass_lane_pow)
  power 2, wave      the same tick forced onto the general wave pass (SMPC_FLAG_WAVE_PER_ROLLOUT:
                     smpc_pass<R, 2, FULL>), the route a power tick had before the power rows
The three contexts are timed in turn, ROUNDS times over, so that a drift of the clocks meets all of
them.  Figures: the scoring-pass kernel and the whole call on the device by HIP events
(SMPC_FLAG_PROFILE), and the wall time of a tick with the events off.  With SMPC_LIB pointing at
another build of the library the same script times that build (its "power 2" line is then its own
route)."""
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
ALL = ("obstacles", "path_align", "path_follow", "goal_angle", "prefer_forward", "cost", "goal", "constraint",
       "twirling", "path_angle", "velocity_deadband", "path_align_legacy")
CLOCK_WARMUP_MS = 200.0
ROUNDS, WARM, TIMED = 3, 20, 60


def shift(u):
    return np.concatenate([u[:, 1:], u[:, -1:]], axis=1)


def kernel_name(g):
    f = g.lib.smpc_debug_last_pass_kernel
    f.restype, f.argtypes = ctypes.c_char_p, []
    return f().decode()


def make(B, T, power, flags):
    cr = default_critics()
    for n in ALL:
        sub = getattr(cr, n)
        sub.enabled = 1 if n in FIVE else 0
        sub.cost_power = power
    scn = make_scenario(T)
    g = Smpc(default_config(batch_size=B, time_steps=T, flags=flags | A.SMPC_FLAG_PROFILE))
    g.set_critics(cr)
    g.set_costmap(scn.cells, scn.origin_x, scn.origin_y, scn.resolution, inscribed_radius=scn.inscribed_radius,
                  cost_scaling_factor=scn.cost_scaling_factor, inflation_radius=scn.inflation_radius)
    g.seed(1234)
    return g, scn


def main():
    sizes = [tuple(int(v) for v in a.split("x")) for a in sys.argv[1:]] or [(2097152, 64), (262144, 64)]
    print(f"library: {LIB_PATH}")
    for B, T in sizes:
        ctxs = [("power 1", *make(B, T, 1, 0)), ("power 2", *make(B, T, 2, 0)),
                ("power 2, wave", *make(B, T, 2, A.SMPC_FLAG_WAVE_PER_ROLLOUT))]
        us = {label: scn.u0 for label, _, scn in ctxs}
        t0 = time.perf_counter()      # the clock warm-up: the workload's own ticks
        while (time.perf_counter() - t0) * 1e3 < CLOCK_WARMUP_MS:
            for label, g, scn in ctxs[:2]:
                un, _ = g.optimize(scn.tick, us[label])
                us[label] = shift(un)
        res = {label: {"pass": [], "dev": [], "wall": []} for label, _, _ in ctxs}
        info = {}
        for _ in range(ROUNDS):
            for label, g, scn in ctxs:
                u = us[label]
                g.set_profile(True)
                for k in range(WARM + TIMED):
                    un, out = g.optimize(scn.tick, u)
                    u = shift(un)
                    if k >= WARM:
                        res[label]["pass"].append(out.score_pass_ms)
                        res[label]["dev"].append(out.device_ms)
                info[label] = (out.pass_kind, kernel_name(g), out.passes)
                g.set_profile(False)
                t0 = time.perf_counter()
                for k in range(TIMED):
                    un, out = g.optimize(scn.tick, u)
                    u = shift(un)
                res[label]["wall"].append((time.perf_counter() - t0) / TIMED * 1e3)
                us[label] = u
        base = float(np.median(res["power 1"]["pass"]))
        for label, g, _ in ctxs:
            r = res[label]
            p = float(np.median(r["pass"]))
            print(f"{B}x{T} {label:14s}: scoring pass {p * 1e3:8.1f} us (x{p / base:5.3f} of power 1; rounds "
                  f"{' '.join('%.1f' % (float(np.median(r['pass'][i * TIMED:(i + 1) * TIMED])) * 1e3) for i in range(ROUNDS))}), "
                  f"device {float(np.median(r['dev'])) * 1e3:8.1f} us, tick {float(np.median(r['wall'])) * 1e3:8.1f} us, "
                  f"pass_kind {info[label][0]}, passes {info[label][2]}, {info[label][1]}", flush=True)
            g.close()


if __name__ == "__main__":
    main()
