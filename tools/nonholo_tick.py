#!/usr/bin/env python3
"""Developer tool: a DiffDrive tick on the lane pass without the vy stream (smpc_pass_lane_nh) against
the same tick on the Omni-form rows, and an Omni tick for scale.  Needs an MI355X.

    tools/nonholo_tick.py [BxT ...]      (default: 2097152x64 2097152x56 262144x64 61440x64)

Per size, in one process and behind the clock warm-up of bench.py (200 ms of the workload's own
ticks), the five critics, iteration_count 1, stored noise from the device RNG:
  DiffDrive          the library's own route (from 61 440 rollouts, plain cruise ticks: smpc_pass_lane_nh)
  DiffDrive, omni    the same tick from a context created under SMPC_NONHOLO_PASS=omni: the Omni-form
                     row, which reads the zero-filled vy noise and carries zeros through the loop —
                     the route such a tick had before the rows without vy, same device code
  Omni               the holonomic model, for scale
The three contexts are timed in turn, ROUNDS times over, so that a drift of the clocks meets all of
them.  Figures: the scoring-pass kernel by HIP events (SMPC_FLAG_PROFILE) and the wall time of a tick
with the events off, each as the median over all rounds, the median of every round and the spread of
the rounds' medians (largest minus smallest); then the difference of the two DiffDrive routes beside
the larger of their spreads, and that difference round by round (a round that a disturbance of the
host slows down slows all three contexts, which are timed one after the other within it)."""
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
ROUNDS, WARM, TIMED = 5, 20, 60
KNOB = "SMPC_NONHOLO_PASS"


def shift(u):
    return np.concatenate([u[:, 1:], u[:, -1:]], axis=1)


def kernel_name(g):
    f = g.lib.smpc_debug_last_pass_kernel
    f.restype, f.argtypes = ctypes.c_char_p, []
    return f().decode()


def make(B, T, model, knob):
    cr = default_critics()
    for n in ALL:
        sub = getattr(cr, n)
        sub.enabled = 1 if n in FIVE else 0
        sub.cost_power = 1
    scn = make_scenario(T)
    saved = os.environ.pop(KNOB, None)
    if knob:
        os.environ[KNOB] = knob          # (the knobs are read when the context is created)
    try:
        g = Smpc(default_config(batch_size=B, time_steps=T, motion_model=model, flags=A.SMPC_FLAG_PROFILE))
    finally:
        os.environ.pop(KNOB, None)
        if saved is not None:
            os.environ[KNOB] = saved
    g.set_critics(cr)
    g.set_costmap(scn.cells, scn.origin_x, scn.origin_y, scn.resolution, inscribed_radius=scn.inscribed_radius,
                  cost_scaling_factor=scn.cost_scaling_factor, inflation_radius=scn.inflation_radius)
    g.seed(1234)
    return g, scn


def rounds_of(values, n):
    return [float(np.median(values[i * n:(i + 1) * n])) for i in range(ROUNDS)]


def main():
    sizes = [tuple(int(v) for v in a.split("x")) for a in sys.argv[1:]] or \
        [(2097152, 64), (2097152, 56), (262144, 64), (61440, 64)]
    print(f"library: {LIB_PATH}")
    for B, T in sizes:
        ctxs = [("DiffDrive", *make(B, T, A.SMPC_MODEL_DIFF_DRIVE, None)),
                ("DiffDrive, omni", *make(B, T, A.SMPC_MODEL_DIFF_DRIVE, "omni")),
                ("Omni", *make(B, T, A.SMPC_MODEL_OMNI, None))]
        us = {label: scn.u0 for label, _, scn in ctxs}
        t0 = time.perf_counter()      # the clock warm-up: the workload's own ticks
        while (time.perf_counter() - t0) * 1e3 < CLOCK_WARMUP_MS:
            for label, g, scn in ctxs:
                un, _ = g.optimize(scn.tick, us[label])
                us[label] = shift(un)
        res = {label: {"pass": [], "wall": []} for label, _, _ in ctxs}
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
                info[label] = (out.pass_kind, kernel_name(g), out.passes)
                g.set_profile(False)
                t0 = time.perf_counter()
                for k in range(TIMED):
                    un, out = g.optimize(scn.tick, u)
                    u = shift(un)
                res[label]["wall"].append((time.perf_counter() - t0) / TIMED * 1e3)
                us[label] = u
        summary = {}
        for label, g, _ in ctxs:
            r = res[label]
            pr = [v * 1e3 for v in rounds_of(r["pass"], TIMED)]
            wr = [v * 1e3 for v in r["wall"]]
            summary[label] = (float(np.median(r["pass"])) * 1e3, max(pr) - min(pr), float(np.median(wr)), max(wr) - min(wr), pr, wr)
            print(f"{B}x{T} {label:16s}: scoring pass {summary[label][0]:8.1f} us (rounds {' '.join('%.1f' % v for v in pr)}; "
                  f"spread {summary[label][1]:.1f}), tick {summary[label][2]:8.1f} us (rounds {' '.join('%.1f' % v for v in wr)}; "
                  f"spread {summary[label][3]:.1f}), pass_kind {info[label][0]}, passes {info[label][2]}, {info[label][1]}",
                  flush=True)
            g.close()
        nh, om = summary["DiffDrive"], summary["DiffDrive, omni"]
        print(f"{B}x{T} omni - library route: scoring pass {om[0] - nh[0]:+.1f} us ({(om[0] - nh[0]) / om[0] * 100:+.1f} %; "
              f"larger spread {max(nh[1], om[1]):.1f}), tick {om[2] - nh[2]:+.1f} us ({(om[2] - nh[2]) / om[2] * 100:+.1f} %; "
              f"larger spread {max(nh[3], om[3]):.1f}); round by round: scoring pass "
              f"{' '.join('%+.1f' % (b - a) for a, b in zip(nh[4], om[4]))}, tick "
              f"{' '.join('%+.1f' % (b - a) for a, b in zip(nh[5], om[5]))}", flush=True)


if __name__ == "__main__":
    main()
