#!/usr/bin/env python3
"""Developer tool: GPU time of one smpc_critic_breakdown call, its scoring pass (smpc_pass_stats)
and its reduction (smpc_reduce_stats + smpc_reduce_stats_final) each by HIP events
(SMPC_FLAG_PROFILE, smpc_debug_stats_ms), next to the tick's own time on the same context.

    critic_stats_time.py [BxT:five|deployed ...]      default: 2000x56:deployed 2097152x64:five

A diagnostic call: there is no target for these numbers."""
import ctypes as C
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from mpcholonavigation_amd import _abi as A
from mpcholonavigation_amd.optimizer import Smpc
from mpcholonavigation_amd.synthetic import make_scenario
from mpcholonavigation_amd.tick import default_config, default_critics

LISTS = {"deployed": ("constraint", "cost", "goal", "goal_angle", "path_align", "path_follow", "path_angle",
                      "prefer_forward", "twirling"),
         "five": ("obstacles", "path_align", "path_follow", "goal_angle", "prefer_forward")}
ALL = ("obstacles", "path_align", "path_follow", "goal_angle", "prefer_forward", "cost", "goal", "constraint",
       "twirling", "path_angle", "velocity_deadband", "path_align_legacy")
CALLS = 20

for arg in sys.argv[1:] or ["2000x56:deployed", "2097152x64:five"]:
    size, which = arg.split(":")
    B, T = (int(v) for v in size.split("x"))
    cr = default_critics()
    for n in ALL:
        getattr(cr, n).enabled = 1 if n in LISTS[which] else 0
    scn = make_scenario(T)
    g = Smpc(default_config(batch_size=B, time_steps=T, flags=A.SMPC_FLAG_PROFILE))
    g.set_critics(cr)
    g.set_costmap(scn.cells, scn.origin_x, scn.origin_y, scn.resolution)
    g.seed(1)
    ms = g.lib.smpc_debug_stats_ms
    ms.restype, ms.argtypes = C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    u = scn.u0
    for _ in range(5):
        un, out = g.optimize(scn.tick, u)
        u = np.concatenate([un[:, 1:], un[:, -1:]], axis=1)
    st = g.critic_stats(scn.tick, u)            # (the first call allocates)
    ps, rs, wall = [], [], []
    for _ in range(CALLS):
        t0 = time.perf_counter()
        st = g.critic_stats(scn.tick, u)
        wall.append((time.perf_counter() - t0) * 1e3)
        a, b = C.c_float(0), C.c_float(0)
        ms(g.h, C.byref(a), C.byref(b))
        ps.append(a.value)
        rs.append(b.value)
    _, out = g.optimize(scn.tick, u)
    print(f"{B}x{T} {which}: breakdown call {np.median(wall):.3f} ms wall (min {min(wall):.3f}); scoring pass "
          f"{np.median(ps) * 1e3:.1f} us (min {min(ps) * 1e3:.1f}), reduction {np.median(rs) * 1e3:.1f} us (min {min(rs) * 1e3:.1f}); "
          f"the tick's own scoring pass {out.score_pass_ms * 1e3:.1f} us (pass_kind {out.pass_kind}); "
          f"effective samples {st.effective_samples:.1f} of {st.batch}, rows "
          f"{[n for n in st.names if st.scored(n)]}")
    g.close()
