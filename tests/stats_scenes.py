"""What the critic-statistics tests share (test_gpu_critic_stats.py, test_gpu_critic_stats_reach.py,
test_gpu_group_critic_stats.py): the rows of a breakdown, the critic list dressed so that every row
scores, the two scenes, and the float64 / float32 restatements the statistics are judged by."""
import math

import numpy as np

from mpcholonavigation_amd import _abi as A
from mpcholonavigation_amd.synthetic import wall_beside_path
from tests.harness import dressed_critics
from tests.helpers import configure, make_case

EPS = 2.0 ** -24
# the struct's sub-structs in the scoring order of smpc.h: row k of a breakdown
ORDER = ("constraint", "cost", "obstacles", "path_align", "path_align_legacy", "path_follow", "goal_angle",
         "prefer_forward", "goal", "path_angle", "twirling", "velocity_deadband")
CONTROL = A.SMPC_STATS_CONTROL
NO_FURTHEST = ("obstacles", "goal_angle", "prefer_forward")      # no critic that consumes the furthest point


def critics(names, power=1):
    """The list `names`, every critic with cost_power `power`, dressed (tests/harness.py); PathAlign
    and its legacy form on the same trajectory_point_step, their offset small enough for a 15-step
    horizon to reach, PathAngle's angle narrow enough for its gate to open."""
    return dressed_critics(names, power,
                           path_align__offset_from_furthest=3, path_align_legacy__offset_from_furthest=3,
                           path_align__trajectory_point_step=4, path_align_legacy__trajectory_point_step=4,
                           path_angle__max_angle_to_furthest=0.05)


def scene(B, T, kind, noise_seed=1234):
    """kind "wall": a cruise tick beside an inflated wall (the path-following gates open, the
    collision critics have something to score); "near": inside the goal thresholds (GoalAngle and
    Goal score, the path critics stand down)."""
    cfg, scn, noise = make_case(B, T, near_goal=(kind == "near"), noise_seed=noise_seed)
    if kind == "wall":
        scn.cells = wall_beside_path(scn)
        scn.tick.pose_yaw = 0.2      # heading off the plan: PathAngle's gate opens
    scn.tick.goal_checker_xy_tolerance = 0.25
    return cfg, scn, noise


def mask_of(names):
    return sum(1 << ORDER.index(n) for n in names) | 1 << CONTROL


def breakdown(Smpc, cfg, scn, noise, cr, tick=None):
    g = Smpc(cfg)
    configure(g, scn, critics=cr, noise=noise)
    st = g.critic_stats(tick or scn.tick, scn.u0, per_rollout=True)
    return g, st


def row_parity(row, ref, T, label):
    """tests.helpers.assert_parity's bar for per-rollout costs, on one row: no collision classified
    differently, at most max(1, 2e-5 B T) neighbouring-cell flips, everything else within 2e-4
    relative (absolute below 1) and never 0.5 apart."""
    d = np.abs(row.astype(np.float64) - ref.astype(np.float64))
    tight = d <= 2e-4 * np.maximum(np.abs(ref), 1.0)
    hard = int(np.sum(d > 100.0))
    soft = int(np.sum(~tight)) - hard
    print(f"[critic stats] {label}: max |d| {float(d.max()):.3e}, hard {hard} soft {soft}, |ref| max {float(np.abs(ref).max()):.3e}")
    assert hard == 0, f"{label}: {hard} collision flips"
    assert soft <= max(1, int(2e-5 * ref.size * T)), f"{label}: {soft} soft cell flips"
    assert float(d[d <= 100.0].max()) < 0.5, f"{label}: mismatch {float(d.max())}"


def k2_of(cfg):
    """-log2(e) / temperature as the library forms it, in float32."""
    return np.float32(np.float32(-1.0) / np.float32(cfg.temperature)) * np.float32(1.4426950408889634)


def check_statistics(st, costs, cfg):
    B = st.batch
    rows = st.per_rollout.astype(np.float64)
    c32 = costs.astype(np.float32)
    best = int(np.argmin(c32))                    # (the first of the least)
    assert st.best_rollout == best
    assert np.float32(st.best_cost) == c32[best]
    assert np.array_equal(st.min, st.per_rollout.min(axis=1))
    assert np.array_equal(st.max, st.per_rollout.max(axis=1))
    assert np.array_equal(st.at_best, st.per_rollout[:, best])
    # the weights: 2^(k2 (c - min)), the argument in float32 as the pass forms it
    w = np.exp2((k2_of(cfg) * (c32 - c32[best])).astype(np.float64))
    tol = math.log2(B) * EPS
    ref_sum = rows.sum(axis=1)
    assert np.all(np.abs(st.sum - ref_sum) <= tol * np.abs(rows).sum(axis=1))
    ref_w = rows @ w / w.sum()
    assert np.all(np.abs(st.weighted - ref_w) <= tol * (np.abs(rows) @ w / w.sum()))
    ess = w.sum() ** 2 / (w * w).sum()
    assert abs(st.effective_samples - ess) <= tol * ess
    assert 1.0 <= st.effective_samples <= B * (1 + tol)
    for k in range(13):
        if not st.scored_mask >> k & 1:
            assert st.sum[k] == st.min[k] == st.max[k] == st.weighted[k] == st.at_best[k] == 0.0
    return ess


def slices_of(B):
    """(number of slices, slice length) of the reduction, as stats_reduce_slices cuts the batch:
    16 384 rollouts a slice, doubled until at most 1024 slices remain."""
    n = 16384
    while -(-B // n) > 1024:
        n *= 2
    return -(-B // n), n


def sliced_float32_statistics(rows, costs, cfg):
    """The reduction's arithmetic restated in NumPy, slice by slice: the weights 2^(k2 (c - m_s))
    against the SLICE's least cost m_s, the argument and the weight in float32 (exp2 correctly
    rounded, which the hardware's v_exp_f32 is not), the sums in double, every slice multiplied by
    the float32 factor 2^(k2 (m_s - m)) in slice order.  -> (weighted float64 [13],
    effective_samples).  What a result beyond check_statistics' bar is compared with to tell a
    defect of the kernels from the error of the device's exponent (test_gpu_critic_stats_reach.py)."""
    c32 = np.asarray(costs, np.float32)
    k2, m = k2_of(cfg), c32.min()
    S, n = slices_of(len(c32))
    W = W2 = 0.0
    Aw = np.zeros(rows.shape[0])
    for s in range(S):
        c = c32[s * n:(s + 1) * n]
        ms = c.min()
        w = np.exp2((k2 * (c - ms)).astype(np.float64)).astype(np.float32).astype(np.float64)
        f = float(np.float32(np.exp2(np.float64(k2 * (ms - m)))))
        W += f * w.sum()
        W2 += f * f * (w * w).sum()
        Aw += f * (rows[:, s * n:(s + 1) * n].astype(np.float64) @ w)
    return Aw / W, W * W / W2


def statistics_ratios(st, costs, cfg, other=None):
    """Error / bar of `weighted` (the largest over the rows) and of `effective_samples` under
    check_statistics' model and bar, log2(B) 2^-24 relative to the absolute sums.  other:
    (weighted, effective_samples) to judge in place of the device's (the float32 restatement)."""
    rows = st.per_rollout.astype(np.float64)
    c32 = costs.astype(np.float32)
    w = np.exp2((k2_of(cfg) * (c32 - c32.min())).astype(np.float64))
    tol = math.log2(st.batch) * EPS
    weighted, ess_dev = (st.weighted, st.effective_samples) if other is None else other
    bar = tol * (np.abs(rows) @ w / w.sum())
    err = np.abs(np.asarray(weighted, np.float64) - rows @ w / w.sum())
    ess = w.sum() ** 2 / (w * w).sum()
    return float((err[bar > 0] / bar[bar > 0]).max()), float(abs(ess_dev - ess) / (tol * ess))

