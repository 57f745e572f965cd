"""Moving obstacles: the definition of smpc_set_moving_obstacles (include/smpc.h) in NumPy.

K discs, disc k with its centre at xy[k, t] when the robot is at trajectory point t and with the
centre-to-centre collision distance radius[k].  For rollout b with the trajectory points
(x[b, t], y[b, t]) the scoring passes form (float32):

    d(b,t,k) = sqrtf(dx*dx + dy*dy)                      float32, every product and sum rounded
    q(b,t,k) = clamp((radius[k] + margin - d) / margin, 0, 1)
    hit(b)   = any over t, k of d < radius[k]
    m(b)     = repulsion_weight * (sum over t, k of q) / T + (hit(b) ? collision_cost : 0)

d is formed as the device forms it, in float32 (so that `d < radius` and `d < radius + margin`
decide the same way on the same trajectory points); q, the sum and m are float64: the yardstick
for the device's float32 sums.  The model knows nothing of how the trajectory points were made:
the tests hand it the oracle's, or hand-made ones.
"""
from types import SimpleNamespace

import numpy as np

EPS = 2.0 ** -24
MAX_OBSTACLES = 64
NEAR = 1e-5            # |d - radius| below this at some step: the rollout's hit may go either way
TRAJ_BOUND = 2e-6      # per-coordinate bound of the device's trajectory points against the oracle's
                       # (tests/test_gpu_parity.py::test_rollout_trajectories_match)


def costs(x, y, xy, radius, collision_cost, repulsion_weight, margin):
    """x, y float32 [B, T]; xy [K, T, 2]; radius [K].  -> namespace(m float64 [B], hit bool [B],
    sum_q float64 [B], live int [B] (terms within reach, the reach widened by the trajectory bound),
    near bool [B], d_max float: the largest distance of a live term)."""
    x = np.ascontiguousarray(x, np.float32)
    y = np.ascontiguousarray(y, np.float32)
    xy = np.asarray(xy, np.float32)
    radius = np.asarray(radius, np.float32)
    B, T = x.shape
    K = len(radius)
    assert xy.shape == (K, T, 2) and 0 <= K <= MAX_OBSTACLES
    mg32 = np.float32(margin)
    sum_q = np.zeros(B, np.float64)
    hit = np.zeros(B, bool)
    near = np.zeros(B, bool)
    live = np.zeros(B, np.int64)
    d_max = 0.0
    for k in range(K):
        dx = x - xy[k, :, 0][None, :]
        dy = y - xy[k, :, 1][None, :]
        d = np.sqrt(dx * dx + dy * dy)            # float32 throughout
        assert d.dtype == np.float32
        reach = radius[k] + mg32                  # float32, as the host forms it
        q = np.clip((np.float64(reach) - d.astype(np.float64)) / np.float64(mg32), 0.0, 1.0)
        sum_q += q.sum(axis=1)
        hit |= (d < radius[k]).any(axis=1)
        near |= (np.abs(d.astype(np.float64) - np.float64(radius[k])) < NEAR).any(axis=1)
        inside = d.astype(np.float64) < np.float64(reach) + 2.0 * TRAJ_BOUND
        live += inside.sum(axis=1)
        if inside.any():
            d_max = max(d_max, float(d[inside].max()))
    m = np.float64(np.float32(repulsion_weight)) * sum_q / T + np.where(hit, np.float64(np.float32(collision_cost)), 0.0)
    return SimpleNamespace(m=m, hit=hit, sum_q=sum_q, live=live, near=near, d_max=d_max)


def tolerance(r, T, K, repulsion_weight, margin):
    """What a float32 evaluation of m on trajectory points within TRAJ_BOUND per coordinate of the
    model's may differ by, per rollout (float64 [B]), for the rollouts whose hit agrees:
      - every live term: its distance moves by at most sqrt(2) TRAJ_BOUND (the two coordinates) plus
        the float32 roundings of the two products, the sum and the square root on either side
        (4 EPS d each side), its q by that over margin plus the rounding of the subtraction and the
        quotient (2 EPS, q <= 1): times repulsion_weight / T;
      - the float32 sum of T K terms, in any order: (T K + 1) EPS sum|q|, times repulsion_weight / T;
      - the last rounding to float32: EPS |m|."""
    eps_d = np.sqrt(2.0) * TRAJ_BOUND + 8.0 * EPS * r.d_max
    per_term = eps_d / margin + 2.0 * EPS
    return (repulsion_weight / T) * (r.live * per_term + (T * K + 1) * EPS * r.sum_q) + EPS * np.abs(r.m)


def make_discs(tick, T, dt, K, seed, ahead=(0.15, 1.1), side=0.35, speed=0.25, radius=(0.12, 0.3)):
    """K discs across the nominal path of a robot at the tick's pose heading along +x of its own
    frame: disc k starts `ahead` metres in front and up to `side` metres beside the path and moves
    with a constant velocity of up to `speed` m/s.  -> (xy float32 [K, T, 2], radius float32 [K])."""
    rng = np.random.default_rng(seed)
    c, s = np.cos(tick.pose_yaw), np.sin(tick.pose_yaw)
    t = np.arange(1, T + 1, dtype=np.float64) * dt
    xy = np.zeros((K, T, 2), np.float64)
    for k in range(K):
        a0 = rng.uniform(*ahead)
        b0 = rng.uniform(-side, side)
        va, vb = rng.uniform(-speed, speed, 2)
        a, b = a0 + va * t, b0 + vb * t
        xy[k, :, 0] = tick.pose_x + c * a - s * b
        xy[k, :, 1] = tick.pose_y + s * a + c * b
    return xy.astype(np.float32), rng.uniform(radius[0], radius[1], K).astype(np.float32)


def far_discs(tick, T, K, distance=50.0):
    """K discs standing `distance` metres from the pose: out of every rollout's reach."""
    xy = np.zeros((K, T, 2), np.float32)
    ang = np.linspace(0.0, 2.0 * np.pi, K, endpoint=False)
    xy[:, :, 0] = (tick.pose_x + distance * np.cos(ang))[:, None]
    xy[:, :, 1] = (tick.pose_y + distance * np.sin(ang))[:, None]
    return xy, np.full(K, 0.3, np.float32)


def integrate(u, pose, dt, holonomic=True):
    """Optimizer::getOptimizedTrajectory / integrateControlSequence: the control sequence u float32
    [3, T] itself integrated from pose (x, y, yaw), float32 cumulative sums, x = (float)(x0 +
    (double)sum), libm float sin and cos.  -> float32 [T, 3] x, y, yaw."""
    u = np.asarray(u, np.float32)
    T = u.shape[1]
    dt = np.float32(dt)
    yaw0 = np.float32(pose[2])
    yaws = np.zeros(T, np.float32)
    acc = np.float32(0)
    for t in range(T):
        inc = np.float32(u[2, t] * dt)
        acc = inc if t == 0 else np.float32(acc + inc)
        yaws[t] = np.float32(acc + yaw0)
    out = np.zeros((T, 3), np.float32)
    ax = ay = np.float32(0)
    for t in range(T):
        a = yaw0 if t == 0 else yaws[t - 1]
        c, s = np.cos(a, dtype=np.float32), np.sin(a, dtype=np.float32)
        dx, dy = np.float32(u[0, t] * c), np.float32(u[0, t] * s)
        if holonomic:
            dx = np.float32(dx - np.float32(u[1, t] * s))
            dy = np.float32(dy + np.float32(u[1, t] * c))
        ax = np.float32(dx * dt) if t == 0 else np.float32(ax + np.float32(dx * dt))
        ay = np.float32(dy * dt) if t == 0 else np.float32(ay + np.float32(dy * dt))
        out[t] = (np.float32(pose[0] + np.float64(ax)), np.float32(pose[1] + np.float64(ay)), yaws[t])
    return out


def fleet_table(i, state, pose, u, dt, holonomic, robot_radius):
    """FleetOptimizer's table for member i: one disc per other member j that has been seen (state
    1: standing at pose[j]; 2: integrate(u[j]) from pose[j]), radius r_i + r_j in float32.
    -> (xy float32 [discs, T, 2], radius float32 [discs])."""
    n, T = len(state), np.asarray(u).shape[2]
    xy, radius = [], []
    r = np.asarray(robot_radius, np.float32)
    for j in range(n):
        if j == i or state[j] == 0:
            continue
        radius.append(np.float32(r[i] + r[j]))
        if state[j] == 2:
            xy.append(integrate(u[j], pose[j], dt[j], bool(holonomic[j]))[:, :2])
        else:
            xy.append(np.tile(np.array(pose[j][:2], np.float64).astype(np.float32), (T, 1)))
    if not xy:
        return np.zeros((0, T, 2), np.float32), np.zeros(0, np.float32)
    return np.stack(xy).astype(np.float32), np.array(radius, np.float32)
