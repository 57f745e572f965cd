"""Moving obstacles without a GPU: the model on hand-made trajectories, the fleet's table function
against NumPy, the refusals that come before a handle is touched, and the seeds of the GPU test."""
import ctypes as C

import numpy as np
import pytest

from mpcholonavigation_amd import _abi as A
from tests import moving_model as mm
from tests import moving_scenes as ms
from tests.harness import lib  # noqa: F401

P = dict(collision_cost=100.0, repulsion_weight=4.0, margin=2.0)


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def straight(T=16, x0=0.0, step=0.125):
    """One rollout along +x: x[t] = x0 + step t, y = 0 (every value a short binary fraction)."""
    x = (x0 + step * np.arange(T, dtype=np.float64)).astype(np.float32)[None, :]
    return x, np.zeros_like(x)


def standing(T, cx, cy):
    xy = np.zeros((1, T, 2), np.float32)
    xy[0, :, 0], xy[0, :, 1] = cx, cy
    return xy


# ---- 1. the model ----------------------------------------------------------------------------------

def test_a_disc_out_of_reach_costs_exactly_nothing():
    x, y = straight()
    r = mm.costs(x, y, standing(16, 0.9375, 3.5), [1.0], **P)      # nearest 3.5 m > radius + margin = 3 m
    assert r.m[0] == 0.0 and not r.hit[0] and r.sum_q[0] == 0.0 and r.live[0] == 0


def test_a_straight_pass_through_the_margin_has_its_closed_form():
    # the disc stands on the line, 4 m ahead: d[t] = 4 - t / 8.  radius 1, margin 2: q = (3 - d) / 2 for
    # t = 9 .. 15, sum = (sum(t / 8) - 7) / 2 = (84 / 8 - 7) / 2 = 1.75; never closer than 2.125 m
    x, y = straight()
    r = mm.costs(x, y, standing(16, 4.0, 0.0), [1.0], **P)
    # (live: the seven terms and the one at d == radius + margin exactly, inside the widened reach)
    assert r.sum_q[0] == 1.75 and not r.hit[0] and r.live[0] == 8
    assert r.m[0] == 4.0 * 1.75 / 16


def test_a_hit_adds_the_collision_cost_once():
    # two discs on the line, both entered: 2.5 m and 3 m ahead, the rollout reaches 1.875 m + 1.5 m
    x, y = straight(x0=1.5)
    xy = np.concatenate([standing(16, 2.5, 0.0), standing(16, 3.0, 0.0)])
    r = mm.costs(x, y, xy, [0.5, 0.5], **P)
    one = [mm.costs(x, y, xy[k:k + 1], [0.5], **P) for k in range(2)]
    assert r.hit[0] and one[0].hit[0] and one[1].hit[0]
    assert r.sum_q[0] == one[0].sum_q[0] + one[1].sum_q[0]
    assert r.m[0] == 4.0 * r.sum_q[0] / 16 + 100.0                # once, not once per disc or per step
    # a second rollout that stays away: nothing of the first one's leaks into it
    x2 = np.concatenate([x, x - 10.0])
    r2 = mm.costs(x2, np.zeros_like(x2), xy, [0.5, 0.5], **P)
    assert r2.m[0] == r.m[0] and r2.m[1] == 0.0 and not r2.hit[1]


def test_q_saturates_at_one_and_the_boundary_is_strict():
    x, y = straight(T=4, step=0.0)                                # standing at the origin
    r = mm.costs(x, y, standing(4, 0.25, 0.0), [1.0], **P)        # deep inside: q = min((3 - 0.25) / 2, 1) = 1
    assert r.sum_q[0] == 4.0 and r.hit[0]
    r = mm.costs(x, y, standing(4, 1.0, 0.0), [1.0], **P)         # d == radius: no hit, q = 1
    assert not r.hit[0] and r.sum_q[0] == 4.0 and r.near[0]
    r = mm.costs(x, y, standing(4, 3.0, 0.0), [1.0], **P)         # d == radius + margin: q = 0
    assert r.m[0] == 0.0


# ---- 2. the fleet's table ----------------------------------------------------------------------------

def test_fleet_table_is_the_models():
    from mpcholonavigation_amd import host_optimizer as H
    n, T = 4, 56
    rng = np.random.default_rng(5)
    u = np.zeros((n, 3, T), np.float32)
    u[:, 0] = 0.3 + 0.05 * rng.standard_normal((n, T))
    u[:, 1] = 0.05 * rng.standard_normal((n, T))
    u[:, 2] = 0.4 * rng.standard_normal((n, T))
    pose = np.array([[1.0, 2.0, 0.0], [4.0, 2.0, np.pi], [2.5, 0.5, 1.2], [9.0, 9.0, -2.0]])
    state = np.array([H.FLEET_PEER_MOVING, H.FLEET_PEER_MOVING, H.FLEET_PEER_STANDING, H.FLEET_PEER_UNSEEN], np.uint8)
    dt = np.full(n, 0.05, np.float32)
    holo = np.array([1, 0, 1, 1], np.uint8)
    rr = np.array([0.25, 0.3, 0.2, 0.5], np.float32)
    for i in range(n):
        xy, radius = H.mutual_avoidance_table(i, state, pose, u, dt, holo, rr)
        want_xy, want_r = mm.fleet_table(i, state, pose, u, dt, holo, rr)
        others = [j for j in range(n) if j != i and state[j] != H.FLEET_PEER_UNSEEN]
        assert xy.shape == (len(others), T, 2) and np.array_equal(radius, want_r), i
        assert np.array_equal(radius, np.array([rr[i] + rr[j] for j in others], np.float32))
        for k, j in enumerate(others):
            if state[j] == H.FLEET_PEER_STANDING:
                assert np.array_equal(xy[k], want_xy[k]) and np.all(xy[k] == pose[j][:2].astype(np.float32)), (i, j)
            else:
                # (the C library's cosf / sinf against NumPy's float32 ones: an ulp of a term, T terms)
                assert np.max(np.abs(xy[k].astype(np.float64) - want_xy[k])) < 1e-6, (i, j)
                assert np.max(np.abs(xy[k][-1] - pose[j][:2])) > 0.3, (i, j)      # it moved
    # a non-holonomic member ignores its vy row
    u2 = u.copy()
    u2[1, 1] = 0.0
    assert np.array_equal(H.mutual_avoidance_table(0, state, pose, u2, dt, holo, rr)[0],
                          H.mutual_avoidance_table(0, state, pose, u, dt, holo, rr)[0])


# ---- 3. refusals ---------------------------------------------------------------------------------------

def test_symbols_bindings_and_refusals_before_the_handle(lib):
    from mpcholonavigation_amd import host_optimizer as H
    from mpcholonavigation_amd.optimizer import Smpc
    for name in ("smpc_set_moving_obstacles", "smpc_get_moving_obstacle_costs", "smpc_moving_obstacles_params_default"):
        assert hasattr(lib, name) and name in A.PROTOTYPES
    for m in ("set_moving_obstacles", "moving_obstacle_costs"):
        assert callable(getattr(Smpc, m)) and callable(getattr(H.Optimizer, m))
    assert callable(H.FleetOptimizer.set_mutual_avoidance)
    p = A.SmpcMovingObstaclesParams()
    lib.smpc_moving_obstacles_params_default(C.byref(p))
    assert p.collision_cost >= 0 and p.repulsion_weight >= 0 and p.margin > 0 and p.reserved == 0
    assert C.sizeof(p) == 16 and A.SMPC_MAX_MOVING_OBSTACLES == mm.MAX_OBSTACLES == 64
    xy, r = np.zeros((1, 8, 2), np.float32), np.ones(1, np.float32)
    assert lib.smpc_set_moving_obstacles(None, C.byref(p), ptr(xy), ptr(r), 1) == A.SMPC_ERR_INVALID
    assert lib.smpc_get_moving_obstacle_costs(None, None, None) == A.SMPC_ERR_INVALID
    host = H.load_fleet_library()
    f = host.sortham_optimizer_set_moving_obstacles
    fake = C.c_void_p(1)      # never dereferenced: the checks come first
    assert f(None, C.byref(p), ptr(xy), ptr(r), 1, 8) == A.SMPC_ERR_INVALID
    assert f(fake, None, ptr(xy), ptr(r), 1, 8) == A.SMPC_ERR_INVALID
    assert f(fake, C.byref(p), None, ptr(r), 1, 8) == A.SMPC_ERR_INVALID
    assert f(fake, C.byref(p), ptr(xy), None, 1, 8) == A.SMPC_ERR_INVALID
    assert f(fake, C.byref(p), ptr(xy), ptr(r), 1, 0) == A.SMPC_ERR_INVALID
    assert f(fake, C.byref(p), ptr(xy), ptr(r), A.SMPC_MAX_MOVING_OBSTACLES + 1, 8) == A.SMPC_ERR_UNSUPPORTED
    assert host.sortham_optimizer_moving_obstacle_costs(None, ptr(r), None, 1) == A.SMPC_ERR_INVALID
    assert host.sortham_fleet_set_mutual_avoidance(None, C.byref(p), ptr(r), 1) == A.SMPC_ERR_INVALID
    assert host.sortham_fleet_set_mutual_avoidance(fake, None, ptr(r), 1) == A.SMPC_ERR_INVALID
    assert host.sortham_fleet_avoidance_table(1, 1, 8, None, None, None, None, None, None, None, None, None) == A.SMPC_ERR_INVALID


# ---- 4. the seeds of the GPU test ----------------------------------------------------------------------

@pytest.mark.parametrize("B,T,flags,kind", ms.TERM_SHAPES)
@pytest.mark.parametrize("K", ms.TERM_K)
def test_the_term_cases_decide_something_and_stay_clear_of_the_boundary(B, T, flags, kind, K):
    r = ms.term_model(B, T, flags, K)
    near, hits, live = float(r.near.mean()), float(r.hit.mean()), float((r.sum_q > 0).mean())
    print(f"[moving] {B}x{T} K={K}: near {near:.4f}, hit {hits:.3f}, in reach {live:.3f}, max m {r.m.max():.3f}")
    assert near <= ms.NEAR_CAP
    assert live > 0.5 and 0.0 < hits < 1.0
