"""The trajectory validator without a GPU: symbols and bindings, defaults and the refusals that come
before a handle is touched, the number of poses checked, the model (tests/validate_model.py) on
hand-made cases, and the premises of the cases the GPU test runs (tests/validate_scenes.py), asserted
on the model alone."""
import ctypes as C

import numpy as np
import pytest

from mpcholonavigation_amd import _abi as A
from tests import footprint_walk_model as W
from tests import moving_model as MM
from tests import validate_model as V
from tests import validate_scenes as S
from tests.harness import lib  # noqa: F401


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


# ---- 1. symbols, defaults, refusals --------------------------------------------------------------------

NAMES = ("smpc_validation_params_default", "smpc_validate_trajectory", "smpc_group_validate_trajectories",
         "smpc_group_validation_counts")


def test_symbols_are_exported_and_bound(lib):
    from mpcholonavigation_amd.optimizer import Smpc, SmpcGroup
    for name in NAMES:
        assert hasattr(lib, name) and name in A.PROTOTYPES, name
    assert callable(Smpc.validate_trajectory)
    assert callable(SmpcGroup.validate_trajectories) and callable(SmpcGroup.validation_counts)
    assert lib.smpc_abi_version() == 3
    assert C.sizeof(A.SmpcValidationParams) == 16 and C.sizeof(A.SmpcValidation) == 24
    assert (A.SMPC_VALIDATION_CAUSE_COSTMAP, A.SMPC_VALIDATION_CAUSE_DISC) == (V.CAUSE_COSTMAP, V.CAUSE_DISC) == (1, 2)


def test_defaults_and_refusals_before_the_handle(lib):
    p = A.SmpcValidationParams(9.0, 9, 9, 9)
    lib.smpc_validation_params_default(C.byref(p))
    assert (p.collision_lookahead_time, p.consider_footprint, p.moving_obstacles, p.reserved) == (2.0, 0, 1, 0)
    lib.smpc_validation_params_default(None)          # a null pointer is left alone
    u = np.zeros((3, 8), np.float32)
    out = A.SmpcValidation()
    assert lib.smpc_validate_trajectory(None, C.byref(p), 0.0, 0.0, 0.0, ptr(u), C.byref(out), None) == A.SMPC_ERR_INVALID
    n = 2
    params = (A.SmpcValidationParams * n)()
    poses = (C.c_double * (3 * n))()
    us = (C.c_void_p * n)(u.ctypes.data, u.ctypes.data)
    outs = (A.SmpcValidation * n)()
    status = (C.c_int32 * n)()
    assert lib.smpc_group_validate_trajectories(None, params, poses, us, None, outs, None, status) == A.SMPC_ERR_INVALID
    a, b = C.c_uint64(7), C.c_uint64(7)
    assert lib.smpc_group_validation_counts(None, C.byref(a), C.byref(b)) == A.SMPC_ERR_INVALID
    assert (a.value, b.value) == (7, 7)


def test_host_faces_are_exported_and_refuse_a_null_handle(lib):
    from mpcholonavigation_amd import host_optimizer as H
    host = H.load_fleet_library()
    for name in ("sortham_optimizer_set_trajectory_validation", "sortham_optimizer_last_validation",
                 "sortham_fleet_validation_counts"):
        assert hasattr(host, name), name
    for m in ("set_trajectory_validation", "last_validation"):
        assert callable(getattr(H.Optimizer, m)) and callable(getattr(H.FleetOptimizer, m))
    assert callable(H.FleetOptimizer.validation_counts)
    p = A.SmpcValidationParams()
    lib.smpc_validation_params_default(C.byref(p))
    assert host.sortham_optimizer_set_trajectory_validation(None, C.byref(p)) == A.SMPC_ERR_INVALID
    v, a, b = A.SmpcValidation(), C.c_uint64(0), C.c_uint64(0)
    assert host.sortham_optimizer_last_validation(None, C.byref(v), C.byref(a), C.byref(b)) == A.SMPC_ERR_INVALID
    assert host.sortham_fleet_validation_counts(None, C.byref(a), C.byref(b)) == A.SMPC_ERR_INVALID


# ---- 2. the poses checked ----------------------------------------------------------------------------

@pytest.mark.parametrize("lookahead,dt,T,n", [
    (2.0, 0.05, 56, 40),          # 40 in float, 39 in double
    (1.0, 0.1, 56, 10),
    (2.0, 0.05, 30, 30),          # beyond the horizon: T
    (1.0e3, 0.0625, 256, 256),
    (0.04, 0.05, 56, 0),          # below one step
    (0.05, 0.05, 56, 1),
])
def test_poses_checked(lookahead, dt, T, n):
    assert V.checked(lookahead, dt, T) == n


def test_the_quotient_is_formed_in_float():
    # the float model_dt 0.05f is a little above 0.05: its quotient in double falls short of 40
    assert int(np.floor(np.float64(np.float32(2.0)) / np.float64(np.float32(0.05)))) == 39
    assert V.checked(2.0, 0.05, 100) == 40


# ---- 3. the model on hand-made cases -----------------------------------------------------------------

def straight(T, x0, y0=0.0, step=0.05):
    p = np.zeros((T, 3), np.float32)
    p[:, 0] = (x0 + step * np.arange(T)).astype(np.float32)
    p[:, 1] = y0
    return p


def small_scene(value=254, track_unknown=False):
    scn = S.wall_scene(value=value, thickness=2, track_unknown=track_unknown)
    return scn          # the band covers x in [2.0, 2.1)


def test_model_first_collision_and_the_lookahead():
    scn = small_scene()
    p = straight(16, 1.825)                  # cell centres: 1.825 + 0.05 t; inside the band at t = 4, 5
    v = V.verdict(scn, p, 16)
    assert (v.valid, v.first_bad, v.cause, v.cost, v.disc, v.checked) == (0, 4, 1, 254.0, 0, 16)
    assert list(np.flatnonzero(v.bad_all)) == [4, 5]
    assert V.verdict(scn, p, 4).valid == 1 and V.verdict(scn, p, 5).first_bad == 4
    v0 = V.verdict(scn, p, 0)
    assert (v0.valid, v0.checked, v0.first_bad, v0.cause, v0.cost) == (1, 0, 0, 0, 0.0)


def test_model_cost_classes():
    p = straight(16, 1.825)
    assert V.verdict(small_scene(253), p, 16).cost == 253.0
    assert V.verdict(small_scene(255), p, 16).cost == 255.0
    assert V.verdict(small_scene(255, track_unknown=True), p, 16).valid == 1
    assert V.verdict(small_scene(200), p, 16).valid == 1
    # off the map counts as 255
    off = straight(8, 4.8)
    v = V.verdict(small_scene(), off, 8)
    assert (v.valid, v.cause, v.cost) == (0, 1, 255.0) and v.first_bad == 4     # 4.8 + 0.05 * 4 = 5.0: the first x off the map


def test_model_footprint_rule():
    scn = S.wall_scene(value=253, thickness=2, footprint="rectangle")
    p = straight(16, 1.825)
    assert V.verdict(scn, p, 16, consider_footprint=False).first_bad == 4
    assert V.verdict(scn, p, 16, consider_footprint=True).valid == 1          # 253 does not collide under a footprint
    lethal = S.wall_scene(value=254, thickness=2, footprint="rectangle")
    # a free centre is free whatever lies under the outline; a centre at or above the possibly-inscribed cost is walked
    assert V.verdict(lethal, p, 16, consider_footprint=True).first_bad == 4
    pic = W.circumscribed_cost(lethal)
    assert 1 <= pic < 100
    lethal.cells[:, 130:140] = 100           # x in [1.5, 2.0): a walked field in front of the band
    v = V.verdict(lethal, p, 16, consider_footprint=True)
    assert (v.first_bad, v.cost) == (0, 254.0)      # the outline's front, 0.25 m ahead of 1.825 m, is in the band


def test_model_discs():
    scn = S.wall_scene(thickness=0)
    p = straight(16, 0.0, step=0.125)
    xy = np.zeros((3, 16, 2), np.float32)
    xy[0, :, 0], xy[1, :, 0], xy[2, :, 0] = 1.0, 0.5, 0.5
    xy[0, :, 1] = xy[1, :, 1] = 0.0625
    xy[2, :, 1] = 5.0
    r = np.array([0.25, 0.125, 1.0], np.float32)
    v = V.verdict(scn, p, 16, xy=xy, radius=r)
    # disc 1 at x = 0.5: d = hypot(0.5 - 0.125 t, 0.0625) < 0.125 at t = 4 alone; disc 0 from t = 7 on
    assert (v.valid, v.first_bad, v.cause, v.disc, v.cost) == (0, 4, 2, 1, 0.0)
    assert V.verdict(scn, p, 4, xy=xy, radius=r).valid == 1
    # the boundary is strict, and the model says when a term is near it
    xy[:, :, 1] = 0.0
    edge = V.verdict(scn, p, 4, xy=xy[1:2], radius=np.array([0.125], np.float32))       # t = 3: d == radius
    assert edge.valid == 1 and edge.near
    # the costmap wins at the same step, and the disc hit there is still reported
    wall = small_scene()
    q = straight(16, 1.825)
    d = np.zeros((2, 16, 2), np.float32)
    d[0, :, 0], d[1, :, 0] = 9.0, q[4, 0]
    v = V.verdict(wall, q, 16, xy=d, radius=np.array([0.01, 0.01], np.float32))
    assert (v.first_bad, v.cause, v.disc, v.cost) == (4, 1, 1, 254.0)


def test_model_end_to_end_ignores_vy_for_a_non_holonomic_model():
    scn = small_scene()
    u = np.zeros((3, 16), np.float32)
    u[0], u[1] = 0.5, 0.25
    v_h, p_h = V.validate(scn, (1.8, 0.0, 0.0), u, 0.05, 2.0)
    v_n, p_n = V.validate(scn, (1.8, 0.0, 0.0), u, 0.05, 2.0, holonomic=False)
    assert np.all(p_n[:, 1] == 0.0) and p_h[-1, 1] > 0.15 and np.array_equal(p_h[:, 0], p_n[:, 0])
    assert v_h.first_bad == v_n.first_bad == 7           # 1.8 + 0.025 (t + 1) >= 2.0


# ---- 4. the premises of the GPU test's cases -----------------------------------------------------------

@pytest.mark.parametrize("case", S.wall_cases(), ids=lambda c: c.name)
def test_wall_case_premises(case):
    v, poses = case.model()
    e = case.expect
    assert not v.near, "a disc term within moving_model.NEAR of its radius"
    for f in ("valid", "cause", "first_bad", "checked", "disc"):
        if f in e:
            assert getattr(v, f) == e[f], (f, getattr(v, f))
    if "cost" in e:
        assert v.cost == e["cost"]
    full = V.verdict(case.scn, poses, case.T, case.consider_footprint,
                     *((case.xy, case.radius) if case.moving_obstacles else (None, None)))
    if e.get("single"):
        assert full.bad_all.sum() == 1
    if e.get("several"):
        assert full.bad_all.sum() > 3
    if "sees" in e:         # the pose does meet that cost, and it is no collision here
        c, _ = V.costmap_costs(case.scn, poses, case.consider_footprint)
        assert (c == e["sees"]).any()
    if e.get("vertex_off"):
        wx, wy = W.vertices(case.scn, *(poses[v.first_bad:v.first_bad + 1, k] for k in range(3)))
        assert not W.vertex_cells(case.scn, wx, wy)[2].all()
        centre, on, _, _ = S.E.lookups(case.scn, poses[:, 0], poses[:, 1])
        assert on[v.first_bad] and centre[v.first_bad] == 100
    if e.get("disc_hits_there"):
        hit, _ = V.disc_hits(poses, case.xy, case.radius)
        assert hit[v.first_bad].any() and not hit[:v.first_bad].any()
    if e.get("vy_matters"):
        other = MM.integrate(case.u, case.pose, case.dt, True)
        assert np.max(np.abs(other[:, 1] - poses[:, 1])) > 0.1
    if case.name.startswith("wall-T") and case.T > 1:
        assert 0 < v.first_bad < case.T - 1


def test_wall_cases_cover_every_shape_and_disc_count():
    cases = S.wall_cases()
    assert {c.T for c in cases} >= set(S.SHAPES)
    counts = {0 if c.xy is None else len(c.radius) for c in cases}
    assert {0, 1, 64} <= counts
    assert any(not c.moving_obstacles and c.xy is not None for c in cases)
    assert any(not c.holonomic and np.abs(c.u[1]).max() > 0 for c in cases)


def test_walk_cases_decide_something():
    cases = S.walk_cases()
    res = {c.name: c.model()[0] for c in cases}
    fp = [c for c in cases if c.consider_footprint]
    assert {len(c.scn.footprint) for c in fp} >= {3, 4, 16}
    assert {c.T for c in cases} >= {1, 15, 56, 64, 65, 256}
    bad = [c for c in fp if not res[c.name].valid]
    assert len(bad) >= 10 and any(res[c.name].valid for c in fp)
    assert any(res[c.name].first_bad == 0 for c in bad)
    # the footprint decides: somewhere the point verdict and the footprint verdict differ
    assert any(not V.same(res[c.name], res[c.name + "-point"]) for c in fp)
    # a vertex off the map ends a rollout somewhere
    off = 0
    for c in bad:
        v, poses = c.model()
        wx, wy = W.vertices(c.scn, *(poses[v.first_bad:v.first_bad + 1, k] for k in range(3)))
        off += int(not W.vertex_cells(c.scn, wx, wy)[2].all())
    assert off > 0
    costs = {res[c.name].cost for c in cases if not res[c.name].valid}
    assert 254.0 in costs and 255.0 in costs
