"""The trajectory validator on the GPU (smpc_validate_trajectory, smpc_group_validate_trajectories):
exact verdicts against the integer model on the poses the call returned, the poses against the
host's integration, an independent judge (the oracle's CostCritic alone), that a validation changes
nothing a tick depends on, and the group call against ungrouped twins.  The cases and their premises:
tests/validate_scenes.py, tests/test_validate_cpu.py."""
import ctypes as C

import numpy as np
import pytest

from mpcholonavigation_amd import _abi as A
from mpcholonavigation_amd.synthetic import make_scenario
from mpcholonavigation_amd.tick import Tick, default_config, default_critics
from tests import harness as H
from tests import moving_model as MM
from tests import validate_model as V
from tests import validate_scenes as S
from tests.harness import Oracle, Smpc, mod  # noqa: F401
from tests.helpers import configure

pytestmark = pytest.mark.gpu

FIELDS = ("valid", "checked", "first_bad", "cause", "disc", "cost")


@pytest.fixture(scope="module")
def contexts(Smpc):
    """One context per (scene, horizon, model_dt, motion model), its costmap and footprint set once."""
    made = {}

    def get(case):
        k = case.key()
        if k not in made:
            made[k] = Smpc(case.config())
            made[k].set_critics(default_critics())
        S.configure(made[k], case)
        return made[k]
    yield get
    H.close(*made.values())


def run(g, case, poses=True):
    return g.validate_trajectory(case.pose, case.u, collision_lookahead_time=case.lookahead,
                                 consider_footprint=case.consider_footprint, moving_obstacles=case.moving_obstacles,
                                 poses=poses)


# ---- exact verdicts and the poses ----------------------------------------------------------------------

@pytest.mark.parametrize("case", S.all_cases(), ids=lambda c: c.name)
def test_verdict_is_the_models_on_the_returned_poses(contexts, case):
    got = run(contexts(case), case)
    n = V.checked(case.lookahead, case.dt, case.T)
    table = (case.xy, case.radius) if case.moving_obstacles else (None, None)
    want = V.verdict(case.scn, got.xyyaw, n, case.consider_footprint, *table)
    assert not want.near, "a disc term within moving_model.NEAR of its radius"
    print(f"[validate] {case.name}: " + ", ".join(f"{f} {getattr(got, f)}" for f in FIELDS))
    for f in FIELDS:
        assert getattr(got, f) == getattr(want, f), (f, getattr(got, f), getattr(want, f))
    # ... and the same verdict as the definition end to end (its own poses)
    full, poses = case.model()
    assert V.same(full, want)
    err = np.max(np.abs(got.xyyaw.astype(np.float64) - poses.astype(np.float64)), axis=0)
    print(f"[validate] {case.name}: poses off by {err[0]:.2e} {err[1]:.2e} {err[2]:.2e} (bound {MM.TRAJ_BOUND:.0e})")
    assert err.max() <= MM.TRAJ_BOUND


def test_poses_are_optional_and_the_same_verdict(contexts):
    case = S.case_named("wall-T56")
    g = contexts(case)
    a, b = run(g, case, poses=False), run(g, case, poses=True)
    assert a.xyyaw is None and all(getattr(a, f) == getattr(b, f) for f in FIELDS)


# ---- refusals ------------------------------------------------------------------------------------------

def test_refusals(Smpc, mod):
    case = S.case_named("wall-T15")
    g = Smpc(case.config())
    with pytest.raises(mod.SmpcError) as e:
        run(g, case)                                   # no costmap yet
    assert e.value.code == A.SMPC_ERR_STATE
    S.configure(g, case)
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(mod.SmpcError) as e:
            g.validate_trajectory(case.pose, case.u, collision_lookahead_time=bad)
        assert e.value.code == A.SMPC_ERR_INVALID
    with pytest.raises(mod.SmpcError) as e:
        g.validate_trajectory(case.pose, case.u, consider_footprint=True)     # no footprint set
    assert e.value.code == A.SMPC_ERR_STATE
    out = A.SmpcValidation()
    p = mod.validation_params(g.lib)
    assert g.lib.smpc_validate_trajectory(g.h, C.byref(p), 0.0, 0.0, 0.0, None, C.byref(out), None) == A.SMPC_ERR_INVALID
    assert g.lib.smpc_validate_trajectory(g.h, None, 0.0, 0.0, 0.0, case.u.ctypes.data, C.byref(out), None) == A.SMPC_ERR_INVALID
    assert g.lib.smpc_validate_trajectory(g.h, C.byref(p), 0.0, 0.0, 0.0, case.u.ctypes.data, None, None) == A.SMPC_ERR_INVALID
    assert run(g, case).valid == 0                     # and the context is none the worse
    grp = mod.SmpcGroup([g])
    with pytest.raises(mod.SmpcError) as e:
        run(g, case)                                   # a member of a group
    assert e.value.code == A.SMPC_ERR_STATE
    H.close(grp, g)


# ---- an independent judge --------------------------------------------------------------------------------

@pytest.mark.parametrize("case", S.judge_cases(), ids=lambda c: c.name)
def test_verdict_is_the_oracles_cost_critic(contexts, Oracle, case):
    got = run(contexts(case), case, poses=False)
    cfg = default_config(batch_size=1, time_steps=case.T, model_dt=case.dt, gamma=0.0, vx_max=100.0, vx_min=-100.0,
                         vy_max=100.0, wz_max=100.0)
    o = Oracle(cfg)
    s = case.scn
    o.set_critics(H.critics_of(("cost",), power=None, footprint=("cost",) if case.consider_footprint else ()))
    o.set_costmap(s.cells, s.origin_x, s.origin_y, s.resolution, track_unknown=s.track_unknown,
                  inscribed_radius=s.inscribed_radius, cost_scaling_factor=s.cost_scaling_factor,
                  inflation_radius=s.inflation_radius)
    if case.consider_footprint:
        o.set_footprint(s.footprint, s.circumscribed, s.layer_scaling)
    zero = np.zeros((1, case.T), np.float32)
    o.set_noise(zero, zero, zero)
    u = case.u
    px = (case.pose[0] + 0.05 * np.arange(20)).astype(np.float32)
    tick = Tick(pose_x=case.pose[0], pose_y=case.pose[1], pose_yaw=case.pose[2],
                speed=(float(u[0, 0]), float(u[1, 0]), float(u[2, 0])), path_x=px,
                path_y=np.full(20, case.pose[1], np.float32), path_yaw=np.zeros(20, np.float32),
                goal_x=float(px[-1]), goal_y=float(case.pose[1]))
    _, out = o.optimize(tick, H.shifted(u))
    o.close()
    print(f"[validate] {case.name}: oracle non_colliding {out.non_colliding}, valid {got.valid}")
    assert int(out.non_colliding) == int(got.valid)


# ---- changes nothing -------------------------------------------------------------------------------------

def _ticking(Smpc, seed, T=56, B=64, n=1):
    gs = []
    for i in range(n):
        g = Smpc(default_config(batch_size=B, time_steps=T))
        scn = make_scenario(T, seed=42 + i)
        configure(g, scn)
        g.seed(seed + i)
        gs.append((g, scn))
    return gs


def test_a_validation_between_ticks_changes_nothing(Smpc):
    (a, scn), (b, _) = _ticking(Smpc, 5)[0], _ticking(Smpc, 5)[0]
    xy, r = MM.make_discs(scn.tick, 56, 0.05, 3, seed=1)
    ua = ub = scn.u0
    for k in range(4):
        tick = H.moved(scn.tick, 0.01 * k)
        for g in (a, b):
            g.set_moving_obstacles(xy, r)
        v = b.validate_trajectory((tick.pose_x, tick.pose_y, tick.pose_yaw), ub, poses=True)
        assert v.checked == 40
        (ua, oa), (ub, ob) = a.optimize(tick, ua), b.optimize(tick, ub)
        b.validate_trajectory((tick.pose_x, tick.pose_y, tick.pose_yaw), ub, collision_lookahead_time=0.3)
        assert np.array_equal(H.bits(ua), H.bits(ub)), k
        assert np.array_equal(H.bits(a.get_costs()), H.bits(b.get_costs())), k
        for f in H.OUT_FIELDS:
            assert getattr(oa, f) == getattr(ob, f), (k, f)
        ua, ub = H.shifted(ua), H.shifted(ub)
    H.close(a, b)


def test_a_grouped_validation_between_rounds_changes_nothing(Smpc, mod):
    n = 3
    A_, B_ = _ticking(Smpc, 9, n=n), _ticking(Smpc, 9, n=n)
    ga, gb = mod.SmpcGroup([g for g, _ in A_]), mod.SmpcGroup([g for g, _ in B_])
    ua = [s.u0 for _, s in A_]
    ub = [s.u0 for _, s in B_]
    for k in range(4):
        ticks = [H.moved(s.tick, 0.01 * k) for _, s in A_]
        poses = [(t.pose_x, t.pose_y, t.pose_yaw) for t in ticks]
        gb.validate_trajectories(poses, ub)
        ra, rb = ga.optimize(ticks, ua), gb.optimize(ticks, ub)
        gb.validate_trajectories(poses, [u for u, _ in rb], take=[1, 0, 1])
        for i in range(n):
            assert np.array_equal(H.bits(ra[i][0]), H.bits(rb[i][0])), (k, i)
            assert np.array_equal(H.bits(A_[i][0].get_costs()), H.bits(B_[i][0].get_costs())), (k, i)
            for f in H.OUT_FIELDS:
                assert getattr(ra[i][1], f) == getattr(rb[i][1], f), (k, i, f)
        ua = [H.shifted(u) for u, _ in ra]
        ub = [H.shifted(u) for u, _ in rb]
    sa, sb = ga.stats(), gb.stats()
    assert (sa.batched_launches, sa.single_ticks) == (sb.batched_launches, sb.single_ticks)
    assert gb.validation_counts().launches == 8 and ga.validation_counts().launches == 0
    H.close(ga, gb, *[g for g, _ in A_ + B_])


# ---- the group call ----------------------------------------------------------------------------------------

GROUP = ("wall-T56", "K64", "253-footprint", "map-and-disc")      # T = 56 all: different maps, tables, footprints


def _members(Smpc, names):
    cases = [S.case_named(nm) for nm in names]
    gs = []
    for c in cases:
        g = Smpc(c.config())
        g.set_critics(default_critics())
        S.configure(g, c)
        gs.append(g)
    return cases, gs


def _group_call(grp, cases, take=None, **kw):
    params = [dict(collision_lookahead_time=c.lookahead, consider_footprint=c.consider_footprint,
                   moving_obstacles=c.moving_obstacles) for c in cases]
    return grp.validate_trajectories([c.pose for c in cases], [c.u for c in cases], params=params, take=take,
                                     want_poses=True, **kw)


@pytest.mark.parametrize("names", [GROUP[:1], GROUP[:3]], ids=["n1", "n3"])
def test_group_results_are_the_single_calls(Smpc, mod, names):
    cases, twins = _members(Smpc, names)
    want = [run(g, c) for g, c in zip(twins, cases)]
    _, gs = _members(Smpc, names)
    grp = mod.SmpcGroup(gs)
    got = _group_call(grp, cases)
    for i, (a, b) in enumerate(zip(got, want)):
        assert all(getattr(a, f) == getattr(b, f) for f in FIELDS), i
        assert np.array_equal(H.bits(a.xyyaw), H.bits(b.xyyaw)), i
    c = grp.validation_counts()
    assert (c.launches, c.members) == (1, len(names))
    H.close(grp, *gs, *twins)


def test_group_take_status_and_counts(Smpc, mod):
    cases, twins = _members(Smpc, GROUP)
    want = [run(g, c) for g, c in zip(twins, cases)]
    _, gs = _members(Smpc, GROUP)
    grp = mod.SmpcGroup(gs)
    # a tables of the group's own: read where it lives
    grp.set_moving_obstacles([None if c.xy is None else (c.xy, c.radius) for c in cases])
    got = _group_call(grp, cases, take=[1, 0, 1, 1])
    assert got[1] is None
    for i in (0, 2, 3):
        assert all(getattr(got[i], f) == getattr(want[i], f) for f in FIELDS), i
        assert np.array_equal(H.bits(got[i].xyyaw), H.bits(want[i].xyyaw)), i
    assert grp.validation_counts().launches == 1 and grp.validation_counts().members == 3
    got = _group_call(grp, cases)
    assert all(getattr(got[1], f) == getattr(want[1], f) for f in FIELDS)
    assert grp.validation_counts().launches == 2 and grp.validation_counts().members == 7
    # a member that fails alone: consider_footprint without a footprint (member 0 has none)
    import dataclasses
    broken = [dataclasses.replace(cases[0], consider_footprint=True)] + list(cases[1:])
    got = _group_call(grp, broken)
    assert isinstance(got[0], mod.SmpcError) and got[0].code == A.SMPC_ERR_STATE
    for i in (1, 2, 3):
        assert all(getattr(got[i], f) == getattr(want[i], f) for f in FIELDS), i
    assert grp.validation_counts().launches == 3 and grp.validation_counts().members == 10
    with pytest.raises(mod.SmpcError) as e:
        _group_call(grp, cases, take=[0, 0, 0, 0])
    assert e.value.code == A.SMPC_ERR_INVALID
    assert grp.validation_counts().launches == 3
    H.close(grp, *gs, *twins)
