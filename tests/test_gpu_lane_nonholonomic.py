"""DiffDrive and Ackermann on the lane-per-rollout pass without a vy stream (smpc_pass_lane_nh).

A non-holonomic model holds vy at zero: no vy noise, state.vy = 0, no vy in the integration, the
gamma term, the update or the Twist (the isHolonomic() branches of optimizer.cpp).  From 61 440
rollouts up a plain cruise tick of such a model — the five critics with ObstaclesCritic scored, every
cost_power 1, T <= 64 in whole quads — runs the rows of smpc_pass_lane_nh, which neither load nor
carry vy; every other tick keeps the Omni-form instance it had, and SMPC_NONHOLO_PASS=omni keeps
those for the plain ticks too.  Three things are checked at the smallest batch the rule reaches,
61 440 rollouts (960 groups):
  a. the instance each tick shape runs, by name;
  b. the two routes give EQUAL results (the Omni-form route only ever adds or multiplies +-0 for vy,
     DESIGN.md 4.2d): control sequence, per-rollout costs and the integer outputs, bit for bit;
  c. parity with the CPU oracle, which restates the reference's non-holonomic branches.
Every non-holonomic case has a sideways measured speed (0.3 m/s) and a stale caller vy row (0.123):
an instance that still looked at vy would show.
"""
import numpy as np
import pytest

from mpcholonavigation_amd import _abi as A
from mpcholonavigation_amd.tick import Tick
from tests.harness import (DEPLOYED, FIVE, NO_OBST, Oracle, Smpc,  # noqa: F401
                           copy_of, create_with_env, critics_of, last_kernel)
from tests.helpers import assert_parity, configure, make_case
from tests.kernel_names import LANE_NH_ROW, LANE_ROW, lane, lane_pow

pytestmark = pytest.mark.gpu

B = 61440
DIFF, ACKER, OMNI = A.SMPC_MODEL_DIFF_DRIVE, A.SMPC_MODEL_ACKERMANN, A.SMPC_MODEL_OMNI
MODEL_NAME = {DIFF: "DiffDrive", ACKER: "Ackermann", OMNI: "Omni"}
KNOB = {"SMPC_NONHOLO_PASS": "omni"}
F, Tr = False, True


# the instance without a vy stream, and the Omni-form instance of the same tick, by horizon
NH_KERNEL, OMNI_KERNEL = LANE_NH_ROW, LANE_ROW

_CASES = {}


def case(batch, T, model=DIFF, **kw):
    """make_case, made once per scene and shared (the noise of 61 440 x 64 is the slow part); the
    config is handed out as a copy with the motion model set, scenario and noise are read only."""
    key = (batch, T, tuple(sorted(kw.items())))
    if key not in _CASES:
        _CASES[key] = make_case(batch, T, **kw)
    cfg, scn, noise = _CASES[key]
    return copy_of(cfg, motion_model=model, ackermann_min_turning_r=0.5), scn, noise


def sideways(t, dx=0.0, dy=0.0, yaw=None, **kw):
    """The tick with a sideways measured speed (ignored by a non-holonomic model), optionally moved."""
    return Tick(t.pose_x + dx, t.pose_y + dy, t.pose_yaw if yaw is None else yaw, (t.speed[0], 0.3, t.speed[2]),
                t.path_x, t.path_y, t.path_yaw, t.goal_x, t.goal_y, **kw)


def colliding(scn):
    """test_gpu_lane_powers.py's colliding tick: the robot 0.45 m beside the plan, heading into the obstacles."""
    return sideways(scn.tick, dy=-0.45, yaw=-0.3)


def stale_u0(scn, model, T):
    """The caller's control sequence with a stale vy row; Ackermann: a tight turn in the first half of
    the horizon, so that the turning-radius bound has work to do (test_non_holonomic_motion_models_parity)."""
    u0 = scn.u0.copy()
    u0[1] = 0.123
    if model == ACKER:
        u0[0, :T // 2] = 0.25
        u0[2, :T // 2] = np.where(np.arange(T // 2) % 8 < 4, 0.9, -0.9)
    return u0


def make_ctx(Smpc, monkeypatch, cfg, scn, noise, critics=None, env=None, seed=None):
    g = create_with_env(Smpc, monkeypatch, cfg, env)
    configure(g, scn, critics=critics if critics is not None else critics_of(FIVE), noise=noise)
    if seed is not None:
        g.seed(seed)
    return g


# ---- a. routing, pinned by name ----------------------------------------------------------------------

NH_TICKS = [(DIFF, 64), (DIFF, 56), (DIFF, 40), (ACKER, 64)]


@pytest.mark.parametrize("model,T", NH_TICKS, ids=[f"{MODEL_NAME[m]}-{T}" for m, T in NH_TICKS])
def test_plain_cruise_tick_runs_the_instance_without_vy(Smpc, monkeypatch, model, T):
    cfg, scn, noise = case(B, T, model)
    g = make_ctx(Smpc, monkeypatch, cfg, scn, noise)
    u = stale_u0(scn, model, T)
    for k in range(2):       # the first tick without a furthest-point prediction, the second speculated
        u, out = g.optimize(sideways(scn.tick), u)
        print(f"[nonholo] {MODEL_NAME[model]} {B}x{T} tick {k}: pass_kind {out.pass_kind} kernel {last_kernel(g)}")
        assert (out.pass_kind, last_kernel(g)) == (1, NH_KERNEL[T]), k
    g.close()


# (id, model, batch, horizon, config flags, critic names, cost_power, near the goal, environment) -> kernel
UNCHANGED = [
    ("omni-64", OMNI, B, 64, 0, FIVE, 1, F, {}, lane()),
    ("diff-30-ragged", DIFF, B, 30, 0, FIVE, 1, F, {}, lane(full=False, quads=False)),
    ("diff-64-near-goal", DIFF, B, 64, 0, FIVE, 1, Tr, {}, lane(ga=True)),
    ("diff-64-no-obstacles-critic", DIFF, B, 64, 0, NO_OBST, 1, F, {}, lane(obst=False)),
    ("diff-64-cost-power-2", DIFF, B, 64, 0, FIVE, 2, F, {}, lane_pow()),
    ("diff-64-deployed-nine", DIFF, B, 64, 0, DEPLOYED, 1, F, {}, lane(dep=True)),
    ("diff-4096-lane-flag", DIFF, 4096, 64, A.SMPC_FLAG_LANE_PER_ROLLOUT, FIVE, 1, F, {}, lane()),
    ("diff-64-knob-omni", DIFF, B, 64, 0, FIVE, 1, F, KNOB, lane()),
]


@pytest.mark.parametrize("c", UNCHANGED, ids=[c[0] for c in UNCHANGED])
def test_every_other_tick_keeps_its_instance(Smpc, monkeypatch, c):
    name, model, batch, T, flags, names, power, near, env, kernel = c
    cfg, scn, noise = case(batch, T, model, near_goal=near)
    cfg.flags |= flags
    g = make_ctx(Smpc, monkeypatch, cfg, scn, noise, critics_of(names, power), env)
    u = stale_u0(scn, DIFF, T)
    for k in range(2):
        u, out = g.optimize(sideways(scn.tick), u)
        print(f"[nonholo] {name} tick {k}: pass_kind {out.pass_kind} kernel {last_kernel(g)}")
        assert (out.pass_kind, last_kernel(g)) == (1, kernel), (name, k)
    g.close()


def test_tick_stripped_after_a_tick_without_vy_runs_the_plain_row(Smpc, monkeypatch):
    """fail_flag_in (the retry after fallback() scores nothing, critic_manager.cpp:70-73): the pass loses
    ObstaclesCritic after the launch was planned; there is no row without vy for that, the plain one runs."""
    cfg, scn, noise = case(B, 64, DIFF)
    g = make_ctx(Smpc, monkeypatch, cfg, scn, noise)
    _, out = g.optimize(sideways(scn.tick), stale_u0(scn, DIFF, 64))
    assert (out.pass_kind, last_kernel(g)) == (1, NH_KERNEL[64])
    u, out = g.optimize(sideways(scn.tick, fail_flag_in=True), np.zeros_like(scn.u0))
    print(f"[nonholo] stripped: pass_kind {out.pass_kind} kernel {last_kernel(g)}")
    assert out.fail_flag == 1
    assert (out.pass_kind, last_kernel(g)) == (1, lane(obst=False))
    g.close()


# ---- b. equal to the Omni-form route ----------------------------------------------------------------

def tick_both(g_nh, g_omni, tick, u0):
    """The tick on both contexts: ((u, out, kernel) of the library's route, the same of the knob's).
    (The name of the instance launched last is one per process: read it before the other runs.)"""
    un, on = g_nh.optimize(tick, u0)
    kn = last_kernel(g_nh)
    uo, oo = g_omni.optimize(tick, u0)
    return (un, on, kn), (uo, oo, last_kernel(g_omni))


def assert_equal_routes(label, u0, res_nh, res_omni, g_nh, g_omni, kernels):
    (un, on, kn), (uo, oo, ko) = res_nh, res_omni
    cn, co = g_nh.get_costs(), g_omni.get_costs()
    print(f"[nonholo] {label}: {kn} | {ko}; max |du| vx "
          f"{float(np.abs(un[0] - uo[0]).max()):.3g} wz {float(np.abs(un[2] - uo[2]).max()):.3g}, costs differing "
          f"{int(np.sum(cn != co))} of {cn.size}, fail {on.fail_flag}/{oo.fail_flag} furthest "
          f"{on.furthest_reached_path_point}/{oo.furthest_reached_path_point} non_colliding "
          f"{on.non_colliding}/{oo.non_colliding} passes {on.passes}/{oo.passes}")
    assert (on.pass_kind, kn) == (1, kernels[0]), label
    assert (oo.pass_kind, ko) == (1, kernels[1]), label
    assert np.array_equal(un[0], uo[0]) and np.array_equal(un[2], uo[2]), label
    assert np.array_equal(un[1], u0[1]) and np.array_equal(uo[1], u0[1]), label
    assert np.array_equal(cn, co), label
    assert (on.fail_flag, on.furthest_valid, on.furthest_reached_path_point, on.non_colliding, on.passes) == \
        (oo.fail_flag, oo.furthest_valid, oo.furthest_reached_path_point, oo.non_colliding, oo.passes), label


def pair(Smpc, monkeypatch, cfg, scn, noise, seed=None):
    return (make_ctx(Smpc, monkeypatch, cfg, scn, noise, seed=seed),
            make_ctx(Smpc, monkeypatch, cfg, scn, noise, env=KNOB, seed=seed))


def run_equal(Smpc, monkeypatch, label, batch, T, model=DIFF, tick_of=None, iterations=1, rng_seed=None, **scn_kw):
    """One tick on the library's route and on the knob's, same inputs; rng_seed: noise from the device
    RNG with that seed on both instead of the stored noise."""
    cfg, scn, noise = case(batch, T, model, **scn_kw)
    cfg.iteration_count = iterations
    g_nh, g_omni = pair(Smpc, monkeypatch, cfg, scn, None if rng_seed is not None else noise, rng_seed)
    tick = tick_of(scn) if tick_of else sideways(scn.tick)
    u0 = stale_u0(scn, model, T)
    res = tick_both(g_nh, g_omni, tick, u0)
    assert_equal_routes(label, u0, res[0], res[1], g_nh, g_omni, (NH_KERNEL[T], OMNI_KERNEL[T]))
    return g_nh, g_omni, scn, res


def close(*ctxs):
    for g in ctxs:
        g.close()


@pytest.mark.parametrize("T", [64, 56, 40])
def test_cruise_tick_equals_the_omni_form_route(Smpc, monkeypatch, T):
    close(*run_equal(Smpc, monkeypatch, f"cruise {B}x{T}", B, T)[:2])


def test_partial_last_group_equals_the_omni_form_route(Smpc, monkeypatch):
    close(*run_equal(Smpc, monkeypatch, "61450x64 (ten rollouts in the last group)", 61450, 64)[:2])


def test_colliding_tick_equals_the_omni_form_route(Smpc, monkeypatch):
    # (make_case's `seed` is the costmap's: scene 44 of test_gpu_lane_powers)
    g_nh, g_omni, _, res = run_equal(Smpc, monkeypatch, f"colliding {B}x64", B, 64, tick_of=colliding, seed=44)
    for _, out, _ in res:
        assert 0 < out.non_colliding < B
    close(g_nh, g_omni)


def test_two_iterations_equal_the_omni_form_route(Smpc, monkeypatch):
    g_nh, g_omni, _, res = run_equal(Smpc, monkeypatch, f"{B}x64, two iterations", B, 64, iterations=2)
    assert res[0][1].passes == 2
    close(g_nh, g_omni)


def test_all_collide_tick_equals_the_omni_form_route(Smpc, monkeypatch):
    g_nh, g_omni, _, res = run_equal(Smpc, monkeypatch, f"all collide {B}x64", B, 64, all_lethal=True)
    for _, out, _ in res:
        assert out.fail_flag == 1 and out.non_colliding == 0
    close(g_nh, g_omni)


def test_device_rng_noise_equals_the_omni_form_route(Smpc, monkeypatch):
    close(*run_equal(Smpc, monkeypatch, f"device RNG {B}x64", B, 64, rng_seed=77)[:2])


def test_speculation_miss_equals_the_omni_form_route(Smpc, monkeypatch):
    """A second tick a metre further along the plan: the carried furthest point is stale, the pass
    reports the true one and the tick is scored again — by the same instance."""
    g_nh, g_omni, scn, res = run_equal(Smpc, monkeypatch, f"{B}x64 tick 0", B, 64)
    assert res[0][1].passes == 1
    tick, u0 = sideways(scn.tick, dx=1.0), stale_u0(scn, DIFF, 64)
    res = tick_both(g_nh, g_omni, tick, u0)
    assert_equal_routes(f"{B}x64 tick 1, moved 1 m", u0, res[0], res[1], g_nh, g_omni, (NH_KERNEL[64], OMNI_KERNEL[64]))
    assert res[0][1].passes == 2 and res[1][1].passes == 2
    close(g_nh, g_omni)


def test_ackermann_equals_the_omni_form_route(Smpc, monkeypatch):
    close(*run_equal(Smpc, monkeypatch, f"Ackermann {B}x64", B, 64, model=ACKER)[:2])


# ---- c. against the oracle -----------------------------------------------------------------------------

ORACLE = [("diff-64", DIFF, 64, F), ("diff-56", DIFF, 56, F), ("ackermann-64", ACKER, 64, F),
          ("diff-64-colliding", DIFF, 64, Tr)]


@pytest.mark.parametrize("c", ORACLE, ids=[c[0] for c in ORACLE])
def test_tick_without_vy_matches_the_oracle(Smpc, Oracle, monkeypatch, c):
    """The bar of test_non_holonomic_motion_models_parity: assert_parity with at most two collision
    flips, non_colliding equal, the caller's vy row returned as it was; Ackermann: the turning radius
    of the result bounded, and the bound active (DiffDrive's answer differs)."""
    name, model, T, coll = c
    cfg, scn, noise = case(B, T, model, **({"seed": 44} if coll else {}))
    g, o = make_ctx(Smpc, monkeypatch, cfg, scn, noise), Oracle(cfg)
    configure(o, scn, critics=critics_of(FIVE), noise=noise)
    tick = colliding(scn) if coll else sideways(scn.tick)
    tick.goal_checker_xy_tolerance = 0.25
    u0 = stale_u0(scn, model, T)
    ug, og = g.optimize(tick, u0)
    uo, oo = o.optimize(tick, u0)
    print(f"[nonholo] oracle {name}: kernel {last_kernel(g)} non_colliding {og.non_colliding}/{oo.non_colliding}")
    assert (og.pass_kind, last_kernel(g)) == (1, NH_KERNEL[T])
    assert np.array_equal(ug[1], u0[1]) and np.array_equal(uo[1], u0[1])
    assert og.non_colliding == oo.non_colliding
    if coll:
        assert 0 < oo.non_colliding < B
    assert_parity(ug, og, uo, oo, g.get_costs(), o.get_costs(), max_flips=2, label=f"nonholo {name} {B}x{T}")
    if model == ACKER:
        ratio = np.abs(ug[0]) / np.maximum(np.abs(ug[2]), 1e-30)
        assert np.all(ratio >= 0.5 * (1 - 1e-6))
        cfg2, _, _ = case(B, T, DIFF)
        o2 = Oracle(cfg2)
        configure(o2, scn, critics=critics_of(FIVE), noise=noise)
        ud, _ = o2.optimize(tick, u0)
        assert not np.array_equal(ud[2], uo[2])
        o2.close()
    g.close()
    o.close()
