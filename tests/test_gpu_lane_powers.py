"""Critics with a cost_power other than 1 on the lane-per-rollout pass (smpc_pass_lane_pow).

A cost_power among the north star's five critics is an ordinary tuning value of the reference
(obstacles_critic.cpp:173-177, path_align_critic.cpp:135: costs += pow(total * weight, power), once per
rollout).  From 61 440 rollouts up such a tick runs the lane pass's power rows instead of the general
wave pass; below that, and for everything else the general pass scores (path orientations, another
trajectory_point_step, T > 64), the route is unchanged.  Every case here runs the smallest batch the
rule reaches, 61 440 rollouts (960 groups), against the CPU oracle on the same stored noise.
"""
import numpy as np
import pytest

from mpcholonavigation_amd import _abi as A
from mpcholonavigation_amd.tick import Tick
from tests.harness import FIVE, Oracle, Smpc, copy_of, critics_of, last_kernel  # noqa: F401
from tests.helpers import assert_parity, configure, make_case, twist_component_errors
from tests.kernel_names import LANE_POW_ROW, lane, lane_pow, wave

pytestmark = pytest.mark.gpu

B = 61440
ALL2 = {n: 2 for n in FIVE}
MIXED = {"obstacles": 2, "path_align": 1, "path_follow": 2, "goal_angle": 3, "prefer_forward": 3}
POWERS = {"all2": ALL2, "mixed": MIXED, "obst2": {"obstacles": 2}, "obst2-pfw3": {"obstacles": 2, "prefer_forward": 3}}
F, Tr = False, True


# the power instance of each tick shape: (T, near the goal) -> kernel
POW_KERNEL = {
    **{(T, F): row for T, row in LANE_POW_ROW.items()},
    (64, Tr): lane_pow(ga=True),
    (40, Tr): lane_pow(full=False, ga=True, quads=False),
}

_CASES = {}


def case(batch, T, **kw):
    """make_case, made once per scene and shared (the noise of 61 440 x 64 is the slow part);
    the config is handed out as a copy, scenario and noise are read only."""
    key = (batch, T, tuple(sorted(kw.items())))
    if key not in _CASES:
        _CASES[key] = make_case(batch, T, **kw)
    cfg, scn, noise = _CASES[key]
    return copy_of(cfg), scn, noise


def colliding_tick(scn):
    """The robot 0.45 m beside the plan, heading into the obstacles: a few hundred rollouts collide."""
    t = scn.tick
    return Tick(t.pose_x, t.pose_y - 0.45, -0.3, t.speed, t.path_x, t.path_y, t.path_yaw, t.goal_x, t.goal_y)


def effective_samples(costs, temperature):
    """(sum w)^2 / sum w^2 of the softmax weights: how many rollouts decide the answer."""
    c = costs.astype(np.float64)
    w = np.exp(-(c - c.min()) / temperature)
    return float(w.sum() ** 2 / np.sum(w * w))


def cost_errors(c, c_ref):
    d = np.abs(c.astype(np.float64) - c_ref.astype(np.float64))
    return float(d.max()), float(np.max(d / np.maximum(np.abs(c_ref), 1.0)))


def check_against_oracle(Smpc, Oracle, cfg, scn, noise, critics, tick, label, kernel=None, min_ess=10.0,
                         with_wave=True):
    """One tick on the library's own choice of pass (the power instance), on the oracle and, for the
    record, on a wave-per-rollout context; the lane pass is held to assert_parity's bar."""
    g, o = Smpc(cfg), Oracle(cfg)
    for obj in (g, o):
        configure(obj, scn, critics=critics, noise=noise)
    ug, og = g.optimize(tick, scn.u0)
    uo, oo = o.optimize(tick, scn.u0)
    cg, co = g.get_costs(), o.get_costs()
    ran = last_kernel(g)
    ess = effective_samples(co, cfg.temperature)
    d_t, r_t = twist_component_errors(ug, uo)
    print(f"[lane powers] {label}: kernel {ran}; oracle effective sample size {ess:.1f}, non_colliding "
          f"{oo.non_colliding} (gpu {og.non_colliding}); lane twist |d| {d_t} rel {r_t}; "
          f"costs max |d| {cost_errors(cg, co)[0]:.3g} max rel {cost_errors(cg, co)[1]:.3g}")
    if with_wave:
        cfg.flags |= A.SMPC_FLAG_WAVE_PER_ROLLOUT
        w = Smpc(cfg)
        configure(w, scn, critics=critics, noise=noise)
        uw, ow = w.optimize(tick, scn.u0)
        d_w, r_w = twist_component_errors(uw, uo)
        cw = w.get_costs()
        print(f"[lane powers] {label}: wave pass ({last_kernel(w)}) twist |d| {d_w} rel {r_w}; "
              f"costs max |d| {cost_errors(cw, co)[0]:.3g} max rel {cost_errors(cw, co)[1]:.3g}")
        assert ow.pass_kind == 0
        w.close()
    assert og.pass_kind == 1, (label, ran)
    if kernel is not None:
        assert ran == kernel, label
    assert ess >= min_ess, f"{label}: the oracle's softmax has {ess:.1f} effective samples"
    assert og.fail_flag == oo.fail_flag, label
    assert og.non_colliding == oo.non_colliding, label
    assert_parity(ug, og, uo, oo, cg, co, max_flips=2, label=label)
    g.close()
    o.close()
    return og, oo


# ---- a. selection ---------------------------------------------------------------------------------

@pytest.mark.parametrize("T,near", list(POW_KERNEL), ids=[f"{T}{'-near-goal' if n else ''}" for T, n in POW_KERNEL])
def test_power_tick_runs_the_power_instance(Smpc, T, near):
    cfg, scn, noise = case(B, T, near_goal=near)
    g = Smpc(cfg)
    configure(g, scn, critics=critics_of(FIVE, ALL2), noise=noise)
    u = scn.u0
    for k in range(2):       # the first tick without a furthest-point prediction, the second speculated
        u, out = g.optimize(scn.tick, u)
        print(f"[lane powers] {B}x{T} near {near} tick {k}: pass_kind {out.pass_kind} kernel {last_kernel(g)}")
        assert (out.pass_kind, last_kernel(g)) == (1, POW_KERNEL[(T, near)]), k
    g.close()


def test_power_1_tick_keeps_its_instance(Smpc):
    cfg, scn, noise = case(B, 64, near_goal=False)
    g = Smpc(cfg)
    configure(g, scn, critics=critics_of(FIVE, {}), noise=noise)
    _, out = g.optimize(scn.tick, scn.u0)
    assert (out.pass_kind, last_kernel(g)) == (1, lane())
    g.close()


def _step3(cr):
    cr.path_align.trajectory_point_step = 3


def _path_yaw(cr):
    cr.path_align.use_path_orientations = 1


# (id, batch, horizon, config flags, change to the critics) -> kernel of the wave pass
STAYS_WAVE = [
    ("small-batch-lane-flag", 2048, 64, A.SMPC_FLAG_LANE_PER_ROLLOUT, None, wave(1, 2, Tr)),
    ("trajectory-point-step-3", B, 64, 0, _step3, wave(1, 2, Tr)),
    ("use-path-orientations", B, 64, 0, _path_yaw, wave(1, 2, Tr)),
    ("horizon-128", B, 128, 0, None, wave(2, 2, Tr)),
]


@pytest.mark.parametrize("c", STAYS_WAVE, ids=[c[0] for c in STAYS_WAVE])
def test_power_tick_outside_the_rule_stays_on_the_wave_pass(Smpc, c):
    name, batch, T, flags, change, kernel = c
    cfg, scn, noise = case(batch, T, near_goal=False)
    cfg.flags |= flags
    cr = critics_of(FIVE, ALL2)
    if change:
        change(cr)
    g = Smpc(cfg)
    configure(g, scn, critics=cr, noise=noise)
    _, out = g.optimize(scn.tick, scn.u0)
    print(f"[lane powers] {name}: pass_kind {out.pass_kind} kernel {last_kernel(g)}")
    assert (out.pass_kind, last_kernel(g)) == (0, kernel), name
    g.close()


# ---- b. parity against the oracle -----------------------------------------------------------------

PARITY = [(T, F, pw) for T in (64, 56, 40, 30) for pw in ("all2", "mixed")] + [(64, Tr, "mixed"), (40, Tr, "mixed")]


@pytest.mark.parametrize("T,near,pw", PARITY, ids=[f"{T}{'-near-goal' if n else ''}-{pw}" for T, n, pw in PARITY])
def test_power_tick_matches_the_oracle(Smpc, Oracle, T, near, pw):
    """Cruise and near-goal ticks with cost powers: the Twist within TWIST_RTOL of the oracle's, at most
    two collision flips (what the lean lane pass is allowed at this size), fail_flag and non_colliding
    equal.  The oracle's answers under "all2" and "mixed" differ from the power-1 answer by 1e-2..1e-1
    and from each other by 1e-4..1e-2 (where small, the per-rollout costs carry the check), with 15-100
    effective samples: a power on the wrong critic, on the sum or not at all cannot pass."""
    cfg, scn, noise = case(B, T, near_goal=near)
    check_against_oracle(Smpc, Oracle, cfg, scn, noise, critics_of(FIVE, POWERS[pw]), scn.tick,
                         f"{B}x{T} {'near goal ' if near else ''}{pw}", kernel=POW_KERNEL[(T, near)])


# ---- c. a scene with colliding rollouts -------------------------------------------------------------

@pytest.mark.parametrize("T", [64, 56])
@pytest.mark.parametrize("pw", ["obst2", "obst2-pfw3"])
def test_power_tick_with_colliding_rollouts_matches_the_oracle(Smpc, Oracle, T, pw):
    """collision_cost through the power (1e5 squared) next to ordinary costs."""
    cfg, scn, noise = case(B, T, seed=44)
    og, oo = check_against_oracle(Smpc, Oracle, cfg, scn, noise, critics_of(FIVE, POWERS[pw]), colliding_tick(scn),
                                  f"colliding {B}x{T} {pw}", kernel=POW_KERNEL[(T, F)])
    assert 0 < oo.non_colliding < B
    assert og.non_colliding == oo.non_colliding


# ---- d. two iterations: the accumulated cost enters the power sum ------------------------------------

def test_power_tick_two_iterations_matches_the_oracle(Smpc, Oracle):
    cfg, scn, noise = case(B, 64, near_goal=False)
    cfg.iteration_count = 2
    check_against_oracle(Smpc, Oracle, cfg, scn, noise, critics_of(FIVE, ALL2), scn.tick, f"{B}x64 all2 two iterations",
                         kernel=POW_KERNEL[(64, F)], min_ess=0.0)


# ---- e. a tick whose flags are stripped after it was planned -----------------------------------------

def test_stripped_power_tick_runs_and_matches_the_oracle(Smpc, Oracle):
    """fail_flag_in (the retry after fallback() scores nothing, critic_manager.cpp:70-73): the pass
    loses ObstaclesCritic after the launch was planned for a power tick."""
    cfg, scn, noise = case(B, 64, near_goal=False)
    g, o = Smpc(cfg), Oracle(cfg)
    for obj in (g, o):
        configure(obj, scn, critics=critics_of(FIVE, ALL2), noise=noise)
    _, out = g.optimize(scn.tick, scn.u0)
    o.optimize(scn.tick, scn.u0)
    assert (out.pass_kind, last_kernel(g)) == (1, POW_KERNEL[(64, F)])
    t = scn.tick
    t2 = Tick(t.pose_x, t.pose_y, t.pose_yaw, t.speed, t.path_x, t.path_y, t.path_yaw, t.goal_x, t.goal_y,
              fail_flag_in=True)
    u0 = np.zeros_like(scn.u0)
    ug, og = g.optimize(t2, u0)
    uo, oo = o.optimize(t2, u0)
    print(f"[lane powers] stripped tick: pass_kind {og.pass_kind} kernel {last_kernel(g)}")
    assert og.fail_flag == 1 and oo.fail_flag == 1
    assert_parity(ug, og, uo, oo, g.get_costs(), o.get_costs(), label="stripped power tick")
    g.close()
    o.close()


# ---- f. every rollout collides ------------------------------------------------------------------------

def test_all_collide_power_tick_matches_the_oracle(Smpc, Oracle):
    cfg, scn, noise = case(B, 64, all_lethal=True)
    g, o = Smpc(cfg), Oracle(cfg)
    for obj in (g, o):
        configure(obj, scn, critics=critics_of(FIVE, ALL2), noise=noise)
    ug, og = g.optimize(scn.tick, scn.u0)
    uo, oo = o.optimize(scn.tick, scn.u0)
    print(f"[lane powers] all collide: pass_kind {og.pass_kind} kernel {last_kernel(g)} passes {og.passes}")
    assert og.fail_flag == 1 and oo.fail_flag == 1
    assert og.non_colliding == 0
    assert_parity(ug, og, uo, oo, label="all collide, powers")
    g.close()
    o.close()
