"""GPU parity: the HIP path (through the C-ABI, libsmpc.so) against the CPU oracle
on identical noise, costmap, plan and control sequence.

Tolerance: emitted Twist (and the whole control sequence) within 1e-4 relative
of the oracle — BASELINE.json north_star.  Integer outputs (fail flag, furthest
reached path point, non-colliding count) must match exactly.
"""
import numpy as np
import pytest

from mpcholonavigation_amd import _abi as A
from mpcholonavigation_amd.synthetic import make_noise, make_scenario
from mpcholonavigation_amd.tick import Tick, default_config, default_critics
from tests.harness import DEPLOYED, FIVE, Oracle, Smpc, bar_tick, dressed_critics  # noqa: F401
from tests.helpers import assert_parity, configure, cost_flips, make_case, rel_err, twist

pytestmark = pytest.mark.gpu


def run_pair(Smpc, Oracle, cfg, scn, noise, critics=None, tick=None, u0=None, store=False,
             track_unknown=False):
    if store:
        cfg.flags |= A.SMPC_FLAG_STORE_TRAJECTORIES
    g, o = Smpc(cfg), Oracle(cfg)
    for obj in (g, o):
        configure(obj, scn, critics=critics, noise=noise, track_unknown=track_unknown)
    tick = tick or scn.tick
    u0 = scn.u0 if u0 is None else u0
    ug, og = g.optimize(tick, u0)
    uo, oo = o.optimize(tick, u0)
    return g, o, (ug, og), (uo, oo)


def test_rollout_trajectories_match(Smpc, Oracle):
    """Rollout (a4-a6): x, y, yaw of every rollout against the oracle."""
    cfg, scn, noise = make_case(1000, 30)
    g, o, (ug, og), (uo, oo) = run_pair(Smpc, Oracle, cfg, scn, noise, store=True)
    xg, yg, wg = g.get_generated_trajectories()
    xo, yo, wo = o.get_trajectories()
    # float scan order differs from the sequential cumsum by a few ulp
    assert np.max(np.abs(xg - xo)) < 2e-6
    assert np.max(np.abs(yg - yo)) < 2e-6
    assert np.max(np.abs(wg - wo)) < 2e-6


@pytest.mark.parametrize("B,T", [(1000, 30), (2000, 56), (4096, 64), (512, 100), (300, 128),
                                 (256, 200), (1, 64), (7, 2), (65, 1)])
def test_cruise_parity(Smpc, Oracle, B, T, both_passes):
    """All five critics live (cruise scenario), several batch/horizon shapes incl.
    cfg1 (1000x30), the reference default horizon 56, ragged T and tiny batches."""
    cfg, scn, noise = make_case(B, T)
    g, o, (ug, og), (uo, oo) = run_pair(Smpc, Oracle, cfg, scn, noise)
    assert og.non_colliding == oo.non_colliding
    assert_parity(ug, og, uo, oo, g.get_costs(), o.get_costs(), label=f"cruise {B}x{T}")


def test_cfg2_parity(Smpc, Oracle):
    """BASELINE configs[1]: 65 536 rollouts x 64 steps, 200x200 costmap."""
    cfg, scn, noise = make_case(65536, 64)
    g, o, (ug, og), (uo, oo) = run_pair(Smpc, Oracle, cfg, scn, noise)
    cg, co = g.get_costs(), o.get_costs()
    flips = cost_flips(cg, co)
    assert flips <= 4, flips     # last-ulp cell flips, out of 4.2 M lookups
    assert_parity(ug, og, uo, oo, cg, co, max_flips=4, label="cfg2")
    # against the oracle with double accumulation the agreement is much tighter
    o.set_accumulate_double(True)
    ud, _ = o.optimize(scn.tick, scn.u0)
    assert rel_err(ug, ud) < 2e-5


def test_cfg3_shape_parity(Smpc, Oracle):
    """configs[2] shape at a batch the oracle finishes quickly: T=128 on a
    2000x2000 costmap (window in LDS, the rest from HBM/L2)."""
    cfg, scn, noise = make_case(8192, 128, map_size=2000)
    g, o, (ug, og), (uo, oo) = run_pair(Smpc, Oracle, cfg, scn, noise)
    assert_parity(ug, og, uo, oo, g.get_costs(), o.get_costs(), max_flips=2, label="cfg3 shape")


def test_near_goal_parity(Smpc, Oracle, both_passes):
    """Goal 0.4 m ahead: GoalAngle live, PathAlign/PathFollow/PreferForward gated off."""
    cfg, scn, noise = make_case(1000, 30, near_goal=True)
    g, o, (ug, og), (uo, oo) = run_pair(Smpc, Oracle, cfg, scn, noise)
    assert not oo.furthest_valid and not og.furthest_valid
    assert_parity(ug, og, uo, oo, g.get_costs(), o.get_costs(), label="near goal")


def test_all_collide_sets_fail_flag(Smpc, Oracle, both_passes):
    """Every rollout collides -> fail_flag, later critics not scored (critic_manager.cpp:70-73)."""
    cfg, scn, noise = make_case(512, 30, all_lethal=True)
    g, o, (ug, og), (uo, oo) = run_pair(Smpc, Oracle, cfg, scn, noise)
    assert og.fail_flag == 1 and oo.fail_flag == 1
    assert og.non_colliding == 0
    assert_parity(ug, og, uo, oo, g.get_costs(), o.get_costs(), label="all collide")
    # the retry after fallback(): fail flag sticky, no critic is scored
    t = scn.tick
    t2 = Tick(t.pose_x, t.pose_y, t.pose_yaw, t.speed, t.path_x, t.path_y, t.path_yaw, t.goal_x,
              t.goal_y, fail_flag_in=True)
    u0 = np.zeros_like(scn.u0)
    ug2, og2 = g.optimize(t2, u0)
    uo2, oo2 = o.optimize(t2, u0)
    assert og2.fail_flag == 1 and oo2.fail_flag == 1
    assert_parity(ug2, og2, uo2, oo2, g.get_costs(), o.get_costs(), label="sticky fail")


@pytest.mark.parametrize("iterations", [1, 2])
def test_all_collide_on_the_reread_form(Smpc, Oracle, iterations):
    """T = 128 on the lane pass's re-read form, which has instances with a collision critic
    scored only: the retry after fallback() (fail_flag_in: nothing is scored,
    critic_manager.cpp:70-73) and the later iterations of an all-collide tick (flags stripped the
    same way) must run — on the wave pass — not fail with a device error.

    What can be asserted about the numbers: with every rollout colliding the costs are
    critical_weight x collision_cost = 2e5 each, where a float's ulp is 0.0156 — 5 % of a softmax
    weight at temperature 0.3.  The first iteration adds ONE rounded sum to zero and matches the
    oracle as everywhere else; from the second on the reference adds its three gamma terms to the
    accumulated 2e5 one by one (optimizer.cpp:365-380), the kernels add their sum once, the costs
    differ by an ulp and the weights by percents.  The reference is no better conditioned against
    itself (-ffast-math may reassociate the same adds), and no Twist comes out of such a tick:
    fail_flag is never cleared inside evalControl, so fallback() resets and finally throws
    (optimizer.cpp:134-183).  Hence: integer outputs exact, costs within two ulp, the control
    sequence within the weights' conditioning."""
    cfg, scn, noise = make_case(1024, 128, all_lethal=True)
    cfg.flags |= A.SMPC_FLAG_LANE_PER_ROLLOUT
    cfg.iteration_count = iterations
    g, o, (ug, og), (uo, oo) = run_pair(Smpc, Oracle, cfg, scn, noise)
    assert og.fail_flag == 1 and oo.fail_flag == 1
    assert og.non_colliding == 0
    assert og.passes == iterations + 1      # the all-collide re-score of the first iteration

    def check(ug, og, uo, oo, label):
        if iterations == 1:
            assert_parity(ug, og, uo, oo, g.get_costs(), o.get_costs(), label=label)
            return
        cg, co = g.get_costs(), o.get_costs()
        ulp = float(np.spacing(np.float32(np.max(np.abs(co)))))
        assert float(np.max(np.abs(cg.astype(np.float64) - co))) <= max(2 * ulp, 2e-4), label
        assert og.fail_flag == oo.fail_flag and og.non_colliding == oo.non_colliding
        assert rel_err(ug, uo) < 5e-2, label

    check(ug, og, uo, oo, f"all collide T=128 it={iterations}")
    t = scn.tick
    t2 = Tick(t.pose_x, t.pose_y, t.pose_yaw, t.speed, t.path_x, t.path_y, t.path_yaw, t.goal_x,
              t.goal_y, fail_flag_in=True)
    u0 = np.zeros_like(scn.u0)
    ug2, og2 = g.optimize(t2, u0)
    uo2, oo2 = o.optimize(t2, u0)
    assert og2.fail_flag == 1 and oo2.fail_flag == 1
    assert og2.pass_kind == 0               # nothing to score: the wave pass
    check(ug2, og2, uo2, oo2, f"sticky fail T=128 it={iterations}")


def test_two_iterations_accumulate_costs(Smpc, Oracle, both_passes):
    """iteration_count=2: costs accumulate, furthest point cached."""
    cfg, scn, noise = make_case(2000, 56)
    cfg.iteration_count = 2
    g, o, (ug, og), (uo, oo) = run_pair(Smpc, Oracle, cfg, scn, noise)
    assert og.passes == 2
    assert_parity(ug, og, uo, oo, g.get_costs(), o.get_costs(), label="2 iterations")


def test_track_unknown_and_off_map(Smpc, Oracle, both_passes):
    """255 cells + rollouts leaving the map: NO_INFORMATION collides unless tracking unknown."""
    for track in (False, True):
        cfg, scn, noise = make_case(1000, 64, map_size=60)   # 3 m map: rollouts leave it
        scn.cells[:, 40:44] = 255
        g, o, (ug, og), (uo, oo) = run_pair(Smpc, Oracle, cfg, scn, noise, track_unknown=track)
        assert og.non_colliding == oo.non_colliding
        assert_parity(ug, og, uo, oo, g.get_costs(), o.get_costs(), max_flips=1,
                      label=f"unknown track={track}")


def test_blocked_path_gates(Smpc, Oracle, both_passes):
    """Invalid path points: PathFollow skips ahead, PathAlign's occupancy gate stands down."""
    cfg, scn, noise = make_case(1000, 56)
    P = len(scn.tick.path_x)
    valid = np.ones(P - 1, np.uint8)
    valid[20:40] = 0
    t = scn.tick
    tick = Tick(t.pose_x, t.pose_y, t.pose_yaw, t.speed, t.path_x, t.path_y, t.path_yaw,
                t.goal_x, t.goal_y, path_pts_valid=valid)
    g, o, (ug, og), (uo, oo) = run_pair(Smpc, Oracle, cfg, scn, noise, tick=tick)
    assert_parity(ug, og, uo, oo, g.get_costs(), o.get_costs(), label="blocked path")
    valid[:] = 1
    valid[3:6] = 0      # a few invalid points: PathAlign stays on, samples skip them
    tick = Tick(t.pose_x, t.pose_y, t.pose_yaw, t.speed, t.path_x, t.path_y, t.path_yaw,
                t.goal_x, t.goal_y, path_pts_valid=valid)
    ug, og = g.optimize(tick, scn.u0)
    uo, oo = o.optimize(tick, scn.u0)
    assert_parity(ug, og, uo, oo, g.get_costs(), o.get_costs(), label="few invalid")


def test_non_default_critic_params(Smpc, Oracle, both_passes):
    """cost_power 2, use_path_orientations, other weights/steps; curved plan; moving robot."""
    cfg, scn, noise = make_case(1500, 60)
    cr = default_critics()
    cr.obstacles.cost_power = 2
    cr.path_align.cost_power = 2
    cr.path_align.use_path_orientations = 1
    cr.path_align.trajectory_point_step = 3
    cr.path_align.offset_from_furthest = 10
    cr.path_follow.cost_power = 2
    cr.path_follow.offset_from_furthest = 3
    cr.prefer_forward.cost_power = 3
    cr.prefer_forward.cost_weight = 7.5
    t = scn.tick
    P = len(t.path_x)
    s = np.arange(P, dtype=np.float32) * np.float32(0.05)
    path_x = (t.pose_x + s * np.cos(0.3 * s)).astype(np.float32)
    path_y = (t.pose_y + s * np.sin(0.3 * s)).astype(np.float32)
    path_yaw = (0.3 * s).astype(np.float32)
    tick = Tick(t.pose_x + 0.013, t.pose_y - 0.021, 0.2, (0.25, -0.05, 0.3), path_x, path_y,
                path_yaw, float(path_x[-1]), float(path_y[-1]))
    u0 = scn.u0.copy()
    u0[0] = np.linspace(0.2, 0.4, cfg.time_steps)
    u0[1] = 0.05
    u0[2] = np.linspace(-0.2, 0.3, cfg.time_steps)
    g, o, (ug, og), (uo, oo) = run_pair(Smpc, Oracle, cfg, scn, noise, critics=cr, tick=tick,
                                        u0=u0)
    assert_parity(ug, og, uo, oo, g.get_costs(), o.get_costs(), max_flips=1, label="custom critics")


def test_single_critics(Smpc, Oracle, both_passes):
    """Each critic alone (the others disabled) and none at all."""
    names = ["obstacles", "path_align", "path_follow", "goal_angle", "prefer_forward", None]
    for only in names:
        near = only == "goal_angle"
        cfg, scn, noise = make_case(800, 56, near_goal=near)
        cr = default_critics()
        for n in names[:-1]:
            getattr(cr, n).enabled = 1 if n == only else 0
        g, o, (ug, og), (uo, oo) = run_pair(Smpc, Oracle, cfg, scn, noise, critics=cr)
        assert_parity(ug, og, uo, oo, g.get_costs(), o.get_costs(), label=f"only {only}")


def test_constraints_clip(Smpc, Oracle):
    """setSpeedLimit-scaled constraints clip the updated sequence (optimizer.cpp:237-249)."""
    cfg, scn, noise = make_case(1000, 30)
    g, o = Smpc(cfg), Oracle(cfg)
    for obj in (g, o):
        configure(obj, scn, noise=noise)
        obj.set_constraints(0.25, -0.1, 0.01, 0.005)
    ug, og = g.optimize(scn.tick, scn.u0)
    uo, oo = o.optimize(scn.tick, scn.u0)
    assert ug[0].max() <= np.float32(0.25) and ug[1].max() <= np.float32(0.01)
    assert np.abs(ug[2]).max() <= np.float32(0.005)
    assert_parity(ug, og, uo, oo, label="clip")


def test_closed_loop_ticks(Smpc, Oracle, both_passes):
    """Ten ticks with the sequence fed back (shifted) like evalControl does."""
    cfg, scn, noise = make_case(2000, 56)
    g, o = Smpc(cfg), Oracle(cfg)
    for obj in (g, o):
        configure(obj, scn, noise=noise)
    ug = uo = scn.u0
    for k in range(10):
        ug, og = g.optimize(scn.tick, ug)
        uo, oo = o.optimize(scn.tick, uo)
        assert_parity(ug, og, uo, oo, label=f"tick {k}", rtol=2e-4)
        # shiftControlSequence (optimizer.cpp:206-225) on both, identically
        ug = np.concatenate([ug[:, 1:], ug[:, -1:]], axis=1)
        uo = np.concatenate([uo[:, 1:], uo[:, -1:]], axis=1)
        uo = ug.copy()      # re-synchronise: parity of one tick, not error growth


def test_device_rng_matches_cpu_twin(Smpc, Oracle):
    """Philox4x32-10 + Box-Muller noise: integer stream identical, normals within 1e-6."""
    cfg = default_config(batch_size=777, time_steps=33)
    g, o = Smpc(cfg), Oracle(cfg)
    g.seed(2024)
    o.seed(2024)
    for a, b in zip(g.get_noise(), o.get_noise()):
        assert np.max(np.abs(a - b)) < 2e-6
    nvx, nvy, nwz = g.get_noise()
    assert abs(nvx.std() - 0.2) < 0.01 and abs(nvy.std() - 0.2) < 0.01
    assert abs(nwz.std() - 0.4) < 0.02 and abs(nvx.mean()) < 0.01
    first = nvx.copy()
    g.reset()
    o.reset()            # next draw epoch on both
    assert np.max(np.abs(g.get_noise()[0] - o.get_noise()[0])) < 2e-6
    assert np.max(np.abs(g.get_noise()[0] - first)) > 0.1


@pytest.mark.parametrize("B,T,flags", [(4096, 64, A.SMPC_FLAG_LANE_PER_ROLLOUT), (4096, 30, 0), (2048, 56, A.SMPC_FLAG_LANE_PER_ROLLOUT)])
def test_background_redraw_is_the_same_epoch_sequence(Smpc, B, T, flags):
    """smpc_redraw_noise_async (regenerate_noises = true off the tick's critical path, as the
    reference's noise thread, noise_generator.cpp:54-63,97-105): the draw goes into a second set of
    tensors on its own stream, the next tick takes it — bit for bit the ticks and the noise of
    the synchronous smpc_redraw_noise; a draw nobody took is dropped by smpc_seed."""
    cfg = default_config(batch_size=B, time_steps=T, flags=flags)
    scn = make_scenario(T)
    ctxs = []
    for _ in range(2):
        g = Smpc(cfg)
        g.set_critics(default_critics())
        g.set_costmap(scn.cells, scn.origin_x, scn.origin_y, scn.resolution)
        g.seed(77)
        ctxs.append(g)
    sync, bg = ctxs
    us = ub = scn.u0
    for k in range(4):
        us, os_ = sync.optimize(scn.tick, us)
        ub, ob = bg.optimize(scn.tick, ub)
        assert np.array_equal(us, ub), k
        assert os_.min_cost == ob.min_cost and os_.furthest_reached_path_point == ob.furthest_reached_path_point
        sync.redraw_noise()
        bg.redraw_noise_async()
        bg.redraw_noise_async()          # a second request before a tick took the first: no-op
    # the draw requested last has not been taken by a tick: get_noise still shows the noise of the last tick ...
    n_last = [x.copy() for x in bg.get_noise()]
    ub2, _ = bg.optimize(scn.tick, ub)   # ... and this tick takes it
    us2, _ = sync.optimize(scn.tick, us)
    assert np.array_equal(us2, ub2)
    for a, b in zip(sync.get_noise(), bg.get_noise()):
        assert np.array_equal(a, b)
    assert not np.array_equal(n_last[0], bg.get_noise()[0])
    bg.redraw_noise_async()
    bg.seed(77)                           # drops the pending draw: epoch 0 of the seed again
    sync.seed(77)
    for a, b in zip(sync.get_noise(), bg.get_noise()):
        assert np.array_equal(a, b)
    for g in ctxs:
        g.close()


def test_error_paths(Smpc):
    """Error convention: negative status + message, no exception across the ABI."""
    from mpcholonavigation_amd.optimizer import SmpcError
    with pytest.raises(SmpcError) as e:
        Smpc(default_config(batch_size=0))
    assert e.value.code == A.SMPC_ERR_INVALID
    with pytest.raises(SmpcError) as e:
        Smpc(default_config(time_steps=257))
    assert e.value.code == A.SMPC_ERR_UNSUPPORTED
    cfg, scn, noise = make_case(64, 30)
    g = Smpc(cfg)
    with pytest.raises(SmpcError) as e:      # no noise yet
        g.optimize(scn.tick, scn.u0)
    assert e.value.code == A.SMPC_ERR_STATE
    g.set_noise(*noise)
    with pytest.raises(SmpcError) as e:      # no costmap yet
        g.optimize(scn.tick, scn.u0)
    assert e.value.code == A.SMPC_ERR_STATE
    cr = default_critics()
    cr.obstacles.consider_footprint = 1      # accepted, but the tick needs a footprint
    g.set_critics(cr)
    g.set_costmap(scn.cells, scn.origin_x, scn.origin_y, scn.resolution)
    with pytest.raises(SmpcError) as e:
        g.optimize(scn.tick, scn.u0)
    assert e.value.code == A.SMPC_ERR_STATE
    with pytest.raises(SmpcError):           # trajectories were not requested
        g.get_generated_trajectories()


def test_speculation_miss_is_rescored(Smpc, Oracle, both_passes):
    """The furthest point of the previous tick is only a guess: when the plan changes
    the pass reports the true value and the tick is re-scored (passes == 2), so the
    result still equals the oracle's.  SMPC_FLAG_NO_SPECULATION gives the two-pass mode."""
    cfg, scn, noise = make_case(2000, 56)
    g, o = Smpc(cfg), Oracle(cfg)
    for obj in (g, o):
        configure(obj, scn, noise=noise)
    ug, og = g.optimize(scn.tick, scn.u0)          # first tick: exact pre-pass, no hint yet
    uo, oo = o.optimize(scn.tick, scn.u0)
    assert og.passes == 1
    assert_parity(ug, og, uo, oo, label="tick 0")
    ug, og = g.optimize(scn.tick, scn.u0)          # same inputs: the hint is right
    assert og.passes == 1
    assert_parity(ug, og, uo, oo, label="tick 1 (hit)")
    t = scn.tick
    # a plan with twice the spacing: the nearest-point index of every endpoint halves
    P = len(t.path_x)
    px = (t.pose_x + 0.1 * np.arange(P)).astype(np.float32)
    tick2 = Tick(t.pose_x, t.pose_y, t.pose_yaw, t.speed, px, t.path_y, t.path_yaw,
                 float(px[-1]), t.goal_y)
    ug, og = g.optimize(tick2, scn.u0)
    uo, oo = o.optimize(tick2, scn.u0)
    assert og.passes == 2                          # miss -> re-scored with the true value
    assert_parity(ug, og, uo, oo, g.get_costs(), o.get_costs(), label="tick 2 (miss)")
    cfg2, _, _ = make_case(2000, 56)
    cfg2.flags |= A.SMPC_FLAG_NO_SPECULATION
    g2 = Smpc(cfg2)
    configure(g2, scn, noise=noise)
    for _ in range(2):
        ug2, og2 = g2.optimize(tick2, scn.u0)
        assert og2.passes == 1
    assert_parity(ug2, og2, uo, oo, label="two-pass mode")


def test_device_sincos_accuracy(Smpc):
    """The rollout's sin/cos (Cody-Waite reduction by pi + near-minimax polynomials) against
    float64: absolute error <= 1.5e-7 (1.25 ulp of 1.0) over the yaw range rollouts reach and
    beyond, library path on huge arguments."""
    g = Smpc(default_config(batch_size=64, time_steps=8))
    rng = np.random.default_rng(3)
    x = np.concatenate([rng.uniform(-40, 40, 200000), rng.uniform(-0.01, 0.01, 20000),
                        np.linspace(-3.2, 3.2, 50001), rng.uniform(-6e4, 6e4, 20000),
                        np.array([0.0, np.pi / 2, -np.pi / 2, np.pi, 1e6, -3e7, 7e4])]).astype(np.float32)
    s, c = g.selftest_sincos(x)
    xs = x.astype(np.float64)
    # absolute accuracy: the rollout multiplies them by a speed (smpc_device_math.h)
    for got, ref in ((s, np.sin(xs)), (c, np.cos(xs))):
        assert np.max(np.abs(got.astype(np.float64) - ref)) < 1.5e-7
    assert np.max(np.abs(s.astype(np.float64) ** 2 + c.astype(np.float64) ** 2 - 1.0)) < 4e-7


def test_row_transpose_reduce(Smpc):
    """smpc_pass_split's 16 x 16 transpose-reduce inside every 16-lane DPP row: lane i of a row
    gets the sum over the row's lanes of their register i — exact on integers."""
    g = Smpc(default_config(batch_size=64, time_steps=8))
    rng = np.random.default_rng(12)
    for n in (16, 32):
        v = rng.integers(-8, 9, size=(64, n)).astype(np.float32)
        got = g.selftest_row_reduce(v)
        want = np.concatenate([v[n * s:n * s + n].sum(axis=0) for s in range(64 // n)])
        assert np.array_equal(got, want), n


@pytest.mark.parametrize("B,M,nseg,T", [(16384, 200, 0, 64), (4096, 200, 2, 64), (65536, 200, 0, 64), (1000, 200, 0, 64),
                                        (16400, 2000, 0, 64), (70000, 200, 4, 64), (70000, 200, 2, 64), (32768, 200, 0, 64),
                                        (16384, 200, 0, 56), (5000, 200, 0, 48), (3000, 200, 0, 40), (2000, 200, 0, 36),
                                        (20000, 200, 0, 60)])
def test_split_horizon_pass_parity(Smpc, Oracle, B, M, nseg, T, monkeypatch):
    """smpc_pass_split (lane = rollout x quarter of the horizon, the small-batch form at T = 64):
    parity with the oracle over three closed-loop ticks — the first without a furthest-point
    prediction (furthest-only pass in front), then speculated; ragged batches (tail lanes), more
    groups than waves (70 000: forced), a costmap larger than the LDS window; horizons below 64
    (the reference's default 56, and 36 .. 60: the step slots behind the horizon idle)."""
    monkeypatch.setenv("SMPC_PASS", "split")
    if nseg:
        monkeypatch.setenv("SMPC_SPLIT_NSEG", str(nseg))     # (else the library's choice: 4 lanes per rollout up to 32 768, then 2)
    cfg, scn, noise = make_case(B, T, map_size=M)
    g, o = Smpc(cfg), Oracle(cfg)
    for obj in (g, o):
        configure(obj, scn, noise=noise)
    ug = uo = scn.u0
    for k in range(3):
        t = scn.tick
        tk = Tick(t.pose_x + 0.02 * k, t.pose_y, t.pose_yaw, t.speed, t.path_x, t.path_y, t.path_yaw, t.goal_x, t.goal_y)
        ug, og = g.optimize(tk, uo)
        uo, oo = o.optimize(tk, uo)
        assert og.pass_kind == 2, og.pass_kind
        assert og.non_colliding == oo.non_colliding
        assert_parity(ug, og, uo, oo, g.get_costs(), o.get_costs(), max_flips=2, label=f"split {B}x{T} map {M} tick {k}",
                      report=(k == 0))
        uo = np.concatenate([uo[:, 1:], uo[:, -1:]], axis=1)


@pytest.mark.parametrize("B,T,kind", [(4096, 64, 0), (16384, 64, 2), (32768, 64, 2), (16384, 56, 0), (32768, 56, 2),
                                      (20000, 60, 2), (32768, 30, 0), (65536, 64, 1)])
def test_pass_chosen_by_size(Smpc, Oracle, B, T, kind):
    """Which scoring pass a context with default flags runs (smpc_prepare.cpp plan_launch): the wave
    pass for small batches, smpc_pass_split from 12 288 rollouts at T = 64 (20 000 at shorter
    horizons that are multiples of four, 36 and up) while one group per wave fits, the lane pass
    from 61 440 — and the result is the oracle's either way."""
    cfg, scn, noise = make_case(B, T)
    g, o = Smpc(cfg), Oracle(cfg)
    for obj in (g, o):
        configure(obj, scn, noise=noise)
    ug, og = g.optimize(scn.tick, scn.u0)
    uo, oo = o.optimize(scn.tick, scn.u0)
    assert og.pass_kind == kind, (og.pass_kind, g.last_pass_kernel() if hasattr(g, "last_pass_kernel") else "")
    assert_parity(ug, og, uo, oo, g.get_costs(), o.get_costs(), max_flips=2, label=f"chosen {B}x{T}")


def test_a_stale_tick_block_fails_the_tick_and_the_context_recovers(Smpc, monkeypatch):
    """The per-tick inputs reach the device by CPU stores through the PCIe BAR, guarded
    by the tick's number: the pass echoes the number of the block it read, and a tick whose pass read
    another tick's block fails loudly.  SMPC_DEBUG_STALE_TICK=3 withholds the third tick's block: that
    tick must fail (not return the second tick's answer), the context falls back to the stream copy,
    and the next tick is what a context that never saw the fault computes."""
    cfg, scn, noise = make_case(4096, 64)
    cfg.flags |= A.SMPC_FLAG_LANE_PER_ROLLOUT
    bar = bar_tick

    good = Smpc(cfg)
    if not bar(good):
        pytest.skip("this device hands the tick block over by a stream copy (no large BAR / no HDP flush register)")
    monkeypatch.setenv("SMPC_DEBUG_STALE_TICK", "3")
    bad = Smpc(cfg)
    monkeypatch.delenv("SMPC_DEBUG_STALE_TICK")
    for g in (good, bad):
        configure(g, scn, noise=noise)
    t = scn.tick
    ticks = [Tick(t.pose_x + 0.03 * k, t.pose_y, t.pose_yaw + 0.02 * k, t.speed, t.path_x, t.path_y, t.path_yaw, t.goal_x, t.goal_y)
             for k in range(5)]
    for k in range(2):
        ug, _ = good.optimize(ticks[k], scn.u0)
        ub, _ = bad.optimize(ticks[k], scn.u0)
        assert np.array_equal(ug, ub)
    good.optimize(ticks[2], scn.u0)
    with pytest.raises(Exception, match="read tick block 2, not 3"):
        bad.optimize(ticks[2], scn.u0)
    assert bar(good) == 1 and bar(bad) == 0          # the faulted context takes the copy from now on
    for k in (3, 4):
        ug, og = good.optimize(ticks[k], scn.u0)
        ub, ob = bad.optimize(ticks[k], scn.u0)
        assert np.array_equal(ug, ub) and np.array_equal(good.get_costs(), bad.get_costs()), k
        assert og.furthest_reached_path_point == ob.furthest_reached_path_point


def test_windowed_furthest_scan_falls_back_exactly(Smpc, Oracle):
    """The lane pass scans the endpoint's nearest path point from three blocks below the scored
    index up and verifies the rest for the wave's winner (smpc_lane.hip).  Paths on which that
    window is wrong: (1) a plan that doubles back, so that points far apart in index are close in
    space; (2) a tick whose plan has three times the spacing of the last one while the speculated
    index still comes from the old plan — every rollout's true nearest point then lies BELOW the
    window and every wave has to fall back.  The furthest reached path point is an integer output:
    exact, tick after tick."""
    B, T = 4096, 64
    cfg, scn, noise = make_case(B, T)
    cfg.flags |= A.SMPC_FLAG_LANE_PER_ROLLOUT
    g, o = Smpc(cfg), Oracle(cfg)
    for obj in (g, o):
        configure(obj, scn, noise=noise)
    t = scn.tick
    P = len(t.path_x)
    res = float(t.path_x[1] - t.path_x[0])
    # (1) out along +x for 34 points, then back along -x, 0.05 m to the side
    k = np.arange(P)
    out_x = t.path_x[0] + res * np.minimum(k, 33)
    back = np.maximum(k - 33, 0)
    ux = (out_x - res * back).astype(np.float32)
    uy = (t.path_y[0] + np.where(k > 33, 0.05, 0.0)).astype(np.float32)
    uturn = Tick(t.pose_x, t.pose_y, t.pose_yaw, t.speed, ux, uy, np.zeros(P, np.float32), float(ux[-1]), float(uy[-1]))
    # (2) the same straight plan at three times the spacing
    cx = (t.path_x[0] + 3.0 * res * k).astype(np.float32)
    coarse = Tick(t.pose_x, t.pose_y, t.pose_yaw, t.speed, cx, t.path_y.copy(), np.zeros(P, np.float32), float(cx[-1]),
                  float(t.path_y[-1]))
    u = scn.u0
    seen = []
    for label, tk in (("straight", t), ("straight", t), ("u-turn", uturn), ("u-turn", uturn), ("straight", t),
                      ("coarse", coarse), ("coarse", coarse), ("straight", t)):
        ug, og = g.optimize(tk, u)
        uo, oo = o.optimize(tk, u)
        assert og.pass_kind == 1
        assert og.furthest_reached_path_point == oo.furthest_reached_path_point, (label, seen)
        assert_parity(ug, og, uo, oo, g.get_costs(), o.get_costs(), max_flips=1, label=f"window {label}", report=False)
        seen.append((label, int(og.furthest_reached_path_point), int(og.passes)))
        u = np.concatenate([uo[:, 1:], uo[:, -1:]], axis=1)
    print("[windowed furthest scan] (plan, furthest point, scoring passes):", seen)
    # the coarse plan's furthest point lies below the window the straight plan's index opens
    straight = [f for l, f, _ in seen if l == "straight"][0]
    coarse_f = [f for l, f, _ in seen if l == "coarse"][0]
    assert coarse_f + 12 < straight, seen


def test_lane_transpose_reduce(Smpc):
    """The in-register 64 x 64 transpose-reduce (v_permlane32/16_swap + bank-masked DPP) of
    the lane-per-rollout pass: exact on integers, and lane t really gets column t."""
    g = Smpc(default_config(batch_size=64, time_steps=8))
    rng = np.random.default_rng(11)
    v = rng.integers(-8, 9, size=(64, 64)).astype(np.float32)
    w = rng.integers(0, 5, size=64).astype(np.float32)
    got = g.selftest_lane_reduce(v, w)
    assert np.array_equal(got, (w[:, None] * v).sum(axis=0))
    v = rng.normal(size=(64, 64)).astype(np.float32)
    w = rng.uniform(0, 1, size=64).astype(np.float32)
    got = g.selftest_lane_reduce(v, w)
    ref = (w[:, None].astype(np.float64) * v).sum(axis=0)
    assert np.max(np.abs(got - ref)) < 2e-5
    g.close()


@pytest.mark.parametrize("B,T,M", [(1000, 30, 200), (4096, 64, 200), (8192, 64, 2000), (2500, 56, 200),
                                   (2500, 100, 200), (300, 61, 200), (65, 3, 200), (64, 1, 200),
                                   (4096, 128, 2000), (3000, 128, 200), (130, 128, 200),
                                   # horizons that are multiples of four below 64: the whole-quads instance
                                   (777, 4, 200), (1500, 36, 200), (3000, 60, 200), (70000, 56, 200)])
def test_lane_per_rollout_pass_parity(Smpc, Oracle, B, T, M):
    """The lane-per-rollout pass (csrc/smpc_lane.hip: lane = rollout, sequential in time,
    in-register transpose-reduce) against the oracle.  Ticks take it for T <= 64 with the
    controls parked in registers — cruise ticks and near-goal ones (GoalAngle active: instances of
    their own, the term in float; the per-rollout costs stay inside the same bound) — and cruise
    ticks for T = 128 in its re-read form; everything else falls back to the wave pass."""
    for near in (False, True):
        cfg, scn, noise = make_case(B, T, map_size=M, near_goal=near)
        cfg.flags |= A.SMPC_FLAG_LANE_PER_ROLLOUT
        g, o, (ug, og), (uo, oo) = run_pair(Smpc, Oracle, cfg, scn, noise)
        assert og.pass_kind == (1 if (T <= 64 or (T == 128 and not near)) else 0)
        assert og.non_colliding == oo.non_colliding
        assert_parity(ug, og, uo, oo, g.get_costs(), o.get_costs(), max_flips=1,
                      label=f"lane pass {B}x{T} near={near}")


ALL11 = DEPLOYED + ("obstacles", "velocity_deadband")


@pytest.mark.parametrize("names,power,near,B,T", [
    (DEPLOYED, 1, False, 2000, 56), (DEPLOYED, 1, True, 2000, 56), (ALL11, 1, False, 3000, 64),
    (ALL11, 2, False, 1500, 40), (ALL11, 1, True, 1000, 100), (("cost",), 1, False, 4096, 64),
    (("constraint", "velocity_deadband", "twirling"), 3, False, 1000, 30),
    (("path_angle", "goal", "cost"), 1, False, 200000, 64)])
def test_other_registered_critics_parity(Smpc, Oracle, names, power, near, B, T):
    """The six critics beyond the north star's five, alone and mixed with
    them, cruise and near-goal, cost_power 1..3, against the oracle (whose restatement of each
    is pinned by the reference's critics_tests.cpp KATs in test_oracle_reference_kats.py)."""
    cfg, scn, noise = make_case(B, T, near_goal=near)
    # a robot heading away from the path so that PathAngle's gate opens, reversing allowed
    cr = dressed_critics(names, power, path_angle__max_angle_to_furthest=0.05,
                        path_angle__forward_preference=0 if power == 2 else 1)
    tick = scn.tick
    tick.goal_checker_xy_tolerance = 0.25
    g, o, (ug, og), (uo, oo) = run_pair(Smpc, Oracle, cfg, scn, noise, critics=cr, tick=tick)
    assert og.fail_flag == oo.fail_flag
    assert og.non_colliding == oo.non_colliding
    assert_parity(ug, og, uo, oo, g.get_costs(), o.get_costs(), max_flips=2,
                  label=f"critics {names} power {power} near {near}")
    # the wave-per-rollout pass scores these (lean MODE 3 or the general pass); a cruise tick of
    # Constraint / Cost / Twirling with power 1 at a lane-pass batch takes that pass's deployed-list
    # instances (test_deployed_list_cruise_tick_on_the_lane_pass)
    assert og.pass_kind == (1 if B >= 60000 else 0)


@pytest.mark.parametrize("names,power,yaw,B,T,blocked", [
    (("path_align_legacy",), 1, 0, 2000, 56, False),
    (("obstacles", "path_align_legacy", "path_follow", "prefer_forward"), 1, 0, 3000, 64, False),
    (("obstacles", "path_align", "path_align_legacy", "path_follow", "prefer_forward"), 2, 0, 1500, 40, False),
    (("obstacles", "path_align_legacy", "path_follow"), 1, 1, 1000, 100, False),
    (("obstacles", "path_align_legacy", "path_follow"), 1, 0, 1000, 30, True),
    (("obstacles", "path_align_legacy", "path_follow", "prefer_forward"), 1, 0, 70000, 64, False)])
def test_path_align_legacy_critic_parity(Smpc, Oracle, names, power, yaw, B, T, blocked):
    """PathAlignLegacyCritic (path_align_legacy_critic.cpp:46-129; the last of the twelve
    registered critics) on the general pass against the oracle, whose restatement is pinned by
    critics_tests.cpp:564-660 (test_path_align_legacy_critic_kat): alone, with the others, next to
    PathAlignCritic with cost_power 2, with path orientations, with a blocked stretch of the plan
    (some nearest points invalid, then the occupancy gate closed), at a lane-pass batch (which
    falls to the wave pass: the critic lives in the general mode only)."""
    cfg, scn, noise = make_case(B, T)
    cr = dressed_critics(names, power, path_align_legacy__use_path_orientations=yaw)
    t = scn.tick
    P = len(t.path_x)
    pyaw = (0.3 * np.sin(0.2 * np.arange(P))).astype(np.float32) if yaw else t.path_yaw
    g, o = Smpc(cfg), Oracle(cfg)
    for obj in (g, o):
        configure(obj, scn, critics=cr, noise=noise)
    u = scn.u0
    for k in range(3):
        valid = None
        if blocked:
            valid = np.ones(P - 1, np.uint8)
            if k == 1:
                valid[8:11] = 0                 # a few invalid points: samples near them do not count
            if k == 2:
                valid[3:30] = 0                 # the occupancy gate closes: the critic stands down
        tk = Tick(t.pose_x + 0.02 * k, t.pose_y, t.pose_yaw, t.speed, t.path_x, t.path_y, pyaw, t.goal_x, t.goal_y,
                  path_pts_valid=valid)
        ug, og = g.optimize(tk, u)
        uo, oo = o.optimize(tk, u)
        assert og.pass_kind == 0
        assert og.non_colliding == oo.non_colliding
        assert_parity(ug, og, uo, oo, g.get_costs(), o.get_costs(), max_flips=2,
                      label=f"legacy {names} power {power} yaw {yaw} blocked {blocked} tick {k}", report=(k == 0))
        u = np.concatenate([uo[:, 1:], uo[:, -1:]], axis=1)
    # two different sampling steps in one list are refused, not guessed
    cr2 = dressed_critics(("path_align", "path_align_legacy"), 1, path_align_legacy__trajectory_point_step=3)
    g.set_critics(cr2)
    from mpcholonavigation_amd.optimizer import SmpcError
    with pytest.raises(SmpcError) as e:
        g.optimize(t, scn.u0)
    assert e.value.code == A.SMPC_ERR_UNSUPPORTED


@pytest.mark.parametrize("B,T,names", [
    (70000, 64, DEPLOYED), (70000, 56, DEPLOYED), (8192, 64, DEPLOYED), (4096, 56, DEPLOYED),
    (8192, 64, ("cost", "path_align", "path_follow", "prefer_forward")),
    (8192, 64, ("obstacles", "constraint", "twirling", "path_align", "path_follow", "prefer_forward")),
])
def test_deployed_list_cruise_tick_on_the_lane_pass(Smpc, Oracle, B, T, names):
    """The reference's deployed critic list (robot_bringup/config/nav2_params.yaml:222) on a cruise
    tick — away from the goal (Goal and GoalAngle gated off), the robot pointing along the path
    (PathAngle inside its angle) — takes the lane-per-rollout pass's deployed-list instances:
    CostCritic in ObstaclesCritic's place in the lookup pipeline, Constraint and Twirling as
    per-step terms.  Against the oracle, closed loop of three ticks; and the wave pass (MODE 3)
    gives the same tick within float reassociation."""
    cfg, scn, noise = make_case(B, T)
    cfg.flags |= A.SMPC_FLAG_LANE_PER_ROLLOUT
    cr = dressed_critics(names)
    g, o = Smpc(cfg), Oracle(cfg)
    for obj in (g, o):
        configure(obj, scn, critics=cr, noise=noise)
    cfg_w = default_config(batch_size=B, time_steps=T)
    cfg_w.flags &= ~A.SMPC_FLAG_LANE_PER_ROLLOUT
    w = Smpc(cfg_w) if B < 60000 else None      # (below the lane pass's default threshold: the wave pass)
    if w is not None:
        configure(w, scn, critics=cr, noise=noise)
    u = scn.u0
    for k in range(3):
        ug, og = g.optimize(scn.tick, u)
        uo, oo = o.optimize(scn.tick, u)
        assert og.pass_kind == 1, "not the lane pass"
        assert og.non_colliding == oo.non_colliding and og.fail_flag == oo.fail_flag
        assert_parity(ug, og, uo, oo, g.get_costs(), o.get_costs(), max_flips=2,
                      label=f"deployed list on the lane pass {B}x{T} {len(names)} critics tick {k}")
        if w is not None:
            uw, ow = w.optimize(scn.tick, u)
            assert ow.pass_kind == 0
            assert rel_err(ug, uw) < 5e-6
        u = np.concatenate([uo[:, 1:], uo[:, -1:]], axis=1)


@pytest.mark.parametrize("lane", [False, True])
def test_huge_yaw_takes_the_checked_sincos(Smpc, Oracle, lane):
    """A rollout whose yaw leaves the range of the fast sin/cos reduction (|yaw| >= 65536):
    the wave pass branches to the library sin/cos for that lane, the lane pass notices it at
    the end of the group and redoes the group with the checked instance.  Supplied noise with
    a few absurd wz samples; everything else as usual."""
    cfg, scn, noise = make_case(4096, 64)
    if lane:
        cfg.flags |= A.SMPC_FLAG_LANE_PER_ROLLOUT
    nvx, nvy, nwz = [n.copy() for n in noise]
    nwz[5, 3] = 3.0e7          # yaw jumps to 1.5e6 rad at step 4 and stays there
    nwz[70, 10] = -2.5e8
    nwz[4000, 62] = 9.0e6      # only the last steps
    g, o, (ug, og), (uo, oo) = run_pair(Smpc, Oracle, cfg, scn, (nvx, nvy, nwz))
    import os
    if not os.environ.get("SMPC_PASS"):
        assert og.pass_kind == (1 if lane else 0)
    assert og.non_colliding == oo.non_colliding
    assert_parity(ug, og, uo, oo, g.get_costs(), o.get_costs(), max_flips=2,
                  label=f"huge yaw lane={lane}")


FOOTPRINT = np.array([[0.25, 0.18], [0.25, -0.18], [-0.25, -0.18], [-0.25, 0.18]])   # 0.5 x 0.36 m


@pytest.mark.parametrize("names,fp_obs,fp_cost,B,T", [
    (("cost", "path_follow", "prefer_forward"), False, True, 2000, 56),
    (("obstacles", "path_align", "path_follow"), True, False, 2000, 56),
    (DEPLOYED, False, True, 2000, 56),
    (("obstacles", "goal", "twirling"), True, False, 1500, 40),
    (("cost", "constraint", "velocity_deadband"), False, True, 1000, 64)])
def test_consider_footprint_parity(Smpc, Oracle, names, fp_obs, fp_cost, B, T):
    """consider_footprint = true (the deployed YAML sets it for CostCritic):
    a rectangular footprint checked with nav2's footprintCostAtPose wherever the centre cost
    reaches the possibly-inscribed cost; GPU general pass vs the oracle's restatement."""
    from scipy import ndimage
    cfg, scn, noise = make_case(B, T)
    # a wall 0.35 m beside the path with nav2's inflation around it (inscribed 0.1 m,
    # radius 0.55 m, scaling 10): sideways rollouts graze or hit it
    res, t = scn.resolution, scn.tick
    cells = np.zeros_like(scn.cells)
    ix0, ix1 = int((t.pose_x + 0.3) / res), int((t.pose_x + 1.3) / res)
    iy = int((t.pose_y + 0.35) / res)
    cells[iy:iy + 2, ix0:ix1] = 254
    d = ndimage.distance_transform_edt(cells != 254) * res
    infl = np.where(d <= 0.1, 253, np.floor(252 * np.exp(-10.0 * (d - 0.1)))).astype(np.uint8)
    infl[d > 0.55] = 0
    cells = np.where(cells == 254, 254, infl).astype(np.uint8)
    scn.cells = cells
    cr = dressed_critics(names)
    cr.obstacles.consider_footprint = int(fp_obs)
    cr.cost.consider_footprint = int(fp_cost)
    g, o = Smpc(cfg), Oracle(cfg)
    for obj in (g, o):
        configure(obj, scn, critics=cr, noise=noise)
        obj.set_footprint(FOOTPRINT, circumscribed_radius=float(np.hypot(0.25, 0.18)),
                          layer_cost_scaling_factor=10.0)
    ug, og = g.optimize(scn.tick, scn.u0)
    uo, oo = o.optimize(scn.tick, scn.u0)
    assert og.fail_flag == oo.fail_flag
    assert og.non_colliding == oo.non_colliding
    assert 0 < oo.non_colliding < B          # the footprint really decides some rollouts
    assert_parity(ug, og, uo, oo, g.get_costs(), o.get_costs(), max_flips=3,
                  label=f"footprint {names} obs={fp_obs} cost={fp_cost}")


def test_consider_footprint_needs_a_footprint(Smpc):
    cfg, scn, noise = make_case(256, 30)
    cr = dressed_critics(("cost",))
    cr.cost.consider_footprint = 1
    g = Smpc(cfg)
    configure(g, scn, critics=cr, noise=noise)
    with pytest.raises(Exception, match="smpc_set_footprint"):
        g.optimize(scn.tick, scn.u0)


@pytest.mark.parametrize("fp_obs,fp_cost,wall,expect", [
    (1, 1, "beside", "some"),          # both check the footprint: some rollouts collide for each
    (1, 0, "beside", "some"),
    (0, 1, "beside", "some"),
    (1, 0, "ahead", "obstacles"),      # every rollout's FOOTPRINT touches the wall, no centre does: Obstacles stops the manager
    (0, 1, "ahead", "cost"),           # ... Cost does, before Obstacles is scored
    (1, 1, "ahead", "cost")])
@pytest.mark.parametrize("iters", [1, 2])
def test_both_collision_critics_with_a_footprint(Smpc, Oracle, fp_obs, fp_cost, wall, expect, iters):
    """CostCritic and ObstaclesCritic in one list with consider_footprint on either: they disagree on
    which rollouts collide, each assigns fail_flag from its own collisions (cost_critic.cpp,
    obstacles_critic.cpp:177) and the manager stops behind the first that finds every rollout
    colliding (critic_manager.cpp:70-73).  A scoring pass reports ONE non-colliding count (Cost's,
    scored first): smpc_optimize counts Obstacles' with a pass of its own and re-scores what the
    reference had scored.  (Round 2 refused this configuration.)"""
    from scipy import ndimage
    B, T = (2000, 56) if wall == "beside" else (1024, 30)
    cfg, scn, noise = make_case(B, T)
    cfg.iteration_count = iters
    res, t = scn.resolution, scn.tick
    cx, cy = int(t.pose_x / res), int(t.pose_y / res)
    cells = np.zeros_like(scn.cells)
    u0 = scn.u0
    if wall == "beside":
        ix0, ix1 = int((t.pose_x + 0.3) / res), int((t.pose_x + 1.3) / res)
        iy = int((t.pose_y + 0.35) / res)
        cells[iy:iy + 2, ix0:ix1] = 254
        d = ndimage.distance_transform_edt(cells != 254) * res
        infl = np.where(d <= 0.1, 253, np.floor(252 * np.exp(-10.0 * (d - 0.1)))).astype(np.uint8)
        infl[d > 0.55] = 0
        cells = np.where(cells == 254, 254, infl).astype(np.uint8)
    else:
        cells[cy - 30:cy + 30, cx - 6:cx + 4] = 100
        cells[cy - 30:cy + 30, cx + 4] = 254
        scn.tick = Tick(t.pose_x, t.pose_y, 0.0, (0.0, 0.0, 0.0), t.path_x, t.path_y, t.path_yaw, t.goal_x, t.goal_y)
        u0 = np.zeros_like(scn.u0)
        u0[0] = -0.2
    scn.cells = cells
    cr = dressed_critics(("constraint", "cost", "obstacles", "path_follow", "prefer_forward", "goal"))
    cr.obstacles.consider_footprint, cr.cost.consider_footprint = fp_obs, fp_cost
    g, o = Smpc(cfg), Oracle(cfg)
    for obj in (g, o):
        configure(obj, scn, critics=cr, noise=noise)
        obj.set_footprint(FOOTPRINT, circumscribed_radius=float(np.hypot(0.25, 0.18)), layer_cost_scaling_factor=10.0)
    ug, og = g.optimize(scn.tick, u0)
    uo, oo = o.optimize(scn.tick, u0)
    assert og.fail_flag == oo.fail_flag == (0 if expect == "some" else 1)
    assert og.non_colliding == oo.non_colliding
    if expect == "some":
        assert 0 < oo.non_colliding < B
        assert_parity(ug, og, uo, oo, g.get_costs(), o.get_costs(), max_flips=3, label=f"both critics fp {fp_obs}{fp_cost} x{iters}")
    else:
        cg, co = g.get_costs().astype(np.float64), o.get_costs().astype(np.float64)
        assert np.max(np.abs(cg - co)) <= 4e-6 * float(np.max(np.abs(co))), (expect, cg[:4], co[:4])
        assert rel_err(ug, uo) < 1e-3       # (every rollout at the collision cost: the weights hang on its last ulp)


def test_sharded_tick_refuses_both_collision_critics_with_a_footprint(Smpc):
    cfg, scn, noise = make_case(256, 30)
    cr = dressed_critics(("cost", "obstacles"))
    cr.cost.consider_footprint = 1
    g = Smpc(cfg)
    configure(g, scn, critics=cr, noise=noise)
    g.set_footprint(FOOTPRINT, 0.31, 10.0)
    with pytest.raises(Exception, match="sharded tick: consider_footprint=true with both"):
        g.shard_begin(scn.tick, scn.u0)
    # ... and more than one iteration per tick (it would silently run one)
    cfg2, scn2, noise2 = make_case(256, 30)
    cfg2.iteration_count = 2
    g2 = Smpc(cfg2)
    configure(g2, scn2, noise=noise2)
    with pytest.raises(Exception, match="sharded tick: iteration_count must be 1"):
        g2.shard_begin(scn2.tick, scn2.u0)
    g2.shard_comm_init(g2.shard_comm_id(), 0, 1)          # (a one-rank communicator: the tick gets as far as its checks)
    with pytest.raises(Exception, match="sharded tick: iteration_count must be 1"):
        g2.shard_tick(scn2.tick, scn2.u0)


@pytest.mark.parametrize("B,T,names", [(2000, 56, FIVE), (3000, 40, None)])
def test_a_second_pass_of_an_iteration_reads_what_the_first_read(Smpc, B, T, names, monkeypatch):
    """iteration_count > 1: iteration k starts from the control sequence iteration k - 1 left on the
    device, and a re-score inside iteration k (all rollouts colliding, the counting pass above) must
    start from the same one — the first pass's reduction has by then overwritten the result buffer.
    SMPC_DEBUG_REPEAT_PASS launches every iteration's pass twice: same bits as once."""
    cfg, scn, noise = make_case(B, T)
    cfg.iteration_count = 3
    cr = dressed_critics(names) if names else None
    outs = []
    for repeat in (False, True):
        if repeat:
            monkeypatch.setenv("SMPC_DEBUG_REPEAT_PASS", "1")
        g = Smpc(cfg)
        configure(g, scn, critics=cr, noise=noise)
        u, out = g.optimize(scn.tick, scn.u0)
        outs.append((u, out, g.get_costs()))
    (u1, o1, c1), (u2, o2, c2) = outs
    assert o2.passes == 2 * o1.passes
    assert np.array_equal(u1, u2) and np.array_equal(c1, c2)
    assert o1.min_cost == o2.min_cost and o1.sum_w == o2.sum_w


@pytest.mark.parametrize("fp_critic,names", [("obstacles", ("obstacles", "path_follow", "prefer_forward")),
                                             ("cost", ("constraint", "cost", "path_follow", "goal"))])
def test_all_collide_with_a_footprint_is_rescored_with_the_footprint(Smpc, Oracle, fp_critic, names):
    """Every rollout collides only because of the FOOTPRINT (a lethal wall 0.2 m ahead: under the
    outline at the common first pose, never under a centre that stays or backs off): the tick fails,
    and the re-score that restates what the reference had scored when its manager stopped
    (critic_manager.cpp:70-73) must find the same collisions — it once dropped the
    consider_footprint switch and let the rollouts whose centres stay clear survive.  (Found by
    tools/fuzz_parity.py.)"""
    B, T = 512, 20
    cfg, scn, noise = make_case(B, T)
    res, t = scn.resolution, scn.tick
    cx, cy = int(t.pose_x / res), int(t.pose_y / res)
    cells = np.zeros_like(scn.cells)
    cells[cy - 30:cy + 30, cx - 6:cx + 4] = 100          # above the possibly-inscribed cost: footprint checked
    cells[cy - 30:cy + 30, cx + 4] = 254
    scn.cells = cells
    scn.tick = Tick(t.pose_x, t.pose_y, 0.0, (0.0, 0.0, 0.0), t.path_x, t.path_y, t.path_yaw, t.goal_x, t.goal_y)
    u0 = np.zeros_like(scn.u0)
    u0[0] = -0.2                                          # backing off: most centres never reach the wall
    cr = dressed_critics(names)
    getattr(cr, fp_critic).consider_footprint = 1
    g, o = Smpc(cfg), Oracle(cfg)
    for obj in (g, o):
        configure(obj, scn, critics=cr, noise=noise)
        obj.set_footprint(FOOTPRINT, circumscribed_radius=float(np.hypot(0.25, 0.18)), layer_cost_scaling_factor=10.0)
    ug, og = g.optimize(scn.tick, u0)
    uo, oo = o.optimize(scn.tick, u0)
    assert oo.fail_flag == 1 and oo.non_colliding == 0
    assert og.fail_flag == 1 and og.non_colliding == 0
    cg, co = g.get_costs(), o.get_costs()
    assert np.max(np.abs(cg.astype(np.float64) - co)) <= 2e-6 * float(np.max(np.abs(co))), (cg[:4], co[:4])
    # without the footprint the same tick does not fail: the footprint is what decides it
    getattr(cr, fp_critic).consider_footprint = 0
    o.set_critics(cr)
    _, o2 = o.optimize(scn.tick, u0)
    assert o2.fail_flag == 0 and o2.non_colliding > 0


@pytest.mark.parametrize("B,T", [(400, 100), (3000, 56), (20000, 64)])
def test_cost_and_obstacles_critics_together(Smpc, Oracle, B, T):
    """Both collision critics in the list, every cost_power 1 (the additive fast forms of MODE 3):
    ObstaclesCritic's terms are ADDED to CostCritic's — they once replaced them (found by
    tools/fuzz_parity.py: 263 of 400 costs off by up to 4 %)."""
    cfg, scn, noise = make_case(B, T)
    cr = dressed_critics(("obstacles", "cost", "path_follow", "prefer_forward", "constraint"))
    g, o = Smpc(cfg), Oracle(cfg)
    for obj in (g, o):
        configure(obj, scn, critics=cr, noise=noise)
    ug, og = g.optimize(scn.tick, scn.u0)
    uo, oo = o.optimize(scn.tick, scn.u0)
    assert og.non_colliding == oo.non_colliding
    assert_parity(ug, og, uo, oo, g.get_costs(), o.get_costs(), max_flips=2, label=f"cost + obstacles {B}x{T}")


@pytest.mark.parametrize("model,names,B,T,iters", [
    (A.SMPC_MODEL_DIFF_DRIVE, FIVE, 2000, 56, 1),
    (A.SMPC_MODEL_DIFF_DRIVE, ALL11, 1500, 40, 2),
    (A.SMPC_MODEL_DIFF_DRIVE, FIVE, 300, 128, 1),
    (A.SMPC_MODEL_ACKERMANN, FIVE, 2000, 56, 1),
    (A.SMPC_MODEL_ACKERMANN, ALL11, 3000, 64, 2),
    (A.SMPC_MODEL_ACKERMANN, ("constraint", "velocity_deadband", "path_follow"), 1000, 30, 3),
    (A.SMPC_MODEL_DIFF_DRIVE, FIVE, 131072, 64, 1),      # lane-per-rollout pass
    (A.SMPC_MODEL_ACKERMANN, FIVE, 131072, 64, 1)])
def test_non_holonomic_motion_models_parity(Smpc, Oracle, model, names, B, T, iters):
    """DiffDrive and Ackermann (motion_models.hpp:85-171 and the
    isHolonomic() branches of optimizer.cpp): no vy noise, state.vy = 0, no vy in the
    integration, gamma term, update or Twist; the caller's control_sequence.vy row is neither
    read nor written; Ackermann bounds the turning radius of the result and ConstraintCritic
    gains its term.  The library runs these as the Omni kernels with vy held at zero; the oracle
    restates the reference's branches literally (pinned by motion_model_tests.cpp KATs)."""
    cfg, scn, noise = make_case(B, T)
    cfg.motion_model = model
    cfg.iteration_count = iters
    cfg.ackermann_min_turning_r = 0.5
    cr = dressed_critics(names, 1)
    tick = scn.tick
    tick.speed = (tick.speed[0], 0.3, tick.speed[2])   # sideways speed: ignored by these models
    tick.goal_checker_xy_tolerance = 0.25
    u0 = scn.u0.copy()
    u0[1] = 0.123                         # a stale vy row: not read, and returned as it was
    if model == A.SMPC_MODEL_ACKERMANN:
        # a tight turn in the first half of the horizon: the weighted update lands near it,
        # inside the minimum turning radius, so applyConstraints has work to do
        u0[0, :T // 2] = 0.25
        u0[2, :T // 2] = np.where(np.arange(T // 2) % 8 < 4, 0.9, -0.9)
    g, o, (ug, og), (uo, oo) = run_pair(Smpc, Oracle, cfg, scn, noise, critics=cr, tick=tick, u0=u0)
    assert np.array_equal(ug[1], u0[1]) and np.array_equal(uo[1], u0[1])
    nvx, nvy, nwz = g.get_noise()
    assert not nvy.any()                  # noises_vy_ stays zero (noise_generator.cpp:117)
    assert og.non_colliding == oo.non_colliding
    assert_parity(ug, og, uo, oo, g.get_costs(), o.get_costs(), max_flips=2,
                  label=f"motion model {model} {names} {B}x{T} x{iters}")
    import os
    if B >= 131072 and not os.environ.get("SMPC_PASS"):
        assert og.pass_kind == 1
    if model == A.SMPC_MODEL_ACKERMANN:
        # the turning-radius bound held, and it was active somewhere
        ratio = np.abs(ug[0]) / np.maximum(np.abs(ug[2]), 1e-30)
        assert np.all(ratio >= 0.5 * (1 - 1e-6))
        cfg2, _, _ = make_case(B, T)
        cfg2.motion_model, cfg2.iteration_count = A.SMPC_MODEL_DIFF_DRIVE, iters
        o2 = Oracle(cfg2)
        configure(o2, scn, critics=cr, noise=noise)
        ud, _ = o2.optimize(tick, u0)
        assert not np.array_equal(ud[2], uo[2])


def test_non_holonomic_model_draws_no_vy_noise(Smpc, Oracle):
    """Device RNG with a DiffDrive model: vx and wz streams as for Omni, vy all zero, and the
    tick matches the oracle drawing from the same Philox streams."""
    cfg, scn, _ = make_case(4096, 56)
    cfg.motion_model = A.SMPC_MODEL_DIFF_DRIVE
    g, o = Smpc(cfg), Oracle(cfg)
    for obj in (g, o):
        configure(obj, scn)
        obj.seed(77)
    ug, og = g.optimize(scn.tick, scn.u0)
    uo, oo = o.optimize(scn.tick, scn.u0)
    gx, gy, gz = g.get_noise()
    ox, oy, oz = o.get_noise()
    assert not gy.any() and not oy.any()
    assert np.max(np.abs(gx - ox)) < 2e-6 and np.max(np.abs(gz - oz)) < 2e-6
    assert_parity(ug, og, uo, oo, g.get_costs(), o.get_costs(), max_flips=2, label="diffdrive rng")


@pytest.mark.parametrize("model", ["Omni", "DiffDrive", "Ackermann"])
def test_reference_smoke_fixture(Smpc, Oracle, model):
    """test/optimizer_smoke_test.cpp:45-116 on the GPU: the reference's 40x40 costmap with the
    8x8 block of cost 250 under the robot, batch 400, horizon 15, the three motion models with
    their critic lists.  The reference's own assertion (no throw: the tick does not fail) plus
    parity with the oracle on the same noise."""
    from tests.helpers import reference_smoke_fixture
    cfg, cells, res, tick, u0, cr = reference_smoke_fixture(model)
    noise = make_noise(cfg.batch_size, cfg.time_steps)
    g, o = Smpc(cfg), Oracle(cfg)
    for obj in (g, o):
        obj.set_critics(cr)
        obj.set_costmap(cells, 0.0, 0.0, res, inscribed_radius=0.0, cost_scaling_factor=10.0,
                        inflation_radius=0.55)
        obj.set_noise(*noise)
    ug, og = g.optimize(tick, u0)       # raises on any error of the C-ABI
    uo, oo = o.optimize(tick, u0)
    assert og.fail_flag == 0 and oo.fail_flag == 0
    assert og.non_colliding == oo.non_colliding
    assert_parity(ug, og, uo, oo, g.get_costs(), o.get_costs(), label=f"reference smoke fixture {model}")


@pytest.mark.parametrize("B,T,off", [(70000, 64, 0), (65536, 40, 131072), (61441, 56, 7)])
def test_fused_time_major_fill_is_the_same_stream(Smpc, monkeypatch, B, T, off):
    """A lane-per-rollout context draws its device-RNG noise straight into the group-major layout
    (smpc_fill_noise_tm) and makes the [B,T] copy only on demand: bit for bit the tensors of the
    two-step path (fill [B,T], transpose), for a whole batch and for a shard of a larger one;
    and the lane pass's tick on them equals the tick on the same tensors handed over through
    smpc_set_noise."""
    cfg = default_config(batch_size=B, time_steps=T, shard_offset=off, global_batch_size=off + B,
                         flags=A.SMPC_FLAG_LANE_PER_ROLLOUT)
    scn = make_scenario(T)
    fused = Smpc(cfg)
    configure(fused, scn)
    fused.seed(99)
    u_f, out_f = fused.optimize(scn.tick, scn.u0)
    u_f2, out_f2 = fused.optimize(scn.tick, u_f)       # speculating tick: lane pass
    assert out_f2.pass_kind == 1
    monkeypatch.setenv("SMPC_NO_FUSED_FILL", "1")
    plain = Smpc(cfg)
    configure(plain, scn)
    plain.seed(99)
    for a, b in zip(fused.get_noise(), plain.get_noise()):
        assert np.array_equal(a, b)
    given = Smpc(cfg)
    configure(given, scn, noise=fused.get_noise())
    u_g, _ = given.optimize(scn.tick, scn.u0)
    u_g2, out_g2 = given.optimize(scn.tick, u_g)
    assert np.array_equal(u_f, u_g) and np.array_equal(u_f2, u_g2)
    # a redraw moves to the next epoch on both paths alike
    fused.redraw_noise()
    plain.redraw_noise()
    for a, b in zip(fused.get_noise(), plain.get_noise()):
        assert np.array_equal(a, b)


def test_lane_pass_reread_form_at_64_steps(Smpc, Oracle, monkeypatch):
    """The re-read form of the lane pass (the one T = 128 takes) forced onto a 64-step horizon:
    the same tick as the parked form, to the last bit of the costs (the rollout is the same
    code; only where the weighted sum's operands come from differs: c = u + n formed again from
    the noise, with the same single rounding) and within float reassociation on u."""
    cfg, scn, noise = make_case(8192, 64)
    cfg.flags |= A.SMPC_FLAG_LANE_PER_ROLLOUT
    parked = Smpc(cfg)
    configure(parked, scn, noise=noise)
    u_p, out_p = parked.optimize(scn.tick, scn.u0)
    monkeypatch.setenv("SMPC_LANE_REREAD", "1")
    rr = Smpc(cfg)
    configure(rr, scn, noise=noise)
    u_r, out_r = rr.optimize(scn.tick, scn.u0)
    assert out_p.pass_kind == out_r.pass_kind == 1
    assert np.array_equal(parked.get_costs(), rr.get_costs())
    assert out_p.furthest_reached_path_point == out_r.furthest_reached_path_point
    np.testing.assert_allclose(u_r, u_p, rtol=2e-6, atol=2e-7)
    o = Oracle(cfg)
    configure(o, scn, noise=noise)
    uo, oo = o.optimize(scn.tick, scn.u0)
    assert_parity(u_r, out_r, uo, oo, rr.get_costs(), o.get_costs(), label="re-read form, 8192x64")


@pytest.mark.parametrize("B,T,lane", [(2000, 56, False), (70000, 64, True)])
def test_moving_pose_closed_loop_predicts_the_furthest_point(Smpc, Oracle, B, T, lane):
    """A closed loop with a MOVING pose and a plan pruned to the robot (bench.py MovingScene):
    the furthest reached path point steps both ways between ticks, the host predicts the index
    from the pose's displacement and the plan's shift (predict_hint), and whatever it predicts
    every tick equals the oracle's tick on the same inputs (a miss is re-scored); the
    prediction is right most of the time (without it: ~2 ticks in 3 miss)."""
    from bench import MovingScene, shift
    cfg, scn, noise = make_case(B, T)
    g, o = Smpc(cfg), Oracle(cfg)
    for obj in (g, o):
        configure(obj, scn, noise=noise)
    mv = MovingScene(scn, cfg.model_dt)
    u = scn.u0
    passes, n_ticks, furthest = 0, 24, []
    for k in range(n_ticks):
        tk = mv.tick()
        ug, og = g.optimize(tk, u)
        uo, oo = o.optimize(tk, u)
        assert og.pass_kind == (1 if lane else 0)
        assert_parity(ug, og, uo, oo, g.get_costs(), o.get_costs(), max_flips=2, label=f"moving tick {k}",
                      report=False)
        passes += og.passes - (1 if k == 0 else 0)      # tick 0 has no guess yet: two passes by design
        furthest.append(int(og.furthest_reached_path_point))
        mv.advance(uo)
        u = shift(uo)
    assert len(set(furthest)) > 1, "the scenario must make the index move"
    assert passes <= n_ticks + n_ticks // 3, f"{passes} scoring passes in {n_ticks} ticks"
