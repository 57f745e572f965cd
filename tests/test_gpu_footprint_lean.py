"""consider_footprint on the lean wave pass: smpc_pass<R, 4, FULL>, the instance a tick runs when
its list has one collision critic with the footprint switch, every cost_power 1 and nothing else
that needs the general pass — the deployed YAML as written (nav2_params.yaml:184-293, CostCritic
consider_footprint: true).  Which instance runs, parity with the CPU oracle, the general pass on
the same tick (SMPC_FOOTPRINT_PASS=general), every kind of second pass, a closed loop, emulated
shards and the host optimizer's C face.

Scene, footprint, lists and shapes: tests/footprint_scenes.py.  The bar is the one of
test_gpu_parity.py::test_consider_footprint_parity on the same scene: assert_parity with
max_flips=3, fail_flag and non_colliding exact."""
import numpy as np
import pytest

from mpcholonavigation_amd import _abi as A
from mpcholonavigation_amd.tick import Tick
from tests.footprint_scenes import (CIRCUMSCRIBED, FOOTPRINT, LAYER_SCALING, SHAPES, critics_of, keep,
                                    list_critics, oracle_tick, setup, wall_case)
from tests.harness import Oracle, Smpc, create_with_env, last_kernel  # noqa: F401
from tests.helpers import assert_parity, rel_err
from tests.kernel_names import wave_at

pytestmark = pytest.mark.gpu


def general_route(Smpc, monkeypatch, cfg):
    """A context whose footprint ticks keep the general pass (the knob is read at smpc_create)."""
    return create_with_env(Smpc, monkeypatch, cfg, {"SMPC_FOOTPRINT_PASS": "general"})


def check(g, ug, og, ref, label):
    assert og.fail_flag == ref.out.fail_flag and og.non_colliding == ref.out.non_colliding, label
    assert_parity(ug, og, ref.u, ref.out, g.get_costs(), ref.costs, max_flips=3, label=label)


# ---- 1. the instance, by name ----------------------------------------------------------------

@pytest.mark.parametrize("B,T", SHAPES)
def test_deployed_list_with_costs_footprint_runs_mode_4(Smpc, B, T):
    cfg, scn, noise = wall_case(B, T)
    g = setup(Smpc(cfg), scn, list_critics("deployed"), noise)
    u = scn.u0
    for k in range(2):       # the first tick without a furthest-point prediction, the second speculated
        u, out = g.optimize(scn.tick, u)
        print(f"[footprint] deployed {B}x{T} tick {k}: pass_kind {out.pass_kind} kernel {last_kernel(g)}")
        assert (out.pass_kind, last_kernel(g)) == (0, wave_at(T, 4)), k
    g.close()


def test_five_critics_with_obstacles_footprint_run_mode_4(Smpc):
    cfg, scn, noise = wall_case(256, 56)
    g = setup(Smpc(cfg), scn, list_critics("five"), noise)
    _, out = g.optimize(scn.tick, scn.u0)
    assert (out.pass_kind, last_kernel(g)) == (0, "smpc_pass<1, 4, false>")
    g.close()


def test_the_knob_keeps_the_general_pass(Smpc, monkeypatch):
    cfg, scn, noise = wall_case(256, 56)
    g = setup(general_route(Smpc, monkeypatch, cfg), scn, list_critics("deployed"), noise)
    _, out = g.optimize(scn.tick, scn.u0)
    assert (out.pass_kind, last_kernel(g)) == (0, "smpc_pass<1, 2, false>")
    g.close()


@pytest.mark.parametrize("why,critics", [
    ("both collision critics with a footprint", lambda: critics_of(("cost", "obstacles", "path_follow"), footprint=("cost",))),
    ("a cost_power of 2", lambda: critics_of(("cost", "path_follow", "prefer_forward"), 2, ("cost",))),
    ("VelocityDeadband in the list", lambda: critics_of(("cost", "path_follow", "velocity_deadband"), footprint=("cost",)))])
def test_what_stays_on_the_general_pass(Smpc, why, critics):
    cfg, scn, noise = wall_case(256, 56)
    g = setup(Smpc(cfg), scn, critics(), noise)
    _, out = g.optimize(scn.tick, scn.u0)
    assert (out.pass_kind, last_kernel(g)) == (0, "smpc_pass<1, 2, false>"), why
    g.close()


def test_a_lane_pass_context_runs_the_wave_pass_for_a_footprint_tick(Smpc):
    """No lane or split instance carries a footprint: the tick takes the wave pass, mode 4."""
    cfg, scn, noise = wall_case(2048, 56)
    cfg.flags |= A.SMPC_FLAG_LANE_PER_ROLLOUT
    g = setup(Smpc(cfg), scn, list_critics("deployed"), noise)
    _, out = g.optimize(scn.tick, scn.u0)
    assert (out.pass_kind, last_kernel(g)) == (0, "smpc_pass<1, 4, false>")
    g.close()


# ---- 2. parity with the oracle ---------------------------------------------------------------

@pytest.mark.parametrize("which", ["deployed", "five"])
@pytest.mark.parametrize("B,T", SHAPES)
def test_parity_with_the_oracle(Smpc, which, B, T):
    on, off = oracle_tick(which, B, T), oracle_tick(which, B, T, footprint=False)
    assert 0 < on.out.non_colliding < off.out.non_colliding < B     # the footprint decides rollouts, not all
    cfg, scn, noise = wall_case(B, T)
    g = setup(Smpc(cfg), scn, list_critics(which), noise)
    ug, og = g.optimize(scn.tick, scn.u0)
    assert last_kernel(g) == wave_at(T, 4)
    check(g, ug, og, on, f"footprint lean {which} {B}x{T}")
    g.close()


@pytest.mark.parametrize("which", ["deployed", "five"])
def test_parity_near_the_goal(Smpc, which):
    ref = oracle_tick(which, 256, 56, near_goal=True)
    cfg, scn, noise = wall_case(256, 56, near_goal=True)
    g = setup(Smpc(cfg), scn, list_critics(which), noise)
    ug, og = g.optimize(scn.tick, scn.u0)
    assert last_kernel(g) == "smpc_pass<1, 4, false>"
    check(g, ug, og, ref, f"footprint lean {which} near goal")
    g.close()


# ---- 3. both routes on the same tick ---------------------------------------------------------

@pytest.mark.parametrize("B,T", [(256, 56), (128, 100)])
def test_lean_and_general_route_agree(Smpc, monkeypatch, B, T):
    """Both routes run the same rollout code and read the same cells: the integer outputs are
    equal.  The per-rollout costs differ by the order of a float sum; the difference is recorded
    here, and each route's costs are bounded on their own, rollout by rollout against an exact
    model with no flip allowance, in tests/test_gpu_footprint_walk.py."""
    ref = oracle_tick("deployed", B, T)
    cfg, scn, noise = wall_case(B, T)
    res = {}
    for route in ("lean", "general"):
        g = general_route(Smpc, monkeypatch, cfg) if route == "general" else Smpc(cfg)
        setup(g, scn, list_critics("deployed"), noise)
        u, out = g.optimize(scn.tick, scn.u0)
        assert last_kernel(g) == wave_at(T, 4 if route == "lean" else 2)
        check(g, u, out, ref, f"{route} route {B}x{T}")
        res[route] = keep(u, out, g.get_costs())
        g.close()
    a, b = res["lean"], res["general"]
    assert a.out.non_colliding == b.out.non_colliding and a.out.fail_flag == b.out.fail_flag
    assert a.out.furthest_reached_path_point == b.out.furthest_reached_path_point
    d = np.abs(a.costs.astype(np.float64) - b.costs) / np.maximum(np.abs(b.costs), 1e-30)
    print(f"[footprint] {B}x{T} lean vs general route: largest relative cost difference {float(d.max()):.3e}, "
          f"control sequence {rel_err(a.u, b.u):.3e}")


# ---- 4. second passes -------------------------------------------------------------------------

def test_speculation_miss_and_two_pass_mode(Smpc, Oracle):
    """A plan with twice the spacing halves every endpoint's nearest-point index: the speculated
    pass misses and the tick is scored again, on the same instance.  SMPC_FLAG_NO_SPECULATION: the
    furthest-only pass in front of every tick instead."""
    cfg, scn, noise = wall_case(256, 56)
    g = setup(Smpc(cfg), scn, list_critics("deployed"), noise)
    o = setup(Oracle(cfg), scn, list_critics("deployed"), noise)
    g.optimize(scn.tick, scn.u0)
    t = scn.tick
    px = (t.pose_x + 0.1 * np.arange(len(t.path_x))).astype(np.float32)
    tick2 = Tick(t.pose_x, t.pose_y, t.pose_yaw, t.speed, px, t.path_y, t.path_yaw, float(px[-1]), t.goal_y)
    ug, og = g.optimize(tick2, scn.u0)
    uo, oo = o.optimize(tick2, scn.u0)
    ref = keep(uo, oo, o.get_costs())
    assert og.passes > cfg.iteration_count and last_kernel(g) == "smpc_pass<1, 4, false>"
    check(g, ug, og, ref, "speculation miss")
    g.close()
    cfg2, _, _ = wall_case(256, 56)
    cfg2.flags |= A.SMPC_FLAG_NO_SPECULATION
    g2 = setup(Smpc(cfg2), scn, list_critics("deployed"), noise)
    for _ in range(2):
        ug2, og2 = g2.optimize(tick2, scn.u0)
        assert og2.passes == 1 and last_kernel(g2) == "smpc_pass<1, 4, false>"
        check(g2, ug2, og2, ref, "two-pass mode")
    g2.close()


@pytest.mark.parametrize("which", ["deployed", "five"])
def test_two_iterations(Smpc, Oracle, which):
    cfg, scn, noise = wall_case(256, 56)
    cfg.iteration_count = 2
    g = setup(Smpc(cfg), scn, list_critics(which), noise)
    o = setup(Oracle(cfg), scn, list_critics(which), noise)
    ug, og = g.optimize(scn.tick, scn.u0)
    uo, oo = o.optimize(scn.tick, scn.u0)
    assert og.passes == 2 and last_kernel(g) == "smpc_pass<1, 4, false>"
    assert 0 < oo.non_colliding < 256
    check(g, ug, og, keep(uo, oo, o.get_costs()), f"two iterations {which}")
    g.close()


@pytest.mark.parametrize("which", ["deployed", "five"])
def test_every_footprint_collides(Smpc, Oracle, which):
    """Walls on both sides under the outline, never under a centre that keeps to the path: the
    tick fails because of the footprint alone, and the re-score of what the reference had scored
    when its manager stopped (critic_manager.cpp:70-73) runs the same instance with the footprint.
    Bounds as in test_gpu_parity.py::test_all_collide_with_a_footprint_is_rescored_with_the_footprint
    and ::test_both_collision_critics_with_a_footprint: every rollout sits at the collision cost,
    the costs agree to 2e-6 relative, the softmax weights hang on their last ulp."""
    cfg, scn, noise = wall_case(256, 56, closed_in=True)
    g = setup(Smpc(cfg), scn, list_critics(which), noise)
    o = setup(Oracle(cfg), scn, list_critics(which), noise)
    ug, og = g.optimize(scn.tick, scn.u0)
    uo, oo = o.optimize(scn.tick, scn.u0)
    assert oo.fail_flag == 1 and oo.non_colliding == 0
    assert og.fail_flag == 1 and og.non_colliding == 0
    assert og.passes == 2 and last_kernel(g) == "smpc_pass<1, 4, false>"
    cg, co = g.get_costs().astype(np.float64), o.get_costs().astype(np.float64)
    assert np.max(np.abs(cg - co)) <= 2e-6 * float(np.max(np.abs(co))), (cg[:4], co[:4])
    assert rel_err(ug, uo) < 1e-3
    # without the footprint the same tick does not fail
    o.set_critics(list_critics(which, footprint=False))
    _, o2 = o.optimize(scn.tick, scn.u0)
    assert o2.fail_flag == 0 and o2.non_colliding > 0
    g.close()


# ---- 5. closed loop -----------------------------------------------------------------------------

def test_closed_loop_of_three_ticks(Smpc, Oracle):
    cfg, scn, noise = wall_case(256, 56)
    g = setup(Smpc(cfg), scn, list_critics("deployed"), noise)
    o = setup(Oracle(cfg), scn, list_critics("deployed"), noise)
    t, u = scn.tick, scn.u0
    for k in range(3):
        tick = Tick(t.pose_x + 0.015 * k, t.pose_y, t.pose_yaw, t.speed, t.path_x, t.path_y, t.path_yaw,
                    t.goal_x, t.goal_y)
        ug, og = g.optimize(tick, u)
        uo, oo = o.optimize(tick, u)
        assert last_kernel(g) == "smpc_pass<1, 4, false>"
        assert 0 < oo.non_colliding < 256
        check(g, ug, og, keep(uo, oo, o.get_costs()), f"closed loop tick {k}")
        u = np.concatenate([ug[:, 1:], ug[:, -1:]], axis=1)      # the GPU's shifted sequence to both sides
    g.close()


# ---- 6. emulated shards -------------------------------------------------------------------------

def test_two_emulated_shards_match_the_single_tick(Smpc):
    """Bars of test_gpu_sharded.py::test_emulated_shards_match_unsharded."""
    import torch
    from mpcholonavigation_amd.tick import default_config
    B, T, G = 256, 56, 2
    ref = oracle_tick("deployed", B, T)
    cfg, scn, noise = wall_case(B, T)
    whole = setup(Smpc(cfg), scn, list_critics("deployed"), noise)
    u_w, out_w = whole.optimize(scn.tick, scn.u0)
    shards = []
    for a in (0, 128):
        c = default_config(batch_size=128, time_steps=T, shard_offset=a, global_batch_size=B)
        shards.append(setup(Smpc(c), scn, list_critics("deployed"), [n[a:a + 128] for n in noise]))
    L = shards[0].tuple_len
    t_f = torch.zeros(G, dtype=torch.float32, device="cuda")
    t_all = torch.zeros(G * L, dtype=torch.float32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    for s in shards:
        s.set_stream(stream)
        s.shard_begin(scn.tick, scn.u0)
    for i, s in enumerate(shards):
        s.shard_furthest(t_f[i:].data_ptr())
    t_max = t_f.max().reshape(1).contiguous()         # stands in for all_reduce(MAX)
    for i, s in enumerate(shards):
        s.shard_score(t_max.data_ptr(), 0, t_all[i * L:].data_ptr())
        assert last_kernel(s) == "smpc_pass<1, 4, false>"
    u_s, out_s = shards[0].shard_combine(t_all.data_ptr(), G)
    assert out_s.furthest_reached_path_point == out_w.furthest_reached_path_point
    assert out_s.non_colliding == out_w.non_colliding == ref.out.non_colliding
    assert rel_err(u_s, u_w) < 2e-6        # same kernels, different reduction tree
    assert_parity(u_s, out_s, ref.u, ref.out, label="2 shards vs oracle")
    for s in shards + [whole]:
        s.close()


# ---- 7. the host optimizer's face -------------------------------------------------------------

DEPLOYED_CLASSES = ["ConstraintCritic", "CostCritic", "GoalCritic", "GoalAngleCritic", "PathAlignCritic",
                    "PathFollowCritic", "PathAngleCritic", "PreferForwardCritic", "TwirlingCritic"]


def test_host_optimizer_takes_a_footprint(Smpc):
    """Optimizer.set_footprint (sortham_optimizer_set_footprint): the first eval_control from a zero
    control sequence is the tick Smpc.optimize runs on the same inputs and noise — the same library
    and the same kernel, so the same bits.  It survives initialize(); without it the tick fails."""
    from mpcholonavigation_amd.host_optimizer import Optimizer
    cfg, scn, noise = wall_case(256, 56)
    cr = list_critics("deployed")
    g = setup(Smpc(cfg), scn, cr, noise)
    _, og = g.optimize(scn.tick, np.zeros_like(scn.u0))

    def host_tick(h, footprint):
        if footprint:
            h.set_footprint(FOOTPRINT, CIRCUMSCRIBED, LAYER_SCALING)
        h.set_costmap(scn.cells, scn.origin_x, scn.origin_y, scn.resolution)
        h.set_noise(*noise)
        return h.eval_control(scn.tick)[1]

    h = Optimizer(cfg, cr, 20.0, critics=DEPLOYED_CLASSES)
    oh = host_tick(h, True)
    assert last_kernel(g) == "smpc_pass<1, 4, false>"
    assert (oh.non_colliding, oh.fail_flag, oh.min_cost) == (og.non_colliding, og.fail_flag, og.min_cost)
    assert 0 < oh.non_colliding < oracle_tick("deployed", 256, 56, footprint=False).out.non_colliding
    # a rebuilt context (another batch size) and then the first shape again: the footprint stays
    cfg_b, _, noise_b = wall_case(128, 56)
    h.initialize(cfg_b, cr, 20.0, critics=DEPLOYED_CLASSES)
    h.set_costmap(scn.cells, scn.origin_x, scn.origin_y, scn.resolution)
    h.set_noise(*noise_b)
    h.eval_control(scn.tick)
    h.initialize(cfg, cr, 20.0, critics=DEPLOYED_CLASSES)
    oh2 = host_tick(h, False)
    assert (oh2.non_colliding, oh2.fail_flag, oh2.min_cost) == (oh.non_colliding, oh.fail_flag, oh.min_cost)
    h.close()
    h0 = Optimizer(cfg, cr, 20.0, critics=DEPLOYED_CLASSES)
    with pytest.raises(RuntimeError, match="smpc_set_footprint"):
        host_tick(h0, False)
    h0.close()
    g.close()
