"""Acceleration limits on the sampled controls (smpc_set_acceleration_limits) on the GPU.

The yardstick is the unchanged library: context A has the limits and the stored noise N; its twin B
has no limits and is given smpc_set_noise(N'_model), N'_model the limited noise of
tests/accel_model.py for the tick's u and speed.  A tick of A equals a tick of B bit for bit, on
every scoring pass; smpc_get_limited_noise equals the model bit for bit.  Every existing parity
test already holds B to the oracle.

Scenes: make_case's scene (and the wall scene for the collision critics), the speed and the incoming
control sequence non-zero on every control; limits 3 / -3 / 3 / 3.5 at model_dt 0.05 with the
default standard deviations, on which tests/test_accel_limits_cpu.py counts more than 10 % of the
elements limited."""
import numpy as np
import pytest

from mpcholonavigation_amd import _abi as A
from mpcholonavigation_amd.synthetic import make_noise, wall_beside_path
from mpcholonavigation_amd.tick import Tick, default_config
from tests import accel_model as am
from tests.footprint_scenes import classes, critics_of, list_critics, setup
from tests.harness import FIVE, LANE, OUT_FIELDS, bits, close, last_kernel, mod  # noqa: F401
from tests.helpers import make_case, rel_err

pytestmark = pytest.mark.gpu

LIM = (3.0, -3.0, 3.0, 3.5)
SPEED = (0.25, 0.05, -0.1)


def same_noise(got, want, label):
    for k, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(bits(g), bits(w)), (label, k, int(np.sum(bits(g) != bits(w))))


def with_speed(t, speed=SPEED, dx=0.0):
    return Tick(t.pose_x + dx, t.pose_y, t.pose_yaw, speed, t.path_x, t.path_y, t.path_yaw, t.goal_x, t.goal_y)


def warm_u(scn, T):
    """The scene's incoming sequence with something on every control."""
    t = np.arange(T, dtype=np.float32)
    u = np.array(scn.u0, np.float32)
    u[0] += 0.02 * np.sin(0.4 * t)
    u[1] += 0.03 * np.cos(0.3 * t)
    u[2] += 0.1 * np.sin(0.2 * t)
    return u.astype(np.float32)


def case(B, T, flags=0, wall=False, model=A.SMPC_MODEL_OMNI, **cfg_kw):
    cfg, scn, noise = make_case(B, T)
    cfg.flags |= flags
    cfg.motion_model = model
    for k, v in cfg_kw.items():
        setattr(cfg, k, v)
    if wall:
        scn.cells = wall_beside_path(scn)
    holo = model == A.SMPC_MODEL_OMNI
    tick = with_speed(scn.tick, SPEED if holo else (SPEED[0], 0.0, SPEED[2]))
    u0 = warm_u(scn, T)
    if not holo:
        u0[1] = 0.0
        noise = (noise[0], np.zeros_like(noise[1]), noise[2])
    return cfg, scn, noise, tick, u0


def model_noise(cfg, noise, u, tick, limits=LIM):
    return am.limited_noise(noise, u, tick.speed, cfg.model_dt, limits, holonomic=cfg.motion_model == A.SMPC_MODEL_OMNI)


def ctx(mod, cfg, scn, noise, cr=None, limits=None, footprint=False):
    g = setup(mod.Smpc(cfg), scn, cr if cr is not None else critics_of(FIVE), noise, footprint)
    if limits is not None:
        g.set_acceleration_limits(*limits)
    return g


def same_tick(ga, gb, ra, rb, label, skip=()):
    (ua, oa), (ub, ob) = ra, rb
    assert np.array_equal(bits(ua), bits(ub)), label
    for f in OUT_FIELDS:
        if f in skip:
            continue
        assert getattr(oa, f) == getattr(ob, f), (label, f, getattr(oa, f), getattr(ob, f))
    assert np.array_equal(bits(ga.get_costs()), bits(gb.get_costs())), label


# ---- 1. the kernel against the model -----------------------------------------------------------

@pytest.mark.parametrize("B,T,flags,kind", [(200, 30, 0, 0), (512, 128, 0, 0), (4100, 64, LANE, 1), (16384, 64, 0, 2)])
def test_limited_noise_is_the_models(mod, B, T, flags, kind):
    cfg, scn, noise, tick, u0 = case(B, T, flags)
    g = ctx(mod, cfg, scn, noise, limits=LIM)
    assert g.get_acceleration_limits() == LIM
    _, out = g.optimize(tick, u0)
    assert out.pass_kind == kind, last_kernel(g)
    want = model_noise(cfg, noise, u0, tick)
    share = [float(np.mean(w != n)) for w, n in zip(want, noise)]
    print(f"[accel] {B}x{T} kernel {last_kernel(g)}: limited share {share}")
    assert min(share) >= 0.10
    same_noise(g.get_limited_noise(), want, f"{B}x{T}")
    # the second tick speculates on the furthest point: no pre-pass, so a lane or split context limits
    # the group-major layout only and the [B,T] answer is made from that
    _, out = g.optimize(tick, u0)
    assert out.pass_kind == kind, last_kernel(g)
    same_noise(g.get_limited_noise(), want, f"{B}x{T} second tick")
    same_noise(g.get_noise(), noise, "the stored noise")
    g.close()


# ---- 2. A == B on every scoring pass --------------------------------------------------------------

F, Tr = False, True
PASSES = [
    # (id, B, T, flags, critics, footprint, wall, model, cfg, environment, pass_kind, kernel prefix)
    ("wave-lean", 2000, 56, 0, FIVE, F, F, A.SMPC_MODEL_OMNI, {}, {}, 0, "smpc_pass<1, 0, false>"),
    ("wave-deployed-footprint", 2000, 56, 0, "deployed", Tr, Tr, A.SMPC_MODEL_OMNI, {}, {}, 0, "smpc_pass<1, 4, false>"),
    ("wave-general-traj", 500, 64, A.SMPC_FLAG_STORE_TRAJECTORIES, "power2", F, Tr, A.SMPC_MODEL_OMNI, {}, {}, 0,
     "smpc_pass<1, 2, true>"),
    ("lane", 4096, 64, LANE, FIVE, F, F, A.SMPC_MODEL_OMNI, {}, {}, 1, "smpc_pass_lane<true, true, false, 1, false,"),
    ("lane-reread", 4096, 128, LANE, FIVE, F, F, A.SMPC_MODEL_OMNI, {}, {}, 1, "smpc_pass_lane<true, true, false, 2, true,"),
    ("split", 16384, 64, 0, FIVE, F, F, A.SMPC_MODEL_OMNI, {}, {}, 2, "smpc_pass_split<4, true>"),
    ("lane-nh-diffdrive", 61440, 64, 0, FIVE, F, F, A.SMPC_MODEL_DIFF_DRIVE, {}, {}, 1, "smpc_pass_lane_nh<"),
    ("wave-ackermann", 1000, 56, 0, FIVE, F, F, A.SMPC_MODEL_ACKERMANN, {}, {}, 0, "smpc_pass<1, 0, false>"),
]


@pytest.mark.parametrize("c", PASSES, ids=[c[0] for c in PASSES])
def test_limited_tick_equals_the_twin_fed_the_models_noise(mod, monkeypatch, c):
    name, B, T, flags, names, footprint, wall, model, cfg_kw, env, kind, kernel = c
    cfg, scn, noise, tick, u0 = case(B, T, flags, wall=wall, model=model, **cfg_kw)
    if names == "deployed":
        cr = list_critics("deployed", footprint)
    elif names == "power2":
        cr = critics_of(FIVE, power=2)
    else:
        cr = critics_of(names)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    ga = ctx(mod, cfg, scn, noise, cr, LIM, footprint)
    gb = ctx(mod, cfg, scn, model_noise(cfg, noise, u0, tick), cr, None, footprint)
    ra = ga.optimize(tick, u0)
    ka = last_kernel(ga)
    rb = gb.optimize(tick, u0)
    kb = last_kernel(gb)
    print(f"[accel] {name}: kernel {ka}, pass_kind {ra[1].pass_kind}, non_colliding {ra[1].non_colliding} of {B}")
    assert ra[1].pass_kind == kind and ka.startswith(kernel) and ka == kb, (name, ka, kb)
    same_tick(ga, gb, ra, rb, name)
    if flags & A.SMPC_FLAG_STORE_TRAJECTORIES:
        for ta, tb in zip(ga.get_generated_trajectories(), gb.get_generated_trajectories()):
            assert np.array_equal(bits(ta), bits(tb)), name
    if model != A.SMPC_MODEL_OMNI:
        assert not ga.get_limited_noise()[1].any(), name
    # the limits decided something: the unlimited tick is another tick
    gc = ctx(mod, cfg, scn, noise, cr, None, footprint)
    uc, _ = gc.optimize(tick, u0)
    assert not np.array_equal(bits(uc), bits(ra[0])), name
    close(ga, gb, gc)


# ---- 3. wide limits -------------------------------------------------------------------------------

@pytest.mark.parametrize("B,T,flags,kind", [(2000, 56, 0, 0), (4096, 64, LANE, 1)])
def test_wide_limits_are_the_unlimited_tick_over_a_closed_loop(mod, B, T, flags, kind):
    cfg, scn, noise, tick, u0 = case(B, T, flags)
    ga = ctx(mod, cfg, scn, noise, limits=(1e6, -1e6, 1e6, 1e6))
    gb = ctx(mod, cfg, scn, noise)
    ua, ub = u0, u0
    for k in range(10):
        t = with_speed(scn.tick, dx=0.015 * k)
        ra, rb = ga.optimize(t, ua), gb.optimize(t, ub)
        assert ra[1].pass_kind == kind
        same_tick(ga, gb, ra, rb, f"{B}x{T} tick {k}")
        ua, ub = ra[0], rb[0]
    same_noise(ga.get_limited_noise(), noise, "wide limits")
    close(ga, gb)


# ---- 4. two iterations ------------------------------------------------------------------------------

@pytest.mark.parametrize("B,T,flags", [(2000, 56, 0), (4096, 64, LANE)])
def test_the_second_iteration_limits_against_its_own_u(mod, B, T, flags):
    cfg, scn, noise, tick, u0 = case(B, T, flags)
    gc = ctx(mod, cfg, scn, noise, limits=LIM)
    u1, _ = gc.optimize(tick, u0)
    cfg2, *_ = case(B, T, flags, iteration_count=2)
    ga = ctx(mod, cfg2, scn, noise, limits=LIM)
    ga.optimize(tick, u0)
    assert not np.array_equal(u1, u0)
    same_noise(ga.get_limited_noise(), model_noise(cfg, noise, u1, tick), f"{B}x{T} iteration 1")
    close(ga, gc)


# ---- 5. smpc_critic_breakdown -----------------------------------------------------------------------

STATS = ("scored_mask", "fail_flag", "batch", "best_rollout", "best_cost", "effective_samples")
ROWS = ("sum", "min", "max", "weighted", "at_best", "per_rollout")


@pytest.mark.parametrize("B,T,flags,kind", [(2000, 56, 0, 0), (4096, 64, LANE, 1)])
def test_breakdown_reads_the_limited_noise(mod, B, T, flags, kind):
    cfg, scn, noise, tick, u0 = case(B, T, flags)
    ga = ctx(mod, cfg, scn, noise, limits=LIM)
    gb = ctx(mod, cfg, scn, model_noise(cfg, noise, u0, tick))
    # (the lane context: before any tick, so its [B,T] limited buffer exists only because of this call)
    sa, sb = ga.critic_stats(tick, u0, per_rollout=True), gb.critic_stats(tick, u0, per_rollout=True)
    for f in STATS:
        assert getattr(sa, f) == getattr(sb, f), f
    for f in ROWS:
        assert np.array_equal(bits(getattr(sa, f)), bits(getattr(sb, f))), f
    same_noise(ga.get_limited_noise(), model_noise(cfg, noise, u0, tick), "after the breakdown")
    # a ten-tick loop: the same bits with and without a breakdown in front of every tick
    gp = ctx(mod, cfg, scn, noise, limits=LIM)
    ua, up = u0, u0
    for k in range(10):
        t = with_speed(scn.tick, dx=0.015 * k)
        ga.critic_stats(t, ua)
        ra, rp = ga.optimize(t, ua), gp.optimize(t, up)
        assert ra[1].pass_kind == kind
        same_tick(ga, gp, ra, rp, f"{B}x{T} tick {k}")
        ua, up = ra[0], rp[0]
    close(ga, gb, gp)


# ---- 6. groups ------------------------------------------------------------------------------------

def test_group_members_with_limits_equal_their_solo_contexts(mod):
    B, T = 2000, 56
    limits = [None, LIM, (1.5, -2.0, 1.0, 2.5)]
    members, solos = [], []
    for i, lim in enumerate(limits):
        cfg, scn, _, tick, u0 = case(B, T)
        noise = make_noise(B, T, std=(cfg.vx_std, cfg.vy_std, cfg.wz_std), seed=900 + i)
        members.append(ctx(mod, cfg, scn, noise, limits=lim))
        solos.append(ctx(mod, cfg, scn, noise, limits=lim))
    grp = mod.SmpcGroup(members)
    us, ut = [u0] * 3, [u0] * 3
    for k in range(5):
        t = with_speed(scn.tick, dx=0.015 * k)
        before = grp.stats()
        res = grp.optimize([t] * 3, us)
        after = grp.stats()
        for i in range(3):
            rt = solos[i].optimize(t, ut[i])
            # (passes: a member scored again on its own after a missed prediction counts the batched pass too)
            same_tick(members[i], solos[i], (res[i][0], res[i][1]), rt, f"round {k} member {i}", skip=("passes",))
            if limits[i] is not None:
                same_noise(members[i].get_limited_noise(), solos[i].get_limited_noise(), f"round {k} member {i}")
            ut[i] = rt[0]
        us = [r[0] for r in res]
        print(f"[accel] group round {k}: batched +{after.batched_launches - before.batched_launches}, "
              f"single +{after.single_ticks - before.single_ticks}, passes {[o.passes for _, o in res]}")
        if k >= 2:
            assert after.batched_launches > before.batched_launches, k
    grp.close()
    close(*members, *solos)


# ---- 7. shards ------------------------------------------------------------------------------------

def test_two_emulated_shards_with_limits_reproduce_the_unsharded_tick(mod):
    import torch
    B, T, G = 4096, 64, 2
    cfg, scn, noise, tick, u0 = case(B, T)
    whole = ctx(mod, cfg, scn, noise, limits=LIM)
    u_w, out_w = whole.optimize(tick, u0)
    cuts = np.linspace(0, B, G + 1).astype(int)
    shards = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        c2 = default_config(batch_size=int(b - a), time_steps=T, shard_offset=int(a), global_batch_size=B)
        shards.append(ctx(mod, c2, scn, [n[a:b] for n in noise], limits=LIM))
    dev = torch.device("cuda", 0)
    L = shards[0].tuple_len
    t_f = torch.zeros(G, dtype=torch.float32, device=dev)
    t_all = torch.zeros(G * L, dtype=torch.float32, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    for s in shards:
        s.set_stream(stream)
        s.shard_begin(tick, u0)
    for g, s in enumerate(shards):
        s.shard_furthest(t_f[g:].data_ptr())
    t_max = t_f.max().reshape(1).contiguous()
    for g, s in enumerate(shards):
        s.shard_score(t_max.data_ptr(), 0, t_all[g * L:].data_ptr())
    u_s, out_s = shards[0].shard_combine(t_all.data_ptr(), G)
    assert out_s.furthest_reached_path_point == out_w.furthest_reached_path_point
    assert out_s.non_colliding == out_w.non_colliding
    # (the bar of tests/test_gpu_sharded.py::test_emulated_shards_match_unsharded for the same comparison)
    assert rel_err(u_s, u_w) < 2e-6
    want = model_noise(cfg, noise, u0, tick)
    for s, a, b in zip(shards, cuts[:-1], cuts[1:]):
        same_noise(s.get_limited_noise(), [w[a:b] for w in want], f"shard {a}:{b}")
    close(whole, *shards)


# ---- 8. noise lifecycle ---------------------------------------------------------------------------

@pytest.mark.parametrize("B,T,flags", [(2000, 56, 0), (4096, 64, LANE)])
def test_the_limiter_follows_the_noise_the_tick_scores_with(mod, B, T, flags):
    cfg, scn, noise, tick, u0 = case(B, T, flags)
    g = ctx(mod, cfg, scn, None, limits=LIM)
    g.seed(77)
    g.optimize(tick, u0)
    n0 = g.get_noise()
    same_noise(g.get_limited_noise(), model_noise(cfg, n0, u0, tick), "seeded")
    g.redraw_noise_async()
    g.optimize(tick, u0)
    n1 = g.get_noise()
    assert not np.array_equal(n1[0], n0[0])
    same_noise(g.get_limited_noise(), model_noise(cfg, n1, u0, tick), "after redraw_noise_async")
    g.set_noise(*noise)
    g.optimize(tick, u0)
    same_noise(g.get_limited_noise(), model_noise(cfg, noise, u0, tick), "after set_noise")
    same_noise(g.get_noise(), noise, "get_noise is N itself")
    g.reset()
    assert g.get_acceleration_limits() == LIM
    g.close()


# ---- 9. host ----------------------------------------------------------------------------------------

def host(cfg, scn, noise, limits=None):
    from mpcholonavigation_amd.host_optimizer import Optimizer
    h = Optimizer(cfg, critics_of(FIVE), 20.0, critics=classes(FIVE), cost_scaling_factor=scn.cost_scaling_factor,
                  inflation_radius=scn.inflation_radius)
    h.set_costmap(scn.cells, scn.origin_x, scn.origin_y, scn.resolution, inscribed_radius=scn.inscribed_radius)
    h.set_noise(*noise)
    if limits is not None:
        h.set_acceleration_limits(*limits)
    return h


def host_loop(ha, hb, cfg, scn, noise, n, label):
    """ha has the limits and N; hb is fed the model's limited noise for its own u before every tick."""
    for k in range(n):
        t = with_speed(scn.tick, dx=0.015 * k)
        hb.set_noise(*model_noise(cfg, noise, hb.get_control_sequence(), t))
        (tw_a, oa), (tw_b, ob) = ha.eval_control(t), hb.eval_control(t)
        assert np.array_equal(tw_a, tw_b), (label, k)
        assert np.array_equal(bits(ha.get_control_sequence()), bits(hb.get_control_sequence())), (label, k)
        # (not `passes`: noise set before every tick makes the twin's furthest-point predictor treat each
        # tick as one on fresh noise, so the two may re-score on different ticks; the results are exact)
        for f in OUT_FIELDS:
            if f != "passes":
                assert getattr(oa, f) == getattr(ob, f), (label, k, f)


def test_host_optimizer_carries_the_limits(mod):
    cfg, scn, noise, _, _ = case(2000, 56)
    ha, hb = host(cfg, scn, noise, LIM), host(cfg, scn, noise)
    host_loop(ha, hb, cfg, scn, noise, 10, "closed loop")
    # the limits survive reset(): the loop again from a zero sequence, the twin still fed the model's noise
    ha.reset()
    hb.reset()
    ha.set_noise(*noise)
    host_loop(ha, hb, cfg, scn, noise, 3, "after reset")
    hc = host(cfg, scn, noise)
    tw_c, _ = hc.eval_control(with_speed(scn.tick))
    hd = host(cfg, scn, noise, LIM)
    tw_d, _ = hd.eval_control(with_speed(scn.tick))
    assert not np.array_equal(tw_c, tw_d)
    close(ha, hb, hc, hd)


def test_fleet_member_with_limits_equals_its_solo_twin(mod):
    from mpcholonavigation_amd.host_optimizer import FleetOptimizer
    B, T = 256, 56
    cfg, scn, _, _, _ = case(B, T)
    limits = [LIM, None, (1.5, -2.0, 1.0, 2.5)]
    noises = [make_noise(B, T, std=(cfg.vx_std, cfg.vy_std, cfg.wz_std), seed=700 + i) for i in range(3)]
    members = [host(cfg, scn, noises[i], limits[i]) for i in range(3)]
    twins = [host(cfg, scn, noises[i], limits[i]) for i in range(3)]
    fleet = FleetOptimizer(members)
    for k in range(5):
        t = with_speed(scn.tick, dx=0.015 * k)
        res = fleet.eval_control([t] * 3)
        for i in range(3):
            tw_t, out_t = twins[i].eval_control(t)
            assert res[i].status == 0 and np.array_equal(res[i].twist, tw_t), (k, i)
            assert np.array_equal(bits(members[i].get_control_sequence()), bits(twins[i].get_control_sequence())), (k, i)
            for f in ("fail_flag", "furthest_valid", "furthest_reached_path_point", "non_colliding", "min_cost", "sum_w"):
                assert getattr(res[i].out, f) == getattr(out_t, f), (k, i, f)
    fleet.close()
    close(*members, *twins)


# ---- 10. refusals -----------------------------------------------------------------------------------

def test_refusals_and_switching_off(mod):
    cfg, scn, noise, tick, u0 = case(2000, 56)
    g = ctx(mod, cfg, scn, noise)
    bad = [(3.0, 3.0, 3.0, 3.5), (-3.0, -3.0, 3.0, 3.5), (3.0, -3.0, -3.0, 3.5), (3.0, -3.0, 3.0, -3.5),
           (3.0, -3.0, 3.0, 0.0), (0.0, -3.0, 3.0, 3.5), (float("nan"), -3.0, 3.0, 3.5), (3.0, -3.0, float("inf"), 3.5),
           (3.0, float("-inf"), 3.0, 3.5)]
    for lim in bad:
        with pytest.raises(mod.SmpcError) as e:
            g.set_acceleration_limits(*lim)
        assert e.value.code == A.SMPC_ERR_INVALID, lim
    assert g.get_acceleration_limits() == (0.0, 0.0, 0.0, 0.0)
    with pytest.raises(mod.SmpcError) as e:
        g.get_limited_noise()                      # limits off
    assert e.value.code == A.SMPC_ERR_STATE
    g.set_acceleration_limits(*LIM)
    with pytest.raises(mod.SmpcError) as e:
        g.get_limited_noise()                      # no tick yet
    assert e.value.code == A.SMPC_ERR_STATE
    u1, _ = g.optimize(tick, u0)
    g.get_limited_noise()
    g.set_acceleration_limits(0.0, 0.0, 0.0, 0.0)  # off again: the next tick is the unlimited tick
    with pytest.raises(mod.SmpcError) as e:
        g.get_limited_noise()
    assert e.value.code == A.SMPC_ERR_STATE
    plain = ctx(mod, cfg, scn, noise)
    plain.optimize(tick, u0)
    ra, rb = g.optimize(tick, u0), plain.optimize(tick, u0)
    # (passes: the two predictors start from different ticks, so one may re-score where the other does not)
    same_tick(g, plain, ra, rb, "switched off", skip=("passes",))
    assert not np.array_equal(bits(u1), bits(ra[0]))
    close(g, plain)
