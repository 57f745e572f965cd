"""Moving obstacles (smpc_set_moving_obstacles) on the GPU.

The yardsticks: tests/moving_model.py for the term itself, on the oracle's trajectories; for
everything around it the unchanged library — the twin context without obstacles, whose costs every
existing parity test already holds to the oracle: a seeded tick's costs are m + the twin's, within
the float32 bound of adding n critics' terms onto a different start.

Measured on an MI355X (worst ratio of |m_device - m_model| to the bound derived in
moving_model.tolerance, over the eight cases of test_the_term_is_the_models): see DESIGN.md 7."""
import numpy as np
import pytest

from mpcholonavigation_amd import _abi as A
from mpcholonavigation_amd.synthetic import make_noise
from mpcholonavigation_amd.tick import Tick, default_config
from tests import accel_model as am
from tests import moving_model as mm
from tests import moving_scenes as ms
from tests import softmax_model as sm
from tests.footprint_scenes import classes, critics_of
from tests.harness import (FIVE, LANE, OUT_FIELDS, Smpc, bits, close, create_with_env, last_kernel, mod,  # noqa: F401
                           moved)
from tests.helpers import make_case, rel_err

pytestmark = pytest.mark.gpu

EPS = mm.EPS
LIM = (3.0, -3.0, 3.0, 3.5)


def sum_bound(n, m, magnitude):
    """The issue's bound, the one the stats rows are held to (tests/test_gpu_critic_stats.py): costs
    that start from m and add n terms in float32 against m + the float64 sum of those terms:
    (n + 1) * 2^-24 * (|m| + sum |t_k|).  magnitude: sum |t_k| where the rows of a breakdown give it,
    else |the twin's cost|, which is no larger (|sum t_k| <= sum |t_k|): the stricter bound."""
    return (n + 1) * EPS * (np.abs(m) + np.abs(magnitude)) + 1e-30


def seeded_equals_twin(g, twin, n, label):
    m, hit = g.moving_obstacle_costs()
    c, ct = g.get_costs().astype(np.float64), twin.get_costs().astype(np.float64)
    err = np.abs(c - (m.astype(np.float64) + ct))
    bound = sum_bound(n, m.astype(np.float64), ct)
    print(f"[moving] {label}: worst cost error / bound {float((err / bound).max()):.3f}, m up to {float(m.max()):.3f}, "
          f"hits {int(hit.sum())} of {len(hit)}")
    assert np.all(err <= bound), (label, float((err / bound).max()))
    return m, hit


def same_tick(ga, gb, ra, rb, label, skip=()):
    (ua, oa), (ub, ob) = ra, rb
    assert np.array_equal(bits(ua), bits(ub)), label
    for f in OUT_FIELDS:
        if f not in skip:
            assert getattr(oa, f) == getattr(ob, f), (label, f, getattr(oa, f), getattr(ob, f))
    assert np.array_equal(bits(ga.get_costs()), bits(gb.get_costs())), label


def row(c):
    name, B, T, flags, names, footprint, wall, model, kind, kernel = c
    cfg, scn, noise, tick, u0 = ms.pass_case(B, T, flags, wall=wall, model=model)
    cr, n = ms.pass_critics(names, footprint)
    return name, cfg, scn, noise, tick, u0, cr, n, footprint, kind, kernel


def across(cfg, tick, K=3, seed=11):
    return mm.make_discs(tick, cfg.time_steps, cfg.model_dt, K, seed, side=0.6, radius=(0.05, 0.15))


# ---- 2. the term against the model ---------------------------------------------------------------------

@pytest.mark.parametrize("B,T,flags,kind", ms.TERM_SHAPES)
@pytest.mark.parametrize("K", ms.TERM_K)
def test_the_term_is_the_models(mod, B, T, flags, kind, K):
    cfg, scn, noise, xy, radius = ms.term_case(B, T, flags, K)
    g = ms.context(mod, cfg, scn, noise, critics_of(FIVE), discs=(xy, radius), params=ms.TERM_PARAMS)
    want = ms.term_model(B, T, flags, K)
    tol = mm.tolerance(want, T, K, ms.TERM_PARAMS["repulsion_weight"], ms.TERM_PARAMS["margin"])
    assert float(want.near.mean()) <= ms.NEAR_CAP
    first = None
    for tick_no in range(2):     # (the second tick speculates: no pre-pass in front of the seed kernel)
        _, out = g.optimize(scn.tick, scn.u0)
        assert out.pass_kind == kind, last_kernel(g)
        m, hit = g.moving_obstacle_costs()
        same = hit == want.hit
        assert np.all(same | want.near), (int(np.sum(~same & ~want.near)), "hits differ away from the boundary")
        err = np.abs(m.astype(np.float64) - want.m)[same]
        ratio = float((err / tol[same]).max())
        print(f"[moving] {B}x{T} K={K} tick {tick_no} kernel {last_kernel(g)}: worst |m - model| / bound {ratio:.3f} "
              f"(worst error {float(err.max()):.3e}), hits {int(hit.sum())}, boundary rollouts {int(want.near.sum())}")
        assert ratio <= 1.0
        if first is None:
            first = (m, hit)
        else:     # one form on equal inputs: bit for bit
            assert np.array_equal(bits(m), bits(first[0])) and np.array_equal(hit, first[1])
    g.close()


def test_the_longest_horizon_and_a_ragged_batch(mod):
    """T = 256 (four steps per lane), B no multiple of four: the row-major form's third instance."""
    B, T, K = 101, 256, 5
    cfg, scn, noise = make_case(B, T)
    xy, radius = mm.make_discs(scn.tick, T, cfg.model_dt, K, 7, **ms.MANY_LONG)
    x, y = ms.oracle_trajectories(B, T)
    want = mm.costs(x, y, xy, radius, **ms.TERM_PARAMS)
    g = ms.context(mod, cfg, scn, noise, critics_of(FIVE), discs=(xy, radius), params=ms.TERM_PARAMS)
    g.optimize(scn.tick, scn.u0)
    m, hit = g.moving_obstacle_costs()
    same = hit == want.hit
    assert np.all(same | want.near) and float(want.near.mean()) <= 0.02
    tol = mm.tolerance(want, T, K, ms.TERM_PARAMS["repulsion_weight"], ms.TERM_PARAMS["margin"])
    ratio = float((np.abs(m - want.m)[same] / tol[same]).max())
    print(f"[moving] {B}x{T} K={K}: worst |m - model| / bound {ratio:.3f}, in reach {int((want.sum_q > 0).sum())}")
    assert ratio <= 1.0 and (want.sum_q > 0).any()
    g.close()


# ---- 3. out of reach: the parent's bits ------------------------------------------------------------------

@pytest.mark.parametrize("c", ms.PASSES, ids=[c[0] for c in ms.PASSES])
def test_out_of_reach_is_the_tick_without_obstacles(mod, c):
    name, cfg, scn, noise, tick, u0, cr, n, footprint, kind, kernel = row(c)
    ga = ms.context(mod, cfg, scn, noise, cr, footprint, discs=mm.far_discs(tick, cfg.time_steps, 4))
    gb = ms.context(mod, cfg, scn, noise, cr, footprint)
    ra, ka = ga.optimize(tick, u0), last_kernel(ga)
    rb, kb = gb.optimize(tick, u0), last_kernel(gb)
    assert ra[1].pass_kind == kind and ka.startswith(kernel) and ka == kb, (name, ka, kb)
    same_tick(ga, gb, ra, rb, name)
    m, hit = ga.moving_obstacle_costs()
    assert not m.any() and not hit.any()
    close(ga, gb)


# ---- 4. in reach -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", ms.PASSES, ids=[c[0] for c in ms.PASSES])
def test_in_reach_adds_m_to_the_twins_costs(mod, c):
    name, cfg, scn, noise, tick, u0, cr, n, footprint, kind, kernel = row(c)
    ga = ms.context(mod, cfg, scn, noise, cr, footprint, discs=across(cfg, tick))
    gb = ms.context(mod, cfg, scn, noise, cr, footprint)
    (ua, oa), ka = ga.optimize(tick, u0), last_kernel(ga)
    (ub, ob), kb = gb.optimize(tick, u0), last_kernel(gb)
    assert oa.pass_kind == kind and ka.startswith(kernel) and ka == kb, (name, ka, kb)
    m, hit = seeded_equals_twin(ga, gb, n, name)
    assert (m > 0).mean() > 0.5 and hit.any(), name
    # the term never declares a failure and does not enter the collision count
    assert oa.fail_flag == ob.fail_flag and oa.non_colliding == ob.non_colliding
    # the update on the device's own costs
    model = sm.update(ga.get_costs(), u0, noise, cfg, (cfg.vx_max, cfg.vx_min, cfg.vy_max, cfg.wz_max), cfg.motion_model)
    sm.judge(model, cfg.batch_size, ua, oa.min_cost, oa.sum_w, label=name)
    assert not np.array_equal(bits(ua), bits(ub)), name
    close(ga, gb)


# ---- 5. second passes see the same seed ------------------------------------------------------------------------

@pytest.mark.parametrize("B,T,flags", [(2000, 56, 0), (4096, 64, LANE)])
def test_a_speculation_miss_is_rescored_from_the_same_seed(mod, B, T, flags):
    cfg, scn, noise, tick, u0 = ms.pass_case(B, T, flags)
    cr = critics_of(FIVE)
    ga = ms.context(mod, cfg, scn, noise, cr, discs=across(cfg, tick))
    gb = ms.context(mod, cfg, scn, noise, cr)
    far = moved(tick, 0.6)
    for g in (ga, gb):
        g.optimize(tick, u0)
    ga.set_moving_obstacles(*across(cfg, far), **ms.PARAMS)
    (ua, oa), (ub, ob) = ga.optimize(far, u0), gb.optimize(far, u0)
    print(f"[moving] speculation {B}x{T}: passes {oa.passes} / {ob.passes}, furthest {oa.furthest_reached_path_point}")
    assert oa.passes == ob.passes == 2, "the moved pose was meant to miss the predicted furthest point"
    assert oa.furthest_reached_path_point == ob.furthest_reached_path_point
    seeded_equals_twin(ga, gb, len(FIVE), f"speculation miss {B}x{T}")
    close(ga, gb)


@pytest.mark.parametrize("B,T,flags", [(2000, 56, 0), (4096, 64, LANE)])
def test_a_repeated_pass_starts_from_the_same_seed(Smpc, mod, monkeypatch, B, T, flags):
    from tests.footprint_scenes import setup
    cfg, scn, noise, tick, u0 = ms.pass_case(B, T, flags)
    cr = critics_of(FIVE)
    ga = setup(create_with_env(Smpc, monkeypatch, cfg, {"SMPC_DEBUG_REPEAT_PASS": "1"}), scn, cr, noise, False)
    ga.set_moving_obstacles(*across(cfg, tick), **ms.PARAMS)
    gp = ms.context(mod, cfg, scn, noise, cr, discs=across(cfg, tick))
    ra, rp = ga.optimize(tick, u0), gp.optimize(tick, u0)
    assert ra[1].passes > rp[1].passes
    same_tick(ga, gp, ra, rp, f"repeat {B}x{T}", skip=("passes",))
    close(ga, gp)


def test_all_lethal_costs_are_m_plus_obstacles_only(mod):
    cfg, scn, noise, tick, u0 = ms.pass_case(2000, 56, all_lethal=True)
    cr = critics_of(FIVE)
    ga = ms.context(mod, cfg, scn, noise, cr, discs=across(cfg, tick))
    gb = ms.context(mod, cfg, scn, noise, cr)
    (ua, oa), (ub, ob) = ga.optimize(tick, u0), gb.optimize(tick, u0)
    assert oa.fail_flag == 1 and ob.fail_flag == 1 and oa.non_colliding == 0
    seeded_equals_twin(ga, gb, 1, "all lethal")
    close(ga, gb)


def test_fail_flag_in_scores_nothing(mod):
    cfg, scn, noise, tick, u0 = ms.pass_case(2000, 56)
    tick.fail_flag_in = True
    cr = critics_of(FIVE)
    ga = ms.context(mod, cfg, scn, noise, cr, discs=across(cfg, tick))
    gb = ms.context(mod, cfg, scn, noise, cr)
    same_tick(ga, gb, ga.optimize(tick, u0), gb.optimize(tick, u0), "fail_flag_in")
    close(ga, gb)


# ---- 6. two iterations -------------------------------------------------------------------------------------

@pytest.mark.parametrize("B,T,flags", [(2000, 56, 0), (4096, 64, LANE)])
def test_the_second_iteration_adds_its_own_m(mod, B, T, flags):
    cfg, scn, noise, tick, u0 = ms.pass_case(B, T, flags)
    # Critics that do not read the furthest reached path point: a tick evaluates that point once, on its
    # first iteration's rollouts, and keeps it, so the second iteration of a tick and a fresh tick started
    # from u_1 would score PathAlign and PathFollow against different path points, obstacles or none.
    names = ("obstacles", "prefer_forward")
    cr, discs = critics_of(names), across(cfg, tick)
    g1 = ms.context(mod, cfg, scn, noise, cr, discs=discs)
    u1, _ = g1.optimize(tick, u0)
    costs_1 = g1.get_costs().astype(np.float64)
    m_0, _ = g1.moving_obstacle_costs()
    # m(u_1) and the obstacle-free costs of a tick started from u_1
    gm = ms.context(mod, cfg, scn, noise, cr, discs=discs)
    gm.optimize(tick, u1)
    m_1, _ = gm.moving_obstacle_costs()
    gf = ms.context(mod, cfg, scn, noise, cr)
    gf.optimize(tick, u1)
    free = gf.get_costs().astype(np.float64)
    cfg2, *_ = ms.pass_case(B, T, flags, iteration_count=2)
    g2 = ms.context(mod, cfg2, scn, noise, cr, discs=discs)
    g2.optimize(tick, u0)
    costs_2 = g2.get_costs().astype(np.float64)
    m_last, _ = g2.moving_obstacle_costs()
    assert not np.array_equal(u1, u0) and not np.array_equal(m_0, m_1)
    assert np.array_equal(bits(m_last), bits(m_1)), "the getter returns the last iteration's m, scored on u_1"
    want = costs_1 + m_1.astype(np.float64) + free
    # (the same kind of bound: the pass rounds costs_1 + m_1 once and adds its n terms: n + 1 roundings of
    # partial sums no larger than |costs_1| + |m_1| + sum |t_k|, |free| standing in for the last)
    bound = (len(names) + 1) * EPS * (np.abs(costs_1) + np.abs(m_1) + np.abs(free)) + 1e-30
    err = np.abs(costs_2 - want)
    print(f"[moving] two iterations {B}x{T}: worst error / bound {float((err / bound).max()):.3f}")
    assert np.all(err <= bound)
    close(g1, gm, gf, g2)


# ---- 7. limits and obstacles together ---------------------------------------------------------------------------

@pytest.mark.parametrize("B,T,flags", [(2000, 56, 0), (4096, 64, LANE)])
def test_limits_and_obstacles_equal_the_twin_fed_the_limited_noise(mod, B, T, flags):
    cfg, scn, noise, tick, u0 = ms.pass_case(B, T, flags)
    cr, discs = critics_of(FIVE), across(cfg, tick)
    limited = am.limited_noise(noise, u0, tick.speed, cfg.model_dt, LIM, holonomic=True)
    ga = ms.context(mod, cfg, scn, noise, cr, discs=discs, limits=LIM)
    gb = ms.context(mod, cfg, scn, limited, cr, discs=discs)
    same_tick(ga, gb, ga.optimize(tick, u0), gb.optimize(tick, u0), f"limits {B}x{T}")
    (ma, ha), (mb, hb) = ga.moving_obstacle_costs(), gb.moving_obstacle_costs()
    assert np.array_equal(bits(ma), bits(mb)) and np.array_equal(ha, hb)
    gc = ms.context(mod, cfg, scn, noise, cr, discs=discs)
    gc.optimize(tick, u0)
    assert not np.array_equal(bits(gc.moving_obstacle_costs()[0]), bits(ma))
    close(ga, gb, gc)


# ---- 7a. the single context's breakdown ------------------------------------------------------------------------

@pytest.mark.parametrize("B,T,flags,kind", [(2000, 56, 0, 0), (4096, 64, LANE, 1)])
def test_a_solo_breakdown_starts_from_the_ticks_seed(mod, B, T, flags, kind):
    """smpc_critic_breakdown with a table set (a lane context: the breakdown reads the [B,T] noise, so
    its seed comes from the row-major form where the tick's came from the group-major one)."""
    cfg, scn, noise, tick, u0 = ms.pass_case(B, T, flags)
    cr, discs = critics_of(FIVE), across(cfg, tick)
    g = ms.context(mod, cfg, scn, noise, cr, discs=discs)
    gp = ms.context(mod, cfg, scn, noise, cr, discs=discs)
    st = g.critic_stats(tick, u0, per_rollout=True)
    with pytest.raises(mod.SmpcError) as e:
        g.moving_obstacle_costs()                       # the breakdown is no tick: nothing to hand out yet
    assert e.value.code == A.SMPC_ERR_STATE
    ra, rp = g.optimize(tick, u0), gp.optimize(tick, u0)
    assert ra[1].pass_kind == kind
    same_tick(g, gp, ra, rp, f"breakdown first {B}x{T}")          # the breakdown changed nothing
    # The rows are the wave-per-rollout pass's arithmetic.  A lane context's tick scores with the lane
    # pass's own (its sin/cos, its square roots): there the rows are held, bit for bit, to the breakdown
    # of a wave context on the same inputs, and that context's tick is what they add up to.
    gw = g
    if kind != 0:
        cfg_w, *_ = ms.pass_case(B, T, 0)
        gw = ms.context(mod, cfg_w, scn, noise, cr, discs=discs)
        sw = gw.critic_stats(tick, u0, per_rollout=True)
        assert np.array_equal(bits(st.per_rollout), bits(sw.per_rollout))
        assert (st.best_rollout, st.best_cost, st.effective_samples) == (sw.best_rollout, sw.best_cost, sw.effective_samples)
        _, ow = gw.optimize(tick, u0)
        assert ow.pass_kind == 0
    costs = gw.get_costs().astype(np.float64)
    m = gw.moving_obstacle_costs()[0].astype(np.float64)
    rows = st.per_rollout.astype(np.float64)
    n_rows = bin(st.scored_mask).count("1")
    bound = sum_bound(n_rows, m, np.abs(rows).sum(axis=0))
    err = np.abs(costs - (rows.sum(axis=0) + m))
    print(f"[moving] solo breakdown {B}x{T}: rows + m against the tick's costs, worst error / bound "
          f"{float((err / bound).max()):.3f}; best rollout {st.best_rollout}")
    assert np.all(err <= bound) and (m > 0).any()
    best = int(np.argmin(gw.get_costs()))
    assert abs(st.best_cost - float(costs.min())) <= float(bound.max())
    # (the two forms round m differently: the breakdown's best rollout is the tick's unless a rival lies within the bound)
    rivals = np.nonzero(costs - costs.min() <= 2.0 * bound.max())[0]
    assert st.best_rollout in rivals, (st.best_rollout, best)
    close(*{id(x): x for x in (g, gp, gw)}.values())


# ---- 8. group ---------------------------------------------------------------------------------------------------

def test_group_members_with_obstacles_ride_and_equal_their_solo_contexts(mod):
    B, T, N = 2000, 56, 4
    cr, n_cr = ms.pass_critics("deployed", False)
    members, solos = [], []
    for i in range(N):
        cfg, scn, _, tick, u0 = ms.pass_case(B, T)
        noise = make_noise(B, T, std=(cfg.vx_std, cfg.vy_std, cfg.wz_std), seed=900 + i)
        discs = across(cfg, tick, seed=20 + i) if i < 2 else None
        members.append(ms.context(mod, cfg, scn, noise, cr, discs=discs))
        solos.append(ms.context(mod, cfg, scn, noise, cr, discs=discs))
    grp = mod.SmpcGroup(members)
    us, ut = [u0] * N, [u0] * N
    for k in range(4):
        t = moved(tick, 0.015 * k)
        before = grp.stats()
        res = grp.optimize([t] * N, us)
        after = grp.stats()
        for i in range(N):
            rt = solos[i].optimize(t, ut[i])
            same_tick(members[i], solos[i], (res[i][0], res[i][1]), rt, f"round {k} member {i}", skip=("passes",))
            if i < 2:
                assert np.array_equal(bits(members[i].moving_obstacle_costs()[0]), bits(solos[i].moving_obstacle_costs()[0]))
            ut[i] = rt[0]
        print(f"[moving] group round {k}: batched +{after.batched_launches - before.batched_launches}, "
              f"single +{after.single_ticks - before.single_ticks}")
        if k >= 2:
            assert after.batched_launches > before.batched_launches, k
        if k == 3:
            stats = grp.critic_stats([t] * N, us, per_rollout=True)
        us = [r[0] for r in res]
    # the breakdown of the round just run (same inputs): its costs are the round's, its rows add up to cost - m
    for i in range(N):
        costs = members[i].get_costs().astype(np.float64)
        rows = stats[i].per_rollout.astype(np.float64).sum(axis=0)
        m = members[i].moving_obstacle_costs()[0].astype(np.float64) if i < 2 else np.zeros(B)
        n_rows = bin(stats[i].scored_mask).count("1")     # (the scored critics and the control row)
        bound = sum_bound(n_rows, m, np.abs(stats[i].per_rollout.astype(np.float64)).sum(axis=0))
        err = np.abs(costs - (rows + m))
        print(f"[moving] group breakdown member {i}: rows + m against the round's costs, worst error / bound "
              f"{float((err / bound).max()):.3f}")
        assert np.all(err <= bound), i
        # (the breakdown's pass keeps every critic's term apart: its total is the round's within the same bound)
        assert abs(stats[i].best_cost - float(costs.min())) <= float(bound.max()), i
        assert stats[i].best_rollout == int(np.argmin(members[i].get_costs())), i
    grp.close()
    close(*members, *solos)


# ---- 9. shards --------------------------------------------------------------------------------------------------

def test_two_emulated_shards_with_obstacles_reproduce_the_unsharded_tick(mod):
    import torch
    B, T, G = 4096, 64, 2
    cfg, scn, noise, tick, u0 = ms.pass_case(B, T)
    cr, discs = critics_of(FIVE), across(cfg, tick)
    whole = ms.context(mod, cfg, scn, noise, cr, discs=discs)
    u_w, out_w = whole.optimize(tick, u0)
    m_w, hit_w = whole.moving_obstacle_costs()
    cuts = np.linspace(0, B, G + 1).astype(int)
    shards = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        c2 = default_config(batch_size=int(b - a), time_steps=T, shard_offset=int(a), global_batch_size=B)
        shards.append(ms.context(mod, c2, scn, [n[a:b] for n in noise], cr, discs=discs))
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
    for s, a, b in zip(shards, cuts[:-1], cuts[1:]):
        m_s, hit_s = s.moving_obstacle_costs()
        assert np.array_equal(bits(m_s), bits(m_w[a:b])) and np.array_equal(hit_s, hit_w[a:b]), (a, b)
    close(whole, *shards)


# ---- 10. fleet --------------------------------------------------------------------------------------------------------

R0, R1 = 0.3, 0.3
FREQ = 20.0


def fleet_pair(B=2000, T=56):
    from mpcholonavigation_amd.host_optimizer import FleetOptimizer, Optimizer
    cfg, scn, _ = make_case(B, T)
    cells = np.zeros_like(scn.cells)
    hosts = []
    for i in range(2):
        h = Optimizer(cfg, critics_of(FIVE), FREQ, critics=classes(FIVE), cost_scaling_factor=scn.cost_scaling_factor,
                      inflation_radius=scn.inflation_radius)
        h.set_costmap(cells, scn.origin_x, scn.origin_y, scn.resolution, inscribed_radius=scn.inscribed_radius)
        h.set_noise(*make_noise(B, T, std=(cfg.vx_std, cfg.vy_std, cfg.wz_std), seed=300 + i))
        hosts.append(h)
    return hosts, FleetOptimizer(hosts), scn


def head_on_tick(pose, goal_x, res=0.05):
    """A straight plan from the robot's x to goal_x along its own line, at the costmap's resolution."""
    x, y, yaw = pose
    sign = 1.0 if goal_x > x else -1.0
    px = (x + sign * res * np.arange(max(int(abs(goal_x - x) / res), 2))).astype(np.float32)
    return Tick(x, y, yaw, (0.0, 0.0, 0.0), px, np.full(len(px), y, np.float32), np.full(len(px), yaw, np.float32),
                float(px[-1]), float(y))


def head_on_run(avoid, rounds=40):
    hosts, fleet, scn = fleet_pair()
    if avoid:
        fleet.set_mutual_avoidance([R0, R1], collision_cost=10000.0, repulsion_weight=20.0, margin=0.6)
    y = scn.tick.pose_y
    poses = [np.array([3.0, y, 0.0]), np.array([4.6, y + 0.02, np.pi])]
    goals = [8.0, 1.0]
    speeds = [(0.0, 0.0, 0.0), (0.0, 0.0, 0.0)]
    least = np.inf
    for k in range(rounds):
        ticks = [head_on_tick(poses[i], goals[i]) for i in range(2)]
        for i in range(2):
            ticks[i].speed = speeds[i]
        res = fleet.eval_control(ticks)
        for i in range(2):
            assert res[i].status == 0, res[i].error
            vx, vy, wz = res[i].twist
            c, s = np.cos(poses[i][2]), np.sin(poses[i][2])
            poses[i] = poses[i] + np.array([(vx * c - vy * s), (vx * s + vy * c), wz]) / FREQ
            speeds[i] = (float(vx), float(vy), float(wz))
        least = min(least, float(np.hypot(*(poses[0][:2] - poses[1][:2]))))
    fleet.close()
    close(*hosts)
    return least


def test_two_robots_head_on_keep_their_distance_with_mutual_avoidance(mod):
    with_avoidance, without = head_on_run(True), head_on_run(False)
    print(f"[moving] head-on, 40 rounds: least centre distance {with_avoidance:.3f} m with mutual avoidance, "
          f"{without:.3f} m without; r_0 + r_1 = {R0 + R1}")
    assert without < R0 + R1
    assert with_avoidance >= R0 + R1


def test_a_member_not_taken_becomes_a_standing_disc(mod):
    hosts, fleet, scn = fleet_pair(B=512)
    fleet.set_mutual_avoidance([R0, R1])
    y = scn.tick.pose_y
    t0, t1 = head_on_tick((3.0, y, 0.0), 8.0), head_on_tick((3.5, y, np.pi), 1.0)
    fleet.eval_control([t0, t1], take=[1, 0])
    with pytest.raises(RuntimeError):
        hosts[0].moving_obstacle_costs()      # member 1 was never seen: member 0 has no obstacle
    fleet.eval_control([t0, t1])              # both seen
    fleet.eval_control([t0, t1], take=[1, 0])
    m, hit = hosts[0].moving_obstacle_costs()  # member 1 stands half a metre ahead, on member 0's line
    print(f"[moving] standing member: {int((m > 0).sum())} of {len(m)} rollouts within reach, {int(hit.sum())} hit")
    assert (m > 0).mean() > 0.5
    fleet.set_mutual_avoidance(None)
    fleet.eval_control([t0, t1])
    with pytest.raises(RuntimeError):
        hosts[0].moving_obstacle_costs()
    fleet.close()
    close(*hosts)


# ---- 11. turning it off ---------------------------------------------------------------------------------------

def test_replacing_clearing_and_the_getters_state(mod):
    cfg, scn, noise, tick, u0 = ms.pass_case(2000, 56)
    cr = critics_of(FIVE)
    g, plain = ms.context(mod, cfg, scn, noise, cr), ms.context(mod, cfg, scn, noise, cr)
    with pytest.raises(mod.SmpcError) as e:
        g.moving_obstacle_costs()                       # off
    assert e.value.code == A.SMPC_ERR_STATE
    xy, radius = across(cfg, tick)
    bad = [dict(margin=0.0), dict(margin=-1.0), dict(collision_cost=-1.0), dict(repulsion_weight=-1.0),
           dict(margin=float("nan")), dict(collision_cost=float("inf"))]
    for kw in bad:
        with pytest.raises(mod.SmpcError) as e:
            g.set_moving_obstacles(xy, radius, **kw)
        assert e.value.code == A.SMPC_ERR_INVALID, kw
    for r in (0.0, -0.2, float("nan")):
        with pytest.raises(mod.SmpcError) as e:
            g.set_moving_obstacles(xy, np.array([r, 0.2, 0.2], np.float32))
        assert e.value.code == A.SMPC_ERR_INVALID, r
    with pytest.raises(mod.SmpcError) as e:
        g.set_moving_obstacles(np.zeros((65, cfg.time_steps, 2), np.float32), np.ones(65, np.float32))
    assert e.value.code == A.SMPC_ERR_UNSUPPORTED
    g.set_moving_obstacles(xy, radius, **ms.PARAMS)
    with pytest.raises(mod.SmpcError) as e:
        g.moving_obstacle_costs()                       # no tick yet
    assert e.value.code == A.SMPC_ERR_STATE
    g.optimize(tick, u0)
    plain.optimize(tick, u0)
    m1, _ = g.moving_obstacle_costs()
    g.reset()                                           # the table survives
    plain.reset()
    g.set_noise(*noise)
    plain.set_noise(*noise)
    g.optimize(tick, u0)
    plain.optimize(tick, u0)
    assert np.array_equal(bits(g.moving_obstacle_costs()[0]), bits(m1))
    g.set_moving_obstacles(*across(cfg, tick, seed=12), **ms.PARAMS)    # replaced: the next tick scores the new table
    g.optimize(tick, u0)
    plain.optimize(tick, u0)
    assert not np.array_equal(bits(g.moving_obstacle_costs()[0]), bits(m1))
    g.set_moving_obstacles(None)                        # off again: the parent's bits
    with pytest.raises(mod.SmpcError) as e:
        g.moving_obstacle_costs()
    assert e.value.code == A.SMPC_ERR_STATE
    same_tick(g, plain, g.optimize(tick, u0), plain.optimize(tick, u0), "switched off", skip=("passes",))
    close(g, plain)
