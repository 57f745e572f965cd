"""Size-independent properties of the HIP path at BASELINE.json's full sizes (where the
oracle is too slow to be the checker), plus shape edge cases and the multi-query
configuration (replicas only)."""
import os

import numpy as np
import pytest

from mpcholonavigation_amd import _abi as A
from mpcholonavigation_amd.synthetic import make_noise, make_scenario
from mpcholonavigation_amd.tick import Tick, default_config, default_critics
from tests.helpers import assert_parity, configure, rel_err

pytestmark = pytest.mark.gpu

FULL = [(65536, 64, 200),      # configs[1]
        (262144, 128, 2000),   # configs[2]
        (262144, 64, 200)]     # configs[3] per-GPU shard


def _ctx(B, T, map_size, noise=None, seed=None, **cfg_kw):
    from mpcholonavigation_amd.optimizer import Smpc
    cfg = default_config(batch_size=B, time_steps=T, **cfg_kw)
    scn = make_scenario(T, map_size=map_size)
    g = Smpc(cfg)
    configure(g, scn, noise=noise)
    if seed is not None:
        g.seed(seed)
    return g, scn


@pytest.mark.parametrize("B,T,M", FULL)
def test_full_size_determinism_and_permutation_invariance(B, T, M):
    """Same inputs -> bit-identical control sequence; permuting the rollouts (rows of the
    noise tensors) changes only the float summation order."""
    g, scn = _ctx(B, T, M, seed=11)
    u1, o1 = g.optimize(scn.tick, scn.u0)
    u2, o2 = g.optimize(scn.tick, scn.u0)
    assert np.array_equal(u1, u2) and o1.min_cost == o2.min_cost
    nvx, nvy, nwz = g.get_noise()
    perm = np.random.default_rng(0).permutation(B)
    g.set_noise(nvx[perm], nvy[perm], nwz[perm])
    u3, o3 = g.optimize(scn.tick, scn.u0)
    assert o3.min_cost == o1.min_cost and o3.non_colliding == o1.non_colliding
    assert o3.furthest_reached_path_point == o1.furthest_reached_path_point
    assert rel_err(u3, u1) < 5e-6
    c1 = np.sort(g.get_costs())
    g.set_noise(nvx, nvy, nwz)
    g.optimize(scn.tick, scn.u0)
    assert np.array_equal(np.sort(g.get_costs()), c1)      # the multiset of costs is the same


@pytest.mark.parametrize("B,T,M", FULL)
def test_full_size_zero_noise_is_a_fixed_point(B, T, M):
    """With zero noise every rollout is the same: equal weights, so the update returns the
    (clipped) input sequence and every cost is identical."""
    z = np.zeros((B, T), np.float32)
    g, scn = _ctx(B, T, M, noise=(z, z, z))
    u0 = scn.u0.copy()
    u0[1] = 0.02
    u0[2] = np.linspace(-0.1, 0.1, T)
    u, out = g.optimize(scn.tick, u0)
    assert np.max(np.abs(u - u0)) < 1e-6
    c = g.get_costs()
    assert np.all(c == c[0])
    assert abs(out.sum_w - B) < 1e-3 * B


@pytest.mark.parametrize("B,T,M", FULL)
def test_full_size_shards_sum_to_the_whole(B, T, M):
    """Two half-batch contexts (device RNG slices of the same stream) combine to the
    whole-batch tick: the data path of the 2-GPU run on one GPU."""
    import torch
    g, scn = _ctx(B, T, M, seed=5)
    u_w, out_w = g.optimize(scn.tick, scn.u0)
    halves = []
    for k in range(2):
        h, _ = _ctx(B // 2, T, M, seed=5, shard_offset=k * (B // 2), global_batch_size=B)
        halves.append(h)
    dev = torch.device("cuda", 0)
    L = halves[0].tuple_len
    t_all = torch.zeros(2 * L, dtype=torch.float32, device=dev)
    S = int(out_w.furthest_reached_path_point)
    for k, h in enumerate(halves):
        h.set_stream(torch.cuda.current_stream().cuda_stream)
        h.shard_begin(scn.tick, scn.u0)
        h.shard_score(0, S, t_all[k * L:].data_ptr())
    u_s, out_s = halves[0].shard_combine(t_all.data_ptr(), 2)
    assert out_s.furthest_reached_path_point == S
    assert out_s.non_colliding == out_w.non_colliding
    assert abs(out_s.min_cost - out_w.min_cost) <= 1e-6 * max(1.0, abs(out_w.min_cost))
    assert rel_err(u_s, u_w) < 5e-6


@pytest.mark.parametrize("B,T", [(4096, 56), (70000, 64)])
def test_reset_and_seed_put_a_context_back_where_it_started(B, T):
    """bench.py warms the clocks with the workload's own ticks and then calls smpc_reset and smpc_seed:
    after that a context has to behave bit for bit like a fresh one — the same noise, no
    furthest-point prediction (first tick: the furthest-only pass in front), the same ticks after."""
    fresh, scn = _ctx(B, T, 200, seed=11)
    used, _ = _ctx(B, T, 200, seed=11)
    u = scn.u0
    for _ in range(12):
        un, _ = used.optimize(scn.tick, u)
        u = np.concatenate([un[:, 1:], un[:, -1:]], axis=1)
    used.reset()
    used.seed(11)
    ua = ub = scn.u0
    for k in range(4):
        ua, oa = fresh.optimize(scn.tick, ua)
        ub, ob = used.optimize(scn.tick, ub)
        assert np.array_equal(ua, ub), k
        assert np.array_equal(fresh.get_costs(), used.get_costs()), k
        for f in ("passes", "pass_kind", "furthest_reached_path_point", "non_colliding", "min_cost", "sum_w"):
            assert getattr(oa, f) == getattr(ob, f), (k, f)
        ua = np.concatenate([ua[:, 1:], ua[:, -1:]], axis=1)
        ub = np.concatenate([ub[:, 1:], ub[:, -1:]], axis=1)


def test_multi_query_replicas_are_independent():
    """configs[4] in miniature: several planning instances (own costmap seed, pose, plan, noise)
    packed on one GPU; each must equal its own oracle, whatever the others do."""
    from mpcholonavigation_amd.optimizer import Smpc
    from oracle.loader import Oracle
    B, T, N = 2048, 64, 6
    ctxs = []
    for k in range(N):
        cfg = default_config(batch_size=B, time_steps=T)
        scn = make_scenario(T, seed=100 + k, warm_vx=0.2 + 0.03 * k)
        noise = make_noise(B, T, seed=500 + k)
        g, o = Smpc(cfg), Oracle(cfg)
        for x in (g, o):
            configure(x, scn, noise=noise)
        ctxs.append((g, o, scn))
    res = [g.optimize(scn.tick, scn.u0) for g, _, scn in ctxs]          # all N on the GPU
    for k, (g, o, scn) in enumerate(ctxs):
        uo, oo = o.optimize(scn.tick, scn.u0)
        assert_parity(res[k][0], res[k][1], uo, oo, g.get_costs(), o.get_costs(),
                      label=f"instance {k}")
    assert len({tuple(np.round(r[0][:, 1], 5)) for r in res}) == N      # really different problems


def test_fallback_counter_is_per_object():
    """the reference's retry counter is function-static (shared by every Optimizer
    in the process); here one instance failing does not touch another's."""
    from mpcholonavigation_amd.host_optimizer import Optimizer
    cfg = default_config(batch_size=256, time_steps=30)
    bad_scn, good_scn = make_scenario(30, all_lethal=True), make_scenario(30)
    bad = Optimizer(cfg, default_critics(), 20.0, retry_attempt_limit=3)
    good = Optimizer(cfg, default_critics(), 20.0, retry_attempt_limit=3)
    bad.set_costmap(bad_scn.cells, 0.0, 0.0, 0.05)
    good.set_costmap(good_scn.cells, 0.0, 0.0, 0.05)
    for _ in range(2):
        with pytest.raises(RuntimeError):
            bad.eval_control(bad_scn.tick)
        tw, out = good.eval_control(good_scn.tick)
        assert out.fail_flag == 0 and np.isfinite(tw).all()


@pytest.mark.parametrize("P", [1, 2, 3, 64, 65, 300, 1024])
def test_path_length_edges(P, both_passes):
    """Plans from a single point to SMPC_MAX_PATH points (argmin over > 64 points, LDS staging).
    Which pass it judged: with SMPC_PASS=lane the lane pass up to the longest plan its LDS layout
    admits (tests/plan_scenes.py: read through smpc_debug_lds_layout), the wave pass beyond it — and
    the wave pass for a context that does not ask (512 rollouts)."""
    from mpcholonavigation_amd.optimizer import Smpc
    from oracle.loader import Oracle
    from tests.plan_scenes import lane_limit
    B, T = 512, 56
    cfg = default_config(batch_size=B, time_steps=T)
    scn = make_scenario(T)
    noise = make_noise(B, T)
    t = scn.tick
    spacing = 2.9 / max(P - 1, 1)
    px = (t.pose_x + spacing * np.arange(P)).astype(np.float32)
    tick = Tick(t.pose_x, t.pose_y, t.pose_yaw, t.speed, px, np.full(P, t.pose_y, np.float32),
                np.zeros(P, np.float32), float(px[-1]) + (3.0 if P == 1 else 0.0), t.pose_y)
    g, o = Smpc(cfg), Oracle(cfg)
    cr = default_critics()
    cr.path_align.offset_from_furthest = 1 if P < 40 else 20
    for x in (g, o):
        configure(x, scn, critics=cr, noise=noise)
    ug, og = g.optimize(tick, scn.u0)
    uo, oo = o.optimize(tick, scn.u0)
    kind = 1 if both_passes == "lane" and P <= lane_limit(T) else 0
    print(f"[path length] P={P} ({both_passes}): pass_kind {og.pass_kind}, lane pass up to P = {lane_limit(T)}")
    assert og.pass_kind == kind, (P, both_passes, og.pass_kind)
    assert_parity(ug, og, uo, oo, g.get_costs(), o.get_costs(), label=f"P={P}", max_flips=1)


def test_path_too_long_is_refused():
    from mpcholonavigation_amd.optimizer import Smpc, SmpcError
    cfg = default_config(batch_size=64, time_steps=30)
    scn = make_scenario(30)
    g = Smpc(cfg)
    configure(g, scn, noise=make_noise(64, 30))
    P = 1025
    t = scn.tick
    tick = Tick(t.pose_x, t.pose_y, 0.0, t.speed, np.linspace(2, 5, P).astype(np.float32),
                np.full(P, 5, np.float32), np.zeros(P, np.float32), 5.0, 5.0)
    with pytest.raises(SmpcError) as e:
        g.optimize(tick, scn.u0)
    assert e.value.code == A.SMPC_ERR_UNSUPPORTED


@pytest.mark.parametrize("T,step", [(64, 1), (64, 2), (64, 7), (128, 4), (256, 4), (200, 4), (30, 29)])
def test_path_align_sampling_geometries(T, step, both_passes):
    """trajectory_point_step / horizon combinations: 1..63 samples per rollout, i.e. every
    segment width (16/32/64 lanes) and group size of the flush."""
    from mpcholonavigation_amd.optimizer import Smpc
    from oracle.loader import Oracle
    B = 384
    cfg = default_config(batch_size=B, time_steps=T)
    scn = make_scenario(T)
    noise = make_noise(B, T)
    cr = default_critics()
    cr.path_align.trajectory_point_step = step
    cr.path_align.offset_from_furthest = 4
    g, o = Smpc(cfg), Oracle(cfg)
    for x in (g, o):
        configure(x, scn, critics=cr, noise=noise)
    ug, og = g.optimize(scn.tick, scn.u0)
    uo, oo = o.optimize(scn.tick, scn.u0)
    assert_parity(ug, og, uo, oo, g.get_costs(), o.get_costs(), label=f"T={T} step={step}",
                  max_flips=1)


def test_too_many_path_align_samples_is_refused():
    from mpcholonavigation_amd.optimizer import Smpc, SmpcError
    cfg = default_config(batch_size=64, time_steps=128)
    scn = make_scenario(128)
    g = Smpc(cfg)
    cr = default_critics()
    cr.path_align.trajectory_point_step = 1          # 127 samples > 63
    configure(g, scn, critics=cr, noise=make_noise(64, 128))
    with pytest.raises(SmpcError) as e:
        g.optimize(scn.tick, scn.u0)
    assert e.value.code == A.SMPC_ERR_UNSUPPORTED


def test_multi_query_contexts_are_independent():
    """BASELINE configs[4] (multi-query: replicas only): contexts ticking concurrently from their
    own host threads and streams give exactly what each gives alone."""
    import threading
    from mpcholonavigation_amd.optimizer import Smpc
    from tests.helpers import configure, make_case
    cases = [make_case(4096, 64, seed=40 + i, noise_seed=100 + i) for i in range(4)]
    alone = []
    for cfg, scn, noise in cases:
        g = Smpc(cfg)
        configure(g, scn, noise=noise)
        u = scn.u0
        for _ in range(3):
            u, out = g.optimize(scn.tick, u)
        alone.append((u.copy(), out.furthest_reached_path_point, out.non_colliding))
        g.close()
    ctxs = []
    for cfg, scn, noise in cases:
        g = Smpc(cfg)
        configure(g, scn, noise=noise)
        ctxs.append(g)
    res = [None] * len(cases)
    go = threading.Barrier(len(cases))

    def run(i):
        g, (cfg, scn, noise) = ctxs[i], cases[i]
        u = scn.u0
        go.wait()
        for _ in range(3):
            u, out = g.optimize(scn.tick, u)
        res[i] = (u.copy(), out.furthest_reached_path_point, out.non_colliding)

    ths = [threading.Thread(target=run, args=(i,)) for i in range(len(cases))]
    for t in ths:
        t.start()
    for t in ths:
        t.join()
    for (ua, fa, na), (uc, fc, nc) in zip(alone, res):
        assert fa == fc and na == nc
        assert np.array_equal(ua, uc)
    for g in ctxs:
        g.close()


def test_multi_query_at_the_stated_size_against_the_oracle():
    """BASELINE configs[4] at its stated per-GPU size: 8 planning instances x 16 384 rollouts x 64
    steps (64 instances packed over 8 GPUs), each with its own costmap, pose, plan, noise and
    speed, ticked through smpc_group_optimize — one upload, one scoring launch, one reduction for
    the eight — and every member held to the oracle on its own inputs (assert_parity), three
    ticks in a closed loop (the first has no furthest-point prediction and the second no drift
    estimate yet: members are re-scored on their own; the third rides the batched launch)."""
    from mpcholonavigation_amd.optimizer import Smpc, SmpcGroup
    from oracle.loader import Oracle
    n, B, T = 8, 16384, 64
    cases = []
    for i in range(n):
        cfg = default_config(batch_size=B, time_steps=T, flags=A.SMPC_FLAG_LANE_PER_ROLLOUT)   # (as bench.py's configs[4])
        scn = make_scenario(T, seed=300 + i, path_points=44 + 2 * i, speed=(0.2 + 0.02 * i, 0.0, 0.0),
                            warm_vx=0.25 + 0.01 * i)
        noise = make_noise(B, T, seed=7000 + i)
        cases.append((cfg, scn, noise))
    members, oracles = [], []
    for cfg, scn, noise in cases:
        g, o = Smpc(cfg), Oracle(cfg)
        for obj in (g, o):
            configure(obj, scn, noise=noise)
        members.append(g)
        oracles.append(o)
    grp = SmpcGroup(members)
    us = [scn.u0 for _, scn, _ in cases]
    passes = []
    for k in range(3):
        ticks = []
        for cfg, scn, noise in cases:
            t = scn.tick
            ticks.append(Tick(t.pose_x + 0.015 * k, t.pose_y, t.pose_yaw, t.speed, t.path_x, t.path_y, t.path_yaw,
                              t.goal_x, t.goal_y))
        res = grp.optimize(ticks, us)
        for i in range(n):
            ug, og = res[i]
            uo, oo = oracles[i].optimize(ticks[i], us[i])
            assert og.non_colliding == oo.non_colliding, (k, i)
            assert_parity(ug, og, uo, oo, members[i].get_costs(), oracles[i].get_costs(), max_flips=1,
                          label=f"configs[4] member {i} tick {k}", report=(i == 0))
            if not os.environ.get("SMPC_PASS"):
                assert og.pass_kind == 1, (k, i)
            us[i] = np.concatenate([uo[:, 1:], uo[:, -1:]], axis=1)   # both sides continue from the oracle's sequence
        passes.append([o.passes for _, o in res])
    print("[configs[4] at size] passes per member, per tick:", passes)
    grp.close()
    for g in members:
        g.close()


def test_grouped_contexts_tick_in_one_launch():
    """smpc_group_optimize (multi-robot fleets): members with different maps, paths (lengths
    40..60), noise and control sequences give bit-for-bit what smpc_optimize gives each of them,
    over a closed loop of ticks, and the steady state really is the batched launch.
    (A group's members always launch full-size blocks — together they fill the CUs — while a
    context of this size on its own launches half-size ones, which sums its partials in another
    order: the contexts ticked alone are created with that choice switched off.)"""
    from mpcholonavigation_amd.optimizer import Smpc, SmpcGroup
    from tests.helpers import configure
    n, B, T = 5, 2048, 56
    cases = []
    for i in range(n):
        cfg = default_config(batch_size=B, time_steps=T, flags=A.SMPC_FLAG_LANE_PER_ROLLOUT)
        scn = make_scenario(T, seed=60 + i, path_points=40 + 5 * i)
        noise = make_noise(B, T, seed=900 + i)
        cases.append((cfg, scn, noise))

    def fresh():
        out = []
        for cfg, scn, noise in cases:
            g = Smpc(cfg)
            configure(g, scn, noise=noise)
            out.append(g)
        return out

    os.environ["SMPC_NO_HALF_BLOCKS"] = "1"      # (read when a context is created)
    try:
        alone = fresh()
    finally:
        del os.environ["SMPC_NO_HALF_BLOCKS"]
    grouped = fresh()
    grp = SmpcGroup(grouped)
    us_a = [scn.u0 for _, scn, _ in cases]
    us_g = [scn.u0 for _, scn, _ in cases]
    kinds = []
    for k in range(5):
        ticks = []
        for i, (cfg, scn, noise) in enumerate(cases):
            t = scn.tick
            ticks.append(Tick(t.pose_x + 0.02 * k, t.pose_y, t.pose_yaw, (0.3, 0.0, 0.0), t.path_x, t.path_y,
                              t.path_yaw, t.goal_x, t.goal_y))
        res_g = grp.optimize(ticks, us_g)
        for i in range(n):
            ua, oa = alone[i].optimize(ticks[i], us_a[i])
            ug, og = res_g[i]
            assert np.array_equal(ua, ug), (k, i)
            assert oa.furthest_reached_path_point == og.furthest_reached_path_point
            assert oa.non_colliding == og.non_colliding
            if not os.environ.get("SMPC_PASS"):      # (the developer override picks the pass)
                assert og.pass_kind == 1
            us_a[i] = np.concatenate([ua[:, 1:], ua[:, -1:]], axis=1)
            us_g[i] = np.concatenate([ug[:, 1:], ug[:, -1:]], axis=1)
        kinds.append([o.passes for _, o in res_g])
    print("[group] passes per member, per tick:", kinds)
    # after the first tick (no furthest-point guess yet) the members ride the batched launch: a
    # member scores twice only on the ticks its furthest-point prediction misses
    if not os.environ.get("SMPC_PASS"):
        later = [p for row in kinds[1:] for p in row]
        assert sum(p == 1 for p in later) >= len(later) - n - 2, kinds   # (tick 1 has no drift estimate yet)
        assert all(p == 1 for p in kinds[-1]), kinds
    grp.close()
    for g in alone + grouped:
        g.close()


def test_grouped_contexts_keep_their_own_temperature():
    """Members of a group share the horizon and nothing else: each member's partials are reduced with
    ITS temperature (the batched reduction once used the first member's for all of them: sum_w 3.72
    for 2.00, the control sequence off by 0.37 — found by tools/fuzz_group.py)."""
    from mpcholonavigation_amd.optimizer import Smpc, SmpcGroup
    from tests.helpers import configure
    B, T = 2048, 56
    temps = (1.0, 0.1, 0.3, 0.05)
    cases = []
    for i, temp in enumerate(temps):
        cfg = default_config(batch_size=B, time_steps=T, flags=A.SMPC_FLAG_LANE_PER_ROLLOUT, temperature=temp,
                             gamma=0.015 * (i + 1))
        scn = make_scenario(T, seed=70 + i)
        cases.append((cfg, scn, make_noise(B, T, seed=950 + i)))

    def fresh():
        out = []
        for cfg, scn, noise in cases:
            g = Smpc(cfg)
            configure(g, scn, noise=noise)
            out.append(g)
        return out

    os.environ["SMPC_NO_HALF_BLOCKS"] = "1"      # (as above: the same block size alone and grouped)
    try:
        alone = fresh()
    finally:
        del os.environ["SMPC_NO_HALF_BLOCKS"]
    grouped = fresh()
    grp = SmpcGroup(grouped)
    us = [scn.u0 for _, scn, _ in cases]
    batched = 0
    for k in range(4):
        ticks = []
        for cfg, scn, noise in cases:
            t = scn.tick
            ticks.append(Tick(t.pose_x + 0.02 * k, t.pose_y, t.pose_yaw, (0.3, 0.0, 0.0), t.path_x, t.path_y, t.path_yaw,
                              t.goal_x, t.goal_y))
        res = grp.optimize(ticks, us)
        for i in range(len(cases)):
            ua, oa = alone[i].optimize(ticks[i], us[i])
            ug, og = res[i]
            assert oa.sum_w == og.sum_w and oa.min_cost == og.min_cost, (k, i, temps[i], oa.sum_w, og.sum_w)
            assert np.array_equal(ua, ug), (k, i, temps[i])
            batched += og.passes == 1
            us[i] = np.concatenate([ua[:, 1:], ua[:, -1:]], axis=1)
    assert batched >= 8          # the batched launch really ran (first tick and prediction misses aside)
    grp.close()
    for g in alone + grouped:
        g.close()


def test_grouped_contexts_with_the_deployed_critic_list():
    """A fleet whose members score the reference's deployed critic list (Constraint / Cost /
    Twirling next to the path critics): the batched launch of smpc_group_optimize has the lane
    pass's deployed-list instances too, and the group gives exactly what each member gives alone
    — bit for bit, over a closed loop — in one launch from the second tick on."""
    from mpcholonavigation_amd.optimizer import Smpc, SmpcGroup
    from tests.harness import DEPLOYED, critics_of
    from tests.helpers import configure
    cr = critics_of(DEPLOYED, power=None)
    n, B, T = 3, 4096, 64
    cases = []
    for i in range(n):
        cfg = default_config(batch_size=B, time_steps=T, flags=A.SMPC_FLAG_LANE_PER_ROLLOUT)
        cases.append((cfg, make_scenario(T, seed=70 + i), make_noise(B, T, seed=950 + i)))

    def fresh(env):
        out = []
        for k, v in env.items():
            os.environ[k] = v
        try:
            for cfg, scn, noise in cases:
                g = Smpc(cfg)
                configure(g, scn, critics=cr, noise=noise)
                out.append(g)
        finally:
            for k in env:
                del os.environ[k]
        return out

    alone, grouped = fresh({"SMPC_NO_HALF_BLOCKS": "1"}), fresh({})
    grp = SmpcGroup(grouped)
    us = [scn.u0 for _, scn, _ in cases]
    kinds = []
    for k in range(5):
        ticks = [scn.tick for _, scn, _ in cases]
        res = grp.optimize(ticks, us)
        for i in range(n):
            ua, oa = alone[i].optimize(ticks[i], us[i])
            ug, og = res[i]
            assert np.array_equal(ua, ug), (k, i)
            assert oa.non_colliding == og.non_colliding and og.pass_kind == 1
        kinds.append([o.passes for _, o in res])
        us = [np.concatenate([u[:, 1:], u[:, -1:]], axis=1) for u, _ in res]
    print("[group, deployed list] passes per member, per tick:", kinds)
    later = [p for row in kinds[2:] for p in row]      # (tick 1 has no drift estimate yet)
    assert sum(p == 1 for p in later) >= len(later) - 3, kinds   # a member re-scores only on a missed prediction
    grp.close()
    for g in alone + grouped:
        g.close()


@pytest.mark.parametrize("B,T,M", [(4096, 56, 200), (131072, 64, 200), (8192, 64, 2000)])
def test_costmap_handoff_uploads_only_what_changed(B, T, M):
    """the controller hands the costmap over every tick.  An unchanged
    map uploads nothing, a changed band of rows uploads that band, an explicit window uploads
    the window — and the tick that follows is bit-identical to one on a fresh context that
    was given the final map whole (the device copy and the pinned host mirror both match)."""
    from mpcholonavigation_amd.optimizer import Smpc
    g, scn = _ctx(B, T, M, seed=5)
    full = M * M
    assert g.costmap_upload_bytes() == (full, full)
    g.optimize(scn.tick, scn.u0)
    configure(g, scn)                                   # the same map again: nothing to do
    assert g.costmap_upload_bytes() == (0, full)

    # the inflation around the robot changes: a band of 9 rows differs
    cells = scn.cells.copy()
    rr = int((scn.tick.pose_y - scn.origin_y) / scn.resolution)
    rc = int((scn.tick.pose_x - scn.origin_x) / scn.resolution)
    cells[rr - 4:rr + 5, rc - 30:rc + 30] = np.maximum(cells[rr - 4:rr + 5, rc - 30:rc + 30], 100)
    g.set_costmap(cells, scn.origin_x, scn.origin_y, scn.resolution, inscribed_radius=scn.inscribed_radius,
                  cost_scaling_factor=scn.cost_scaling_factor, inflation_radius=scn.inflation_radius)
    assert g.costmap_upload_bytes()[0] == 9 * M         # rows rr-4 .. rr+4
    g.optimize(scn.tick, scn.u0)
    c1 = g.get_costs()

    # then a window (where every rollout starts) is handed over explicitly
    cells[rr - 2:rr + 2, rc - 3:rc + 3] = 150
    g.update_costmap_region(cells, rc - 3, rr - 2, 6, 4)
    assert g.costmap_upload_bytes()[0] == 24
    u2, o2 = g.optimize(scn.tick, scn.u0)
    c2 = g.get_costs()
    assert not np.array_equal(c1, c2)                   # the window mattered

    f = Smpc(default_config(batch_size=B, time_steps=T))
    f.set_critics(default_critics())
    f.set_costmap(cells, scn.origin_x, scn.origin_y, scn.resolution, inscribed_radius=scn.inscribed_radius,
                  cost_scaling_factor=scn.cost_scaling_factor, inflation_radius=scn.inflation_radius)
    f.seed(5)
    uf, of = f.optimize(scn.tick, scn.u0)
    assert np.array_equal(u2, uf) and np.array_equal(c2, f.get_costs())
    assert o2.non_colliding == of.non_colliding

    # a rolling window moves: new origin, same size -> whatever rows differ; a new size -> all
    g.set_costmap(np.roll(cells, 3, axis=0), scn.origin_x, scn.origin_y + 3 * scn.resolution, scn.resolution)
    assert 0 < g.costmap_upload_bytes()[0] <= full
    small = cells[: M // 2, : M // 2]
    g.set_costmap(small, scn.origin_x, scn.origin_y, scn.resolution)
    assert g.costmap_upload_bytes()[0] == small.size
    with pytest.raises(RuntimeError, match="region outside"):
        g.update_costmap_region(cells, M // 2 - 2, 0, 4, 4)


@pytest.mark.parametrize("B,T,flags,speculate", [
    (1000, 30, 0, True),                              # configs[0]: wave-per-rollout pass, ragged T
    (2000, 56, 0, True),                              # the deployed shape
    (2000, 56, 0, False),                             # two-pass mode: furthest-only pass, then scoring
    (4096, 64, A.SMPC_FLAG_LANE_PER_ROLLOUT, True),   # lane pass, 8 blocks
    (65536, 64, 0, True),                             # configs[1]: lane pass, 128 blocks
    (262144, 64, 0, True),                            # the 8-GPU share: 256 blocks
])
def test_fused_reduction_matches_the_launch(B, T, flags, speculate, monkeypatch):
    """The reduction inside the scoring launch (smpc_tail.h: the blocks that finish last reduce the
    grid's partials; opt-in, SMPC_FUSED_REDUCE=1) against the separate smpc_reduce_partials launch:
    the same additions in the same order, so every tick agrees bit for bit — control sequence,
    minimum cost, sum of weights, furthest point, collision count — over a closed loop."""
    from mpcholonavigation_amd.optimizer import Smpc
    if not speculate:
        flags |= A.SMPC_FLAG_NO_SPECULATION
    cfg = default_config(batch_size=B, time_steps=T, flags=flags)
    scn = make_scenario(T)
    noise = make_noise(B, T, seed=5)
    separate = Smpc(cfg)
    monkeypatch.setenv("SMPC_FUSED_REDUCE", "1")      # (read when the context is created)
    fused = Smpc(cfg)
    monkeypatch.delenv("SMPC_FUSED_REDUCE")
    for g in (separate, fused):
        configure(g, scn, noise=noise)
    us = uf = scn.u0
    for k in range(4):
        t = scn.tick
        tk = Tick(t.pose_x + 0.015 * k, t.pose_y, t.pose_yaw, (0.3, 0.0, 0.0), t.path_x, t.path_y, t.path_yaw,
                  t.goal_x, t.goal_y)
        us, os_ = separate.optimize(tk, us)
        uf, of = fused.optimize(tk, uf)
        assert np.array_equal(us, uf), k
        for f in ("min_cost", "sum_w", "furthest_reached_path_point", "non_colliding", "passes", "pass_kind"):
            assert getattr(os_, f) == getattr(of, f), (k, f)
        us = np.concatenate([us[:, 1:], us[:, -1:]], axis=1)
        uf = np.concatenate([uf[:, 1:], uf[:, -1:]], axis=1)
    separate.close()
    fused.close()
