"""smpc_critic_breakdown on the GPU: every row against the oracle's term for that critic, the rows
against the tick's own costs, the statistics against float64 NumPy on the device's rows, no side
effect on the ticks around a call, the mask, the host face.

Shapes (one per instance of smpc_pass_stats and the partial PathAlign flush): 400 x 15 (the reference
smoke fixture's shape: R = 1, ragged), 192 x 64 (R = 1, whole), 2 000 x 56 (the deployed nine),
200 x 128 (R = 2, whole), 130 x 200 (R = 4, ragged; 130 is no multiple of the flush group).
What lies beyond one slice of the reduction (B > 16 384), a footprint, a non-holonomic model and a lane
context's device noise is in test_gpu_critic_stats_reach.py."""
import numpy as np
import pytest

from mpcholonavigation_amd import _abi as A
from mpcholonavigation_amd.tick import Tick, default_config, default_critics
from tests import softmax_model as sm
from tests.harness import DEPLOYED, FIVE, OUT_FIELDS, Oracle, Smpc, last_kernel, shifted  # noqa: F401
from tests.helpers import configure, cost_flips, make_case
from tests.stats_scenes import CONTROL, EPS, ORDER, breakdown, check_statistics, critics, mask_of, row_parity, scene

pytestmark = pytest.mark.gpu

SHAPES = [(400, 15, ORDER), (192, 64, ORDER), (2000, 56, DEPLOYED), (200, 128, ORDER), (130, 200, ORDER)]


@pytest.mark.parametrize("kind", ["wall", "near"])
@pytest.mark.parametrize("power", [1, 2])
@pytest.mark.parametrize("B,T,names", SHAPES, ids=[f"{b}x{t}" for b, t, _ in SHAPES])
def test_rows_match_the_oracle_critic_by_critic(Smpc, Oracle, B, T, names, power, kind):
    """Row k of per_rollout against the oracle's term for critic k: the oracle scoring a list of
    that critic alone with gamma = 0, so that its costs ARE the term, (float)pow(v, power).  Row 12
    against the float64 gamma formula of tests/softmax_model.py; its bound is that file's
    worst-case count for sums of this form (gamma_uc_bound's reasoning on the reference's own
    form u (cv - u)): T + 2 roundings per control on gamma_magnitude, and three more for the
    product with gamma / std^2 and the two additions of the three controls' terms."""
    cfg, scn, noise = scene(B, T, kind)
    cr = critics(names, power)
    # first: the tick's total costs against the oracle's count zero flips on this scene and seed
    g, o = Smpc(cfg), Oracle(cfg)
    for obj in (g, o):
        configure(obj, scn, critics=cr, noise=noise)
    _, og = g.optimize(scn.tick, scn.u0)
    _, oo = o.optimize(scn.tick, scn.u0)
    assert og.fail_flag == oo.fail_flag == 0
    assert cost_flips(g.get_costs(), o.get_costs()) == 0, "pick another seed: the totals already flip"
    st = g.critic_stats(scn.tick, scn.u0, per_rollout=True)
    assert st.batch == B and not st.fail_flag and st.per_rollout.shape == (13, B)
    cfg0 = default_config(batch_size=B, time_steps=T, gamma=0.0)
    scored = 0
    for k, n in enumerate(ORDER):
        if n not in names:
            assert not st.scored_mask >> k & 1 and not st.per_rollout[k].any(), n
            continue
        o1 = Oracle(cfg0)
        configure(o1, scn, critics=critics((n,), power), noise=noise)
        o1.optimize(scn.tick, scn.u0)
        ref = o1.get_costs()
        row_parity(st.per_rollout[k], ref, T, f"{B}x{T} {kind} power {power} {n}")
        if not st.scored_mask >> k & 1:
            assert not st.per_rollout[k].any() and not ref.any(), n
        else:
            scored += 1
    # every host gate opens in one of the two scenes
    far = {"path_align", "path_align_legacy", "path_follow", "prefer_forward", "path_angle", "twirling"}
    near = {"goal_angle", "goal"}
    for n in (far if kind == "wall" else near) & set(names):
        assert st.scored(st.names[ORDER.index(n)]), n
    assert scored >= 5
    model = sm.gamma_terms(scn.u0, noise, cfg)
    bound = (T + 5) * EPS * sm.gamma_magnitude(scn.u0, noise, cfg) + 1e-30
    d = np.abs(st.per_rollout[CONTROL].astype(np.float64) - model)
    print(f"[critic stats] {B}x{T} control row: max |d| / bound {float((d / bound).max()):.3f}")
    assert np.all(d <= bound)


@pytest.mark.parametrize("B,T,names", SHAPES, ids=[f"{b}x{t}" for b, t, _ in SHAPES])
def test_rows_add_up_to_the_ticks_costs(Smpc, B, T, names):
    """smpc_get_costs after smpc_optimize on the same inputs against the float64 sum of the 13
    rows, every rollout: one float rounding per stored term and one per chained add."""
    cfg, scn, noise = scene(B, T, "wall")
    cr = critics(names, 2)      # (a cost_power other than 1: the tick itself runs the general pass)
    g, st = breakdown(Smpc, cfg, scn, noise, cr)
    _, out = g.optimize(scn.tick, scn.u0)
    assert last_kernel(g).startswith("smpc_pass<") and out.pass_kind == 0
    costs = g.get_costs().astype(np.float64)
    rows = st.per_rollout.astype(np.float64)
    n = bin(st.scored_mask).count("1")
    err = np.abs(rows.sum(axis=0) - costs)
    bound = (n + 1) * EPS * np.abs(rows).sum(axis=0)
    print(f"[critic stats] rows add up {B}x{T}: {n} rows, max err / bound {float((err / np.maximum(bound, 1e-300)).max()):.3f}")
    assert np.all(err <= bound)
    assert st.best_cost == np.float32(costs.min()) and st.best_rollout == int(np.argmin(costs))


@pytest.mark.parametrize("B,T,names", SHAPES, ids=[f"{b}x{t}" for b, t, _ in SHAPES])
def test_statistics_against_float64_numpy(Smpc, B, T, names):
    cfg, scn, noise = scene(B, T, "wall")
    g, st = breakdown(Smpc, cfg, scn, noise, critics(names, 1))
    g.optimize(scn.tick, scn.u0)
    ess = check_statistics(st, g.get_costs(), cfg)
    print(f"[critic stats] {B}x{T}: effective samples {st.effective_samples:.2f} (float64 {ess:.2f}), best {st.best_rollout}")


def test_statistics_with_tied_minima(Smpc):
    """Every rollout has a twin with the same noise, hence the same cost: the best rollout is the
    lower index of the least pair."""
    B, T = 400, 15
    cfg, scn, noise = scene(B, T, "wall")
    noise = tuple(np.concatenate([n[:B // 2], n[:B // 2]]) for n in noise)
    g, st = breakdown(Smpc, cfg, scn, noise, critics(ORDER, 1))
    g.optimize(scn.tick, scn.u0)
    costs = g.get_costs()
    assert np.array_equal(costs[:B // 2], costs[B // 2:])
    check_statistics(st, costs, cfg)
    assert st.best_rollout < B // 2


def closed_loop(Smpc, cfg, scn, cr, noise, seed, with_breakdown, ticks=10):
    g = Smpc(cfg)
    configure(g, scn, critics=cr, noise=noise)
    if noise is None:
        g.seed(seed)
    t, u, log = scn.tick, scn.u0, []
    for k in range(ticks):
        tk = Tick(t.pose_x + 0.02 * k, t.pose_y + 0.003 * k, t.pose_yaw, t.speed, t.path_x, t.path_y, t.path_yaw,
                  t.goal_x, t.goal_y)
        if with_breakdown:
            st = g.critic_stats(tk, u)
            assert st.batch == cfg.batch_size and st.scored_mask >> CONTROL & 1
        u, out = g.optimize(tk, u)
        log.append((u.copy(), tuple(getattr(out, n) for n in OUT_FIELDS), g.get_costs(), last_kernel(g)))
        u = shifted(u)
    return log


@pytest.mark.parametrize("B,T,kind,kernel", [(2000, 56, 0, "smpc_pass<"), (61440, 64, 1, "smpc_pass_lane<")],
                         ids=["wave-2000x56", "lane-61440x64"])
def test_a_breakdown_leaves_the_ticks_as_they_are(Smpc, B, T, kind, kernel):
    """A ten-tick moving-pose closed loop, plain and with a breakdown in front of every tick: u,
    every non-timing field of smpc_tick_out, the costs and the kernel the tick ran, bit for bit."""
    cfg, scn, noise = make_case(B, T)
    if kind == 1:
        noise = None                          # device RNG: the lane context keeps only the group-major noise
    plain = closed_loop(Smpc, cfg, scn, default_critics(), noise, 7, False)
    probed = closed_loop(Smpc, cfg, scn, default_critics(), noise, 7, True)
    assert plain[0][1][OUT_FIELDS.index("pass_kind")] == kind and plain[-1][3].startswith(kernel)
    assert any(p[1][OUT_FIELDS.index("passes")] == 1 for p in plain[1:]), "no tick speculated: the predictor is not exercised"
    for k, (a, b) in enumerate(zip(plain, probed)):
        assert np.array_equal(a[0], b[0]), f"tick {k}: u"
        assert a[1] == b[1], f"tick {k}: {dict(zip(OUT_FIELDS, a[1]))} != {dict(zip(OUT_FIELDS, b[1]))}"
        assert np.array_equal(a[2], b[2]), f"tick {k}: costs"
        assert a[3] == b[3], f"tick {k}: {a[3]} != {b[3]}"


def test_mask_semantics(Smpc):
    from mpcholonavigation_amd.optimizer import SmpcError, SmpcGroup
    B, T = 400, 15
    bit = {n: 1 << k for k, n in enumerate(ORDER)}
    # far from the goal / near it
    cfg, scn, noise = scene(B, T, "wall")
    g, far = breakdown(Smpc, cfg, scn, noise, critics(ORDER))
    assert not far.scored_mask & (bit["goal_angle"] | bit["goal"])
    assert far.scored_mask & bit["path_align"] and far.scored("PathAlignCritic") and not far.scored("GoalCritic")
    cfg_n, scn_n, noise_n = scene(B, T, "near")
    _, near = breakdown(Smpc, cfg_n, scn_n, noise_n, critics(ORDER))
    assert near.scored_mask & bit["goal_angle"] and near.scored_mask & bit["goal"]
    assert not near.scored_mask & (bit["path_align"] | bit["path_follow"] | bit["prefer_forward"])
    # a blocked path closes PathAlign's occupancy gate
    t = scn.tick
    valid = np.ones(len(t.path_x) - 1, np.uint8)
    valid[0:30] = 0
    blocked = Tick(t.pose_x, t.pose_y, t.pose_yaw, t.speed, t.path_x, t.path_y, t.path_yaw, t.goal_x, t.goal_y,
                   path_pts_valid=valid, goal_checker_xy_tolerance=0.25)
    st = g.critic_stats(blocked, scn.u0, per_rollout=True)
    assert st.scored_mask == far.scored_mask & ~(bit["path_align"] | bit["path_align_legacy"])
    assert not st.per_rollout[ORDER.index("path_align")].any()
    # every rollout collides: the rows of the re-score (the list up to the first collision critic)
    cfg_l, scn_l, noise_l = make_case(B, T, all_lethal=True)
    for names, kept in ((FIVE, ("obstacles",)), (ORDER, ("constraint", "cost"))):
        gl, st = breakdown(Smpc, cfg_l, scn_l, noise_l, critics(names))
        assert st.fail_flag and st.scored_mask == mask_of(kept), (names, bin(st.scored_mask))
        _, out = gl.optimize(scn_l.tick, scn_l.u0)
        assert out.fail_flag == 1
        rows = st.per_rollout.astype(np.float64)
        n = bin(st.scored_mask).count("1")
        assert np.all(np.abs(rows.sum(axis=0) - gl.get_costs()) <= (n + 1) * EPS * np.abs(rows).sum(axis=0))
    # the retry after fallback(): nothing is scored
    retry = Tick(t.pose_x, t.pose_y, t.pose_yaw, t.speed, t.path_x, t.path_y, t.path_yaw, t.goal_x, t.goal_y,
                 fail_flag_in=True)
    st = g.critic_stats(retry, scn.u0, per_rollout=True)
    assert st.scored_mask == 1 << CONTROL and st.fail_flag
    assert not st.per_rollout[:CONTROL].any() and st.per_rollout[CONTROL].any()
    g.optimize(retry, scn.u0)
    check_statistics(st, g.get_costs(), cfg)
    # a member of a group
    g2 = Smpc(cfg)
    configure(g2, scn, critics=critics(ORDER), noise=noise)
    grp = SmpcGroup([g, g2])
    with pytest.raises(SmpcError) as e:
        g.critic_stats(scn.tick, scn.u0)
    assert e.value.code == A.SMPC_ERR_STATE
    grp.close()
    assert g.critic_stats(scn.tick, scn.u0).scored_mask == far.scored_mask


def test_host_face_leaves_eval_control_alone():
    """sortham::Optimizer::getCriticStats followed by evalControl gives the Twist evalControl gives
    alone, tick after tick."""
    from mpcholonavigation_amd.host_optimizer import Optimizer
    B, T = 2000, 56
    cfg, scn, noise = make_case(B, T)
    hosts = []
    for _ in range(2):
        h = Optimizer(cfg, default_critics(), 20.0)
        h.set_costmap(scn.cells, scn.origin_x, scn.origin_y, scn.resolution)
        h.set_noise(*noise)
        hosts.append(h)
    t = scn.tick
    for k in range(4):
        tk = Tick(t.pose_x + 0.015 * k, t.pose_y, t.pose_yaw, (0.3, 0.0, 0.0), t.path_x, t.path_y, t.path_yaw,
                  t.goal_x, t.goal_y)
        st = hosts[1].critic_stats(tk, per_rollout=(k == 0))
        assert st.batch == B and st.scored("ObstaclesCritic") and st.scored("ControlCost") and not st.scored("CostCritic")
        assert 1.0 <= st.effective_samples <= B
        tw0, out0 = hosts[0].eval_control(tk)
        tw1, out1 = hosts[1].eval_control(tk)
        assert np.array_equal(tw0, tw1), (k, tw0, tw1)
        assert np.array_equal(hosts[0].get_control_sequence(), hosts[1].get_control_sequence())
        assert (out0.passes, out0.furthest_reached_path_point) == (out1.passes, out1.furthest_reached_path_point)
