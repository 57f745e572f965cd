"""smpc_critic_breakdown where tests/test_gpu_critic_stats.py does not reach: more than one slice
of the reduction, a footprint, a non-holonomic model, a lane context whose noise exists only
group-major.

A. Statistics across slices.  smpc_reduce_stats cuts the batch into slices of 16 384 rollouts, each
   with weights against its own least cost m_s; smpc_reduce_stats_final rescales them by
   2^(k2 (m_s - m)) and picks the batch's first least cost.  Judged by check_statistics (float64
   NumPy on the device's own rows and costs) at 16 384 (S = 1), 16 385 (S = 2, a last slice of one
   rollout, ld != B), 16 390 (the slice ends inside a quad), 32 769 (S = 3) and 1 048 581 rollouts
   (S = 65: the lane loop over slices takes a second trip, the pass's grid several), the best rollout
   steered to both sides of a slice edge, ties across slices, and a slice whose factor underflows.
   The bar stays check_statistics': log2(B) 2^-24 relative to the absolute sums.  Every case prints
   measured / bar for `weighted` and `effective_samples`; where one exceeds 1 the float32
   restatement (sliced_float32_statistics: a correctly rounded exp2) is printed next to it, which
   tells a defect of the kernels from the error of v_exp_f32.
B. consider_footprint on one collision critic (both is refused): rows against the oracle critic by
   critic, against the general and the lean tick, the closed-in scene, the refusal's error path, the
   host face.
C. DiffDrive and Ackermann: rows against the oracle, the Constraint row's turning-radius term at work.
D. SMPC_FLAG_LANE_PER_ROLLOUT contexts drawing with the device RNG: the breakdown itself makes the
   [B, T] copy of the group-major noise (ensure_row_major), also of the set a background draw
   swapped in — through the furthest-point pre-pass with the five critics, through score_rows' own
   call with a list that has no path critic.

The float32 CPU oracle is used in B, C and D only, at B <= 256 rollouts (C: 400)."""
import numpy as np
import pytest

from mpcholonavigation_amd import _abi as A
from mpcholonavigation_amd.synthetic import make_noise
from mpcholonavigation_amd.tick import Tick
from tests import softmax_model as sm
from tests.footprint_scenes import CIRCUMSCRIBED, FOOTPRINT, LAYER_SCALING, LISTS, critics_of, setup, wall_case
from tests.harness import FIVE, OUT_FIELDS, Oracle, Smpc, copy_of, last_kernel, shifted  # noqa: F401
from tests.helpers import configure, cost_flips
from tests.kernel_names import wave_at
from tests.stats_scenes import (CONTROL, EPS, NO_FURTHEST, ORDER, check_statistics, critics, mask_of, row_parity, scene,
                                slices_of, sliced_float32_statistics, statistics_ratios)

pytestmark = pytest.mark.gpu

DIFF, ACKER, OMNI = A.SMPC_MODEL_DIFF_DRIVE, A.SMPC_MODEL_ACKERMANN, A.SMPC_MODEL_OMNI
MODEL_NAME = {DIFF: "DiffDrive", ACKER: "Ackermann", OMNI: "Omni"}
SLICE = 16384


def rounding_bound(st):
    """test_rows_add_up_to_the_ticks_costs' bound on |sum of the rows - the general pass's cost|:
    one float rounding per stored term and one per chained add."""
    n = bin(st.scored_mask).count("1")
    return (n + 1) * EPS * np.abs(st.per_rollout.astype(np.float64)).sum(axis=0)


def control_row(st, u0, noise, cfg, T, model, label):
    """Row 12 against the float64 gamma formula, test_rows_match_the_oracle_critic_by_critic's bound."""
    ref = sm.gamma_terms(u0, noise, cfg, model)
    bound = (T + 5) * EPS * sm.gamma_magnitude(u0, noise, cfg, model) + 1e-30
    d = np.abs(st.per_rollout[CONTROL].astype(np.float64) - ref)
    print(f"[critic stats] {label} control row: max |d| / bound {float((d / bound).max()):.3f}")
    assert np.all(d <= bound), label


# ---- A. statistics across slices -------------------------------------------------------------------------

def wall_ctx(Smpc, B, T, power=1, seed=7, noise=None, flags=0):
    """A context of B rollouts on the wall scene with the twelve critics; noise from the device RNG
    (the scene is built for four rollouts: no host noise of the large batch is ever made)."""
    cfg, scn, _ = scene(4, T, "wall")
    cfg.batch_size = B
    cfg.flags |= flags
    g = Smpc(cfg)
    configure(g, scn, critics=critics(ORDER, power), noise=noise)
    if noise is None:
        g.seed(seed)
    return cfg, scn, g


def judged(g, cfg, scn, label, S):
    """critic_stats, then the tick; the ratios printed, then check_statistics.  -> (st, costs)"""
    B = cfg.batch_size
    assert slices_of(B) == (S, SLICE), label
    st = g.critic_stats(scn.tick, scn.u0, per_rollout=True)
    assert st.batch == B and not st.fail_flag and st.per_rollout.shape == (13, B)
    _, out = g.optimize(scn.tick, scn.u0)
    costs = g.get_costs()
    rw, re = statistics_ratios(st, costs, cfg)
    print(f"[critic stats reach] {label}: {S} slices, weighted {rw:.3f} effective_samples {re:.3f} of the bar; "
          f"effective samples {st.effective_samples:.2f}, best {st.best_rollout} in slice {st.best_rollout // SLICE}; "
          f"tick ran {last_kernel(g)}")
    if max(rw, re) > 1.0:
        fw, fe = statistics_ratios(st, costs, cfg, sliced_float32_statistics(st.per_rollout, costs, cfg))
        print(f"[critic stats reach] {label}: the float32 restatement: weighted {fw:.3f} effective_samples {fe:.3f} of the bar")
    check_statistics(st, costs, cfg)
    return st, costs


ACROSS = [(16384, 15, 1), (16385, 15, 2), (16390, 15, 2), (32769, 15, 3), (1048581, 15, 65), (16385, 128, 2)]


@pytest.mark.parametrize("B,T,S", ACROSS, ids=[f"{b}x{t}" for b, t, _ in ACROSS])
def test_statistics_across_slices(Smpc, B, T, S):
    """The ratios measured on an MI355X (error / bar, `weighted` then `effective_samples`) are in
    DESIGN.md 7; the bar is check_statistics' own."""
    cfg, scn, g = wall_ctx(Smpc, B, T)
    st, costs = judged(g, cfg, scn, f"{B}x{T}", S)
    assert st.scored_mask & 1 << ORDER.index("path_align") and st.scored_mask >> CONTROL & 1


@pytest.mark.parametrize("B,T", [(16385, 15), (1048581, 15)], ids=["16385x15", "1048581x15"])
def test_rows_add_up_to_the_ticks_costs_across_slices(Smpc, B, T):
    """test_rows_add_up_to_the_ticks_costs with its bound, every rollout: at 16 385 the rows' leading
    dimension (16 388) is not the batch, at 1 048 581 the pass's grid takes several trips."""
    # (cost_power 2: the tick itself runs the general pass; the large batch is kept off the lane pass)
    cfg, scn, g = wall_ctx(Smpc, B, T, power=2, flags=A.SMPC_FLAG_WAVE_PER_ROLLOUT if B > 61440 else 0)
    st = g.critic_stats(scn.tick, scn.u0, per_rollout=True)
    _, out = g.optimize(scn.tick, scn.u0)
    print(f"[critic stats reach] rows add up {B}x{T}: tick ran {last_kernel(g)}")
    assert last_kernel(g).startswith("smpc_pass<") and out.pass_kind == 0
    costs = g.get_costs().astype(np.float64)
    err = np.abs(st.per_rollout.astype(np.float64).sum(axis=0) - costs)
    bound = rounding_bound(st)
    print(f"[critic stats reach] rows add up {B}x{T}: {bin(st.scored_mask).count('1')} rows, max err / bound "
          f"{float((err / np.maximum(bound, 1e-300)).max()):.3f}")
    assert np.all(err <= bound)
    assert st.best_cost == np.float32(costs.min()) and st.best_rollout == int(np.argmin(costs))


@pytest.fixture(scope="module")
def drawn(Smpc):
    """One tick of 32 769 rollouts (three slices) on the device RNG's noise: (cfg, scn, the noise,
    its costs, the breakdown).  Shared and read only."""
    B, T = 32769, 15
    cfg, scn, g = wall_ctx(Smpc, B, T)
    st = g.critic_stats(scn.tick, scn.u0)
    g.optimize(scn.tick, scn.u0)
    noise = tuple(g.get_noise())
    return cfg, scn, noise, g.get_costs(), st


@pytest.mark.parametrize("target", [0, 16383, 16384, 32768])
def test_best_rollout_steered_across_the_slices(Smpc, drawn, target):
    """The best rollout's three noise rows change places with those of `target`: a rollout's cost
    depends on its own noise only, so `target` is now the best, at_best is its column and best_cost
    is what it was, bit for bit.  0; 16 383 and 16 384, the two sides of a slice edge; B - 1, alone
    in the ragged last slice."""
    cfg, scn, noise, costs0, st0 = drawn
    b = int(np.argmin(costs0))
    assert st0.best_rollout == b
    swapped = [n.copy() for n in noise]
    for n in swapped:
        n[[b, target]] = n[[target, b]]
    _, _, g = wall_ctx(Smpc, cfg.batch_size, cfg.time_steps, noise=swapped)
    st, costs = judged(g, cfg, scn, f"steered from {b} to {target}", 3)
    assert st.best_rollout == target
    assert np.array_equal(st.at_best, st.per_rollout[:, target])
    assert np.float32(st.best_cost) == np.float32(st0.best_cost) == costs0[b] == costs[target]
    assert np.array_equal(costs[[b, target]], costs0[[target, b]])


def test_ties_across_slices(Smpc, drawn):
    """The best rollout's noise copied to one rollout of each other slice: the best rollout is the
    lowest index among them."""
    cfg, scn, noise, costs0, _ = drawn
    b = int(np.argmin(costs0))
    picks = {0: 12345, 1: SLICE + 77, 2: 2 * SLICE}       # (slice 2 has one rollout)
    picks[b // SLICE] = b
    tied = [n.copy() for n in noise]
    for n in tied:
        for i in picks.values():
            n[i] = n[b]
    _, _, g = wall_ctx(Smpc, cfg.batch_size, cfg.time_steps, noise=tied)
    st, costs = judged(g, cfg, scn, f"ties at {sorted(picks.values())}", 3)
    assert len(set(costs[list(picks.values())])) == 1 and costs[b] == costs0[b]
    assert st.best_rollout == min(picks.values())
    assert int(np.sum(costs == costs.min())) == 3


def test_ties_in_one_lane_of_the_last_reduction(Smpc):
    """smpc_reduce_stats_final gives slice s to lane s % 64: only from 65 slices on does a lane compare
    two slices itself (0 and 64) before the wave does.  At 1 048 581 rollouts the best rollout's noise
    goes to one rollout of slice 0 and to the last rollout, in slice 64: the best is the one in slice 0."""
    B, T = 1048581, 15
    cfg, scn, g = wall_ctx(Smpc, B, T)
    g.optimize(scn.tick, scn.u0)
    b = int(np.argmin(g.get_costs()))
    assert b // SLICE not in (0, 64), "pick another seed: the best rollout must lie between the two"
    noise = g.get_noise()
    for n in noise:
        n[7] = n[B - 1] = n[b]
    g.set_noise(*noise)
    st, costs = judged(g, cfg, scn, f"ties at [7, {b}, {B - 1}]", 65)
    assert costs[7] == costs[b] == costs[B - 1] == costs.min()
    assert st.best_rollout == 7 and np.array_equal(st.at_best, st.per_rollout[:, 7])


def test_tied_minima_with_the_twin_in_another_slice(Smpc):
    """test_statistics_with_tied_minima's construction at 32 768 rollouts: every rollout's twin sits
    16 384 further on, in the other slice."""
    B, T = 32768, 15
    cfg, scn, noise = scene(B // 2, T, "wall")
    cfg.batch_size = B
    noise = tuple(np.concatenate([n, n]) for n in noise)
    _, _, g = wall_ctx(Smpc, B, T, noise=noise)
    st, costs = judged(g, cfg, scn, f"twins {B}x{T}", 2)
    assert np.array_equal(costs[:B // 2], costs[B // 2:])
    assert st.best_rollout < B // 2


def test_a_slice_that_contributes_nothing(Smpc, drawn):
    """Every rollout of the middle slice gets the noise of a colliding rollout: the slice's factor
    2^(k2 (m_s - m)) underflows to 0, `weighted` and `effective_samples` still meet the model, and
    min, max and sum still see the slice.
    (No rollout of the device's draw collides on this scene at 15 steps — the oracle on the same
    Philox streams counts 32 769 of 32 769 clear — so the colliding rollout is built: no vx or wz
    noise and vy noise 0.5 m/s at every step, which carries it into the wall; that it collides is
    asserted on the device's costs.)"""
    cfg, scn, noise, costs0, _ = drawn
    filled = [n.copy() for n in noise]
    for n, v in zip(filled, (0.0, 0.5, 0.0)):
        n[SLICE:2 * SLICE] = v
    _, _, g = wall_ctx(Smpc, cfg.batch_size, cfg.time_steps, noise=filled)
    st, costs = judged(g, cfg, scn, "a colliding middle slice", 3)
    inside = costs[SLICE:2 * SLICE]
    assert np.all(inside == inside[0]) and inside[0] > 1.0e4, inside[:4]
    k2 = float(np.float32(-1.0) / np.float32(cfg.temperature)) * 1.4426950408889634
    assert k2 * (float(inside[0]) - float(costs.min())) < -200.0            # (2^-149 is the least float)
    assert not SLICE <= st.best_rollout < 2 * SLICE
    coll = ORDER.index("cost")
    assert st.max[coll] == st.per_rollout[coll, SLICE] > st.per_rollout[coll, :SLICE].max()
    outside = np.r_[0:SLICE, 2 * SLICE:cfg.batch_size]
    assert st.sum[coll] > 2.0 * st.per_rollout[coll, outside].astype(np.float64).sum()


# ---- B. a footprint ------------------------------------------------------------------------------------------

FP_SHAPES = [(256, 56), (128, 100), (64, 200)]       # R = 1, 2 and 4, each ragged


def footprint_ctx(Smpc, which, B, T, power, closed_in=False, footprint=True):
    names, coll = LISTS[which]
    cfg, scn, noise = wall_case(B, T, closed_in=closed_in)
    cr = critics_of(names, power, (coll,) if footprint else ())
    return cfg, scn, noise, cr, setup(Smpc(cfg), scn, cr, noise)


@pytest.mark.parametrize("power", [1, 2])
@pytest.mark.parametrize("which", ["deployed", "five"])
@pytest.mark.parametrize("B,T", FP_SHAPES, ids=[f"{b}x{t}" for b, t in FP_SHAPES])
def test_footprint_rows_match_the_oracle_critic_by_critic(Smpc, Oracle, B, T, which, power):
    """test_rows_match_the_oracle_critic_by_critic with consider_footprint on the list's collision
    critic: the oracle scores each critic alone with gamma = 0 and the same footprint.  The seed is
    make_case's default (1234), the first one tried: the totals flip nowhere on these shapes."""
    names, coll = LISTS[which]
    cfg, scn, noise, cr, g = footprint_ctx(Smpc, which, B, T, power)
    o = setup(Oracle(cfg), scn, cr, noise)
    _, og = g.optimize(scn.tick, scn.u0)
    _, oo = o.optimize(scn.tick, scn.u0)
    assert og.fail_flag == oo.fail_flag == 0
    flips = cost_flips(g.get_costs(), o.get_costs())
    print(f"[critic stats reach] footprint {which} {B}x{T} power {power}: {flips} flips of the totals, "
          f"{oo.non_colliding} of {B} clear, tick ran {last_kernel(g)}")
    assert flips == 0, "pick another seed: the totals already flip"
    assert 0 < oo.non_colliding < B and og.non_colliding == oo.non_colliding
    st = g.critic_stats(scn.tick, scn.u0, per_rollout=True)
    assert st.batch == B and not st.fail_flag
    cfg0 = copy_of(cfg, gamma=0.0)
    for k, n in enumerate(ORDER):
        if n not in names:
            assert not st.scored_mask >> k & 1 and not st.per_rollout[k].any(), n
            continue
        o1 = setup(Oracle(cfg0), scn, critics_of((n,), power, (n,) if n == coll else ()), noise)
        o1.optimize(scn.tick, scn.u0)
        ref = o1.get_costs()
        row_parity(st.per_rollout[k], ref, T, f"footprint {which} {B}x{T} power {power} {n}")
        if not st.scored_mask >> k & 1:
            assert not st.per_rollout[k].any() and not ref.any(), n
    assert st.scored_mask >> ORDER.index(coll) & 1 and st.scored_mask >> ORDER.index("path_follow") & 1
    control_row(st, scn.u0, noise, cfg, T, OMNI, f"footprint {which} {B}x{T}")
    # the footprint decides rollouts: the same row without it is another one
    _, _, _, _, g0 = footprint_ctx(Smpc, which, B, T, power, footprint=False)
    plain = g0.critic_stats(scn.tick, scn.u0, per_rollout=True).per_rollout[ORDER.index(coll)]
    assert int(np.sum(plain != st.per_rollout[ORDER.index(coll)])) >= B // 10


@pytest.mark.parametrize("power", [1, 2])
@pytest.mark.parametrize("which", ["deployed", "five"])
@pytest.mark.parametrize("B,T", FP_SHAPES, ids=[f"{b}x{t}" for b, t in FP_SHAPES])
def test_footprint_rows_add_up_to_the_ticks_costs(Smpc, B, T, which, power):
    """cost_power 2: the tick runs the general pass, whose arithmetic the breakdown repeats — the
    rounding bound of test_rows_add_up_to_the_ticks_costs.  cost_power 1: the tick runs the lean
    footprint instance smpc_pass<R, 4, FULL>, another kernel — the float64 sum of the rows against
    its costs under row_parity's bar."""
    cfg, scn, noise, cr, g = footprint_ctx(Smpc, which, B, T, power)
    st = g.critic_stats(scn.tick, scn.u0, per_rollout=True)
    _, out = g.optimize(scn.tick, scn.u0)
    costs = g.get_costs()
    total = st.per_rollout.astype(np.float64).sum(axis=0)
    print(f"[critic stats reach] footprint {which} {B}x{T} power {power}: tick ran {last_kernel(g)}")
    assert out.pass_kind == 0 and out.fail_flag == 0 and last_kernel(g) == wave_at(T, 4 if power == 1 else 2)
    if power == 2:
        err, bound = np.abs(total - costs), rounding_bound(st)
        print(f"[critic stats reach] footprint rows add up: max err / bound {float((err / np.maximum(bound, 1e-300)).max()):.3f}")
        assert np.all(err <= bound)
        check_statistics(st, costs, cfg)
    else:
        row_parity(costs, total, T, f"footprint {which} {B}x{T}: lean tick against the rows")


@pytest.mark.parametrize("power", [1, 2])
@pytest.mark.parametrize("which,kept", [("deployed", ("constraint", "cost")), ("five", ("obstacles",))])
def test_every_footprint_collides(Smpc, which, kept, power):
    """wall_case(closed_in=True): the outline lies on the walls from the first pose on.  The
    breakdown reports the failed tick — fail_flag, and exactly the list up to the collision critic
    scored — and its rows add up to that tick's costs (the rounding bound where the tick re-scores
    on the general pass, row_parity's bar where it does on the lean instance)."""
    B, T = 256, 56
    cfg, scn, noise, cr, g = footprint_ctx(Smpc, which, B, T, power, closed_in=True)
    st = g.critic_stats(scn.tick, scn.u0, per_rollout=True)
    assert st.fail_flag and st.scored_mask == mask_of(kept), bin(st.scored_mask)
    _, out = g.optimize(scn.tick, scn.u0)
    print(f"[critic stats reach] closed in {which} power {power}: tick ran {last_kernel(g)}, {out.passes} passes")
    assert out.fail_flag == 1 and out.non_colliding == 0
    costs = g.get_costs()
    total = st.per_rollout.astype(np.float64).sum(axis=0)
    if power == 2:
        assert last_kernel(g) == wave_at(T, 2)
        assert np.all(np.abs(total - costs) <= rounding_bound(st))
    else:
        assert last_kernel(g) == wave_at(T, 4)
        row_parity(costs, total, T, f"closed in {which}: lean tick against the rows")
    for k, n in enumerate(ORDER):
        assert n in kept or not st.per_rollout[k].any(), n
    hit = st.per_rollout[ORDER.index(kept[-1])]
    assert hit.min() == hit.max() > 0.0        # every rollout pays the collision cost
    # without the footprint nothing fails
    _, _, _, _, g0 = footprint_ctx(Smpc, which, B, T, power, closed_in=True, footprint=False)
    assert not g0.critic_stats(scn.tick, scn.u0).fail_flag


def moving_ticks(g, scn, before=None, ticks=10):
    t, u, log = scn.tick, scn.u0, []
    for k in range(ticks):
        tk = Tick(t.pose_x + 0.02 * k, t.pose_y + 0.003 * k, t.pose_yaw, t.speed, t.path_x, t.path_y, t.path_yaw,
                  t.goal_x, t.goal_y)
        if before:
            before(tk, u)
        u, out = g.optimize(tk, u)
        log.append((u.copy(), tuple(getattr(out, n) for n in OUT_FIELDS), g.get_costs(), last_kernel(g)))
        u = shifted(u)
    return log


def same_ticks(plain, probed):
    for k, (a, b) in enumerate(zip(plain, probed)):
        assert np.array_equal(a[0], b[0]), f"tick {k}: u"
        assert a[1] == b[1], f"tick {k}: {dict(zip(OUT_FIELDS, a[1]))} != {dict(zip(OUT_FIELDS, b[1]))}"
        assert np.array_equal(a[2], b[2]), f"tick {k}: costs"
        assert a[3] == b[3], f"tick {k}: {a[3]} != {b[3]}"


def test_both_collision_critics_with_a_footprint_are_refused_and_nothing_moves(Smpc):
    """SMPC_ERR_UNSUPPORTED with its message — after prepare_tick has already run for the refused
    call.  Ten moving-pose ticks with a refused call in front of each are bit for bit those of a
    twin that never asked: u, the non-timing fields of the result block, the costs, the kernel."""
    from mpcholonavigation_amd.optimizer import SmpcError
    B, T = 256, 56
    names = LISTS["deployed"][0] + ("obstacles",)
    cfg, scn, noise = wall_case(B, T)
    cr = critics_of(names, footprint=("cost", "obstacles"))
    g, twin = (setup(Smpc(cfg), scn, cr, noise) for _ in range(2))
    refused = []

    def ask(tk, u):
        with pytest.raises(SmpcError) as e:
            g.critic_stats(tk, u, per_rollout=True)
        assert e.value.code == A.SMPC_ERR_UNSUPPORTED
        assert "critic breakdown: consider_footprint=true with both ObstaclesCritic and CostCritic in the list" in str(e.value)
        refused.append(1)

    plain = moving_ticks(twin, scn)
    probed = moving_ticks(g, scn, before=ask)
    print(f"[critic stats reach] refused {len(refused)} times; ticks ran {sorted({p[3] for p in plain})}, "
          f"passes {[p[1][OUT_FIELDS.index('passes')] for p in plain]}")
    assert len(refused) == 10 and plain[0][1][OUT_FIELDS.index("fail_flag")] == 0
    same_ticks(plain, probed)
    # (either switch refuses while both critics are in the list); without ObstaclesCritic the same context answers
    g.set_critics(critics_of(names, footprint=("cost",)))
    with pytest.raises(SmpcError):
        g.critic_stats(scn.tick, scn.u0)
    g.set_critics(critics_of(LISTS["deployed"][0], footprint=("cost",)))
    st = g.critic_stats(scn.tick, scn.u0)
    assert st.scored("CostCritic") and not st.scored("ObstaclesCritic") and not st.fail_flag


DEPLOYED_CLASSES = ["ConstraintCritic", "CostCritic", "GoalCritic", "GoalAngleCritic", "PathAlignCritic",
                    "PathFollowCritic", "PathAngleCritic", "PreferForwardCritic", "TwirlingCritic"]


def test_host_face_with_a_footprint_leaves_eval_control_alone():
    """test_host_face_leaves_eval_control_alone on the deployed list with CostCritic's footprint:
    getCriticStats reports CostCritic scored, evalControl afterwards gives the twin's Twist."""
    from mpcholonavigation_amd.host_optimizer import Optimizer
    B, T = 2000, 56
    cfg, scn, noise = wall_case(B, T)
    cr = critics_of(LISTS["deployed"][0], footprint=("cost",))
    hosts = []
    for _ in range(2):
        h = Optimizer(cfg, cr, 20.0, critics=DEPLOYED_CLASSES)
        h.set_footprint(FOOTPRINT, CIRCUMSCRIBED, LAYER_SCALING)
        h.set_costmap(scn.cells, scn.origin_x, scn.origin_y, scn.resolution)
        h.set_noise(*noise)
        hosts.append(h)
    t = scn.tick
    for k in range(4):
        tk = Tick(t.pose_x + 0.015 * k, t.pose_y, t.pose_yaw, (0.3, 0.0, 0.0), t.path_x, t.path_y, t.path_yaw,
                  t.goal_x, t.goal_y)
        st = hosts[1].critic_stats(tk, per_rollout=(k == 0))
        assert st.batch == B and st.scored("CostCritic") and st.scored("ControlCost") and not st.scored("ObstaclesCritic")
        assert not st.fail_flag and 1.0 <= st.effective_samples <= B
        if k == 0:      # the footprint is in the row: some rollouts pay CostCritic's collision cost, some do not
            row = st.per_rollout[ORDER.index("cost")]
            assert 10 <= int(np.sum(row == row.max())) < B
        tw0, out0 = hosts[0].eval_control(tk)
        tw1, out1 = hosts[1].eval_control(tk)
        assert np.array_equal(tw0, tw1), (k, tw0, tw1)
        assert np.array_equal(hosts[0].get_control_sequence(), hosts[1].get_control_sequence())
        assert (out0.passes, out0.furthest_reached_path_point, out0.non_colliding, out0.min_cost) == \
            (out1.passes, out1.furthest_reached_path_point, out1.non_colliding, out1.min_cost)


# ---- C. DiffDrive and Ackermann ------------------------------------------------------------------------

def nonholonomic_case(B, T, kind, model):
    """scene() for a model without vy (vy_max = 0, vy_std = 0), minimum turning radius 0.5 m; the
    control sequence turns at 0.25 m/s and +-0.9 rad/s over the first half of the horizon (radius
    0.28 m: inside the minimum, test_gpu_parity.py::test_non_holonomic_motion_models_parity) and
    carries a stale vy row, which such a model neither reads nor writes."""
    cfg, scn, _ = scene(B, T, kind)
    cfg = copy_of(cfg, motion_model=model, vy_max=0.0, vy_std=0.0, ackermann_min_turning_r=0.5)
    noise = make_noise(B, T, std=(cfg.vx_std, 0.0, cfg.wz_std), seed=1234)
    u0 = scn.u0.copy()
    u0[1] = 0.123
    u0[0, :T // 2] = 0.25
    u0[2, :T // 2] = np.where(np.arange(T // 2) % 8 < 4, 0.9, -0.9)
    return cfg, scn, noise, u0


@pytest.mark.parametrize("kind", ["wall", "near"])
@pytest.mark.parametrize("power", [1, 2])
@pytest.mark.parametrize("model", [DIFF, ACKER], ids=["DiffDrive", "Ackermann"])
@pytest.mark.parametrize("B,T", [(400, 15), (200, 128)], ids=["400x15", "200x128"])
def test_nonholonomic_rows_match_the_oracle(Smpc, Oracle, B, T, model, power, kind):
    """test_rows_match_the_oracle_critic_by_critic for the two models without vy, the twelve
    critics.  Ackermann: ConstraintCritic also pays min_turning_r - |vx| / |wz| per step
    (con_acker_r); its row is non-zero for at least a tenth of the rollouts and is not DiffDrive's.
    The seed is make_noise's default (1234), the first one tried."""
    cfg, scn, noise, u0 = nonholonomic_case(B, T, kind, model)
    cr = critics(ORDER, power)
    g, o = Smpc(cfg), Oracle(cfg)
    for obj in (g, o):
        configure(obj, scn, critics=cr, noise=noise)
    _, og = g.optimize(scn.tick, u0)
    _, oo = o.optimize(scn.tick, u0)
    assert og.fail_flag == oo.fail_flag == 0
    label = f"{MODEL_NAME[model]} {B}x{T} {kind} power {power}"
    flips = cost_flips(g.get_costs(), o.get_costs())
    print(f"[critic stats reach] {label}: {flips} flips of the totals, tick ran {last_kernel(g)}")
    assert flips == 0, "pick another seed: the totals already flip"
    st = g.critic_stats(scn.tick, u0, per_rollout=True)
    assert st.batch == B and not st.fail_flag
    cfg0 = copy_of(cfg, gamma=0.0)
    scored = 0
    for k, n in enumerate(ORDER):
        o1 = Oracle(cfg0)
        configure(o1, scn, critics=critics((n,), power), noise=noise)
        o1.optimize(scn.tick, u0)
        ref = o1.get_costs()
        row_parity(st.per_rollout[k], ref, T, f"{label} {n}")
        if not st.scored_mask >> k & 1:
            assert not st.per_rollout[k].any() and not ref.any(), n
        else:
            scored += 1
    assert scored >= 5 and st.scored_mask & 1
    control_row(st, u0, noise, cfg, T, model, label)
    if model == ACKER:
        row = st.per_rollout[0]
        cfg_d = copy_of(cfg, motion_model=DIFF)
        gd = Smpc(cfg_d)
        configure(gd, scn, critics=cr, noise=noise)
        row_d = gd.critic_stats(scn.tick, u0, per_rollout=True).per_rollout[0]
        print(f"[critic stats reach] {label}: Constraint row non-zero for {int(np.sum(row != 0))} of {B}, "
              f"differs from DiffDrive's for {int(np.sum(row != row_d))}")
        assert int(np.sum(row != 0)) >= B // 10
        assert int(np.sum(row > row_d)) >= B // 10


# ---- D. lane contexts with the device RNG's noise -----------------------------------------------------

LANE_SHAPES = [(192, 64), (130, 56), (257, 60)]     # whole groups; ragged horizon, partial group; the noise tests' shape
# a list without a path critic: no furthest-point pre-pass runs in front of the stats pass, and that
# pre-pass relayouts the noise itself (launch_furthest) — here only score_rows' own call does
LANE_LISTS = {"five": FIVE, "no-path-critic": NO_FURTHEST}


def lane_ctx(Smpc, B, T, model, seed=7, names=FIVE):
    cfg, scn, _ = scene(4, T, "wall")
    cfg = copy_of(cfg, batch_size=B, motion_model=model, flags=cfg.flags | A.SMPC_FLAG_LANE_PER_ROLLOUT)
    g = Smpc(cfg)
    configure(g, scn, critics=critics(names, 1))
    g.seed(seed)
    return cfg, scn, g


def rows_against_the_oracle(Oracle, st, cfg, scn, noise, label, u0=None, names=FIVE):
    """Every row of a breakdown of the list `names` against the oracle on `noise` (row_parity), the control row
    against the float64 formula."""
    T = cfg.time_steps
    u0 = scn.u0 if u0 is None else u0
    cfg0 = copy_of(cfg, gamma=0.0, flags=0)
    for k, n in enumerate(ORDER):
        if n not in names:
            assert not st.scored_mask >> k & 1 and not st.per_rollout[k].any(), n
            continue
        o1 = Oracle(cfg0)
        configure(o1, scn, critics=critics((n,), 1), noise=noise)
        o1.optimize(scn.tick, u0)
        ref = o1.get_costs()
        row_parity(st.per_rollout[k], ref, T, f"{label} {n}")
        if not st.scored_mask >> k & 1:
            assert not st.per_rollout[k].any() and not ref.any(), n
    for n in ("obstacles", "path_align", "path_follow", "prefer_forward"):
        assert n not in names or st.scored_mask >> ORDER.index(n) & 1, n
    control_row(st, u0, noise, cfg, T, cfg.motion_model, label)


@pytest.mark.parametrize("which", list(LANE_LISTS))
@pytest.mark.parametrize("model", [OMNI, DIFF], ids=["Omni", "DiffDrive"])
@pytest.mark.parametrize("B,T", LANE_SHAPES, ids=[f"{b}x{t}" for b, t in LANE_SHAPES])
def test_lane_context_rows_on_device_noise(Smpc, Oracle, B, T, model, which):
    """The breakdown comes FIRST: the draw filled the group-major tensors only, so the [B, T] copy
    the stats pass reads is the one the breakdown makes.  Then get_noise, the oracle on that noise,
    and the tick, which runs a lane-pass instance: its costs against the rows' float64 sum under
    row_parity's bar.  Both lists: with the five the furthest-point pre-pass asks for the copy, without a
    path critic score_rows does."""
    names = LANE_LISTS[which]
    cfg, scn, g = lane_ctx(Smpc, B, T, model, names=names)
    st = g.critic_stats(scn.tick, scn.u0, per_rollout=True)
    assert st.batch == B and not st.fail_flag
    noise = g.get_noise()
    assert noise[0].any() and noise[2].any() and noise[1].any() == (model == OMNI)
    label = f"lane context {MODEL_NAME[model]} {B}x{T} {which}"
    rows_against_the_oracle(Oracle, st, cfg, scn, noise, label, names=names)
    _, out = g.optimize(scn.tick, scn.u0)
    print(f"[critic stats reach] {label}: tick ran {last_kernel(g)}")
    assert out.pass_kind == 1 and last_kernel(g).startswith("smpc_pass_lane") and out.fail_flag == 0
    costs = g.get_costs()
    row_parity(costs, st.per_rollout.astype(np.float64).sum(axis=0), T, f"{label}: lane tick against the rows")
    assert np.array_equal(st.at_best, st.per_rollout[:, st.best_rollout])
    assert np.array_equal(st.min, st.per_rollout.min(axis=1)) and np.array_equal(st.max, st.per_rollout.max(axis=1))


@pytest.mark.parametrize("which", list(LANE_LISTS))
@pytest.mark.parametrize("model", [OMNI, DIFF], ids=["Omni", "DiffDrive"])
@pytest.mark.parametrize("B,T", LANE_SHAPES, ids=[f"{b}x{t}" for b, t in LANE_SHAPES])
def test_lane_context_rows_with_a_background_draw_pending(Smpc, Oracle, B, T, model, which):
    """seed, tick, redraw_noise_async, breakdown, tick: the breakdown takes the new epoch's tensors
    (absorb_redraw) and relayouts THAT set.  The second tick is bit for bit the one of a twin that
    made the same calls without the breakdown; the rows match the oracle on the noise get_noise
    returns after that tick, which is the new epoch's."""
    runs, names = [], LANE_LISTS[which]
    for ask in (False, True):
        cfg, scn, g = lane_ctx(Smpc, B, T, model, names=names)
        u, _ = g.optimize(scn.tick, scn.u0)
        g.redraw_noise_async()
        st = g.critic_stats(scn.tick, u, per_rollout=True) if ask else None
        u2, out = g.optimize(scn.tick, u)
        runs.append((u2, tuple(getattr(out, n) for n in OUT_FIELDS), g.get_costs(), last_kernel(g)))
    same_ticks(runs[:1], runs[1:])
    label = f"pending draw {MODEL_NAME[model]} {B}x{T} {which}"
    print(f"[critic stats reach] {label}: second tick ran {runs[1][3]}")
    assert runs[1][3].startswith("smpc_pass_lane")
    noise = g.get_noise()
    _, _, g_old = lane_ctx(Smpc, B, T, model)
    old = g_old.get_noise()
    assert not np.array_equal(old[0], noise[0]) and not np.array_equal(old[2], noise[2])
    rows_against_the_oracle(Oracle, st, cfg, scn, noise, label, u0=u, names=names)
    row_parity(runs[1][2], st.per_rollout.astype(np.float64).sum(axis=0), T, f"{label}: lane tick against the rows")


@pytest.mark.parametrize("model", [OMNI, DIFF], ids=["Omni", "DiffDrive"])
@pytest.mark.parametrize("B,T", LANE_SHAPES, ids=[f"{b}x{t}" for b, t in LANE_SHAPES])
def test_lane_context_rows_are_those_of_the_unfused_fill(Smpc, monkeypatch, B, T, model):
    """SMPC_NO_FUSED_FILL=1: the draw fills [B, T] and relayouts the other way.  The same rows and
    statistics, bit for bit, also for the set a background draw swaps in."""
    res = []
    for unfused in (False, True):
        if unfused:
            monkeypatch.setenv("SMPC_NO_FUSED_FILL", "1")
        cfg, scn, g = lane_ctx(Smpc, B, T, model)
        first = g.critic_stats(scn.tick, scn.u0, per_rollout=True)
        g.redraw_noise_async()
        second = g.critic_stats(scn.tick, scn.u0, per_rollout=True)
        res.append((first, second, g.get_noise()))
    monkeypatch.delenv("SMPC_NO_FUSED_FILL")
    (f1, f2, fn), (u1, u2, un) = res
    for a, b in zip(fn, un):
        assert np.array_equal(a, b)
    assert not np.array_equal(f1.per_rollout, f2.per_rollout)       # (another epoch)
    for a, b in ((f1, u1), (f2, u2)):
        assert np.array_equal(a.per_rollout, b.per_rollout)
        assert (a.scored_mask, a.best_rollout, a.best_cost, a.effective_samples) == \
            (b.scored_mask, b.best_rollout, b.best_cost, b.effective_samples)
        for f in ("sum", "min", "max", "weighted", "at_best"):
            assert np.array_equal(getattr(a, f), getattr(b, f)), f
