"""Every scoring pass at the longest plan its LDS layout admits, against the strict oracle.

Each pass copies the plan into LDS next to the costmap window, the lookup table and the per-wave
scratch; plan_launch compares the layout's total with 160 KB and lets a tick whose lane-pass layout
no longer fits fall to the wave pass.  At the limit the last wave's scratch ends at the last byte
of the CU's LDS, and nothing faults where a region is one element short: an LDS write out of range
is dropped, a read returns 0, and some waves' costs are slightly wrong.  Only parity at the exact
limit sees that.

Every case takes its P from the layout export (tests/plan_scenes.py: lane_limit, split_limit,
plan_limit — P* below), asserts the pass and the instance it judged (pass_kind and
smpc_debug_last_pass_kernel), and applies tests.helpers.assert_parity with the per-rollout costs at
the bar of test_gpu_properties.py::test_path_length_edges: rtol 1e-4 on the Twist, integer outputs
exact, max_flips=1.  The plans (long, short, lethal, near) are described in tests/plan_scenes.py.

Batches: 2048 with the lane flag launches half blocks (four waves); 70 000 is more than four groups
per CU, so all eight waves' scratch is live, including the slice that ends at the last byte.

PathAlign sample counts of the wave-pass cases: make_lds switches the segment width at 15 / 16 and
31 / 32 samples (nsamp = (T - 1) / trajectory_point_step).  With T in {100, 128, 200, 256} the counts
15, 16 and 31 are reachable, 32 is not (it needs T - 1 in [32 s, 33 s)): the cases use the nearest
count on either side of each switch, 14..18 and 28..36.

The last test is not marked gpu: every scene here must give the same integer outputs, and parity
at the same bar, on the strict oracle and on the oracle built with the reference's -ffast-math
flags, and the two builds may not differ in a cell lookup that assert_parity cannot see yet that
weighs on the Twist (plan_scenes.hidden_flip_influence).  A scene on which the two reference builds
disagree is a knife edge and proves nothing; such a scene got another noise seed
(plan_scenes.RESEEDED), nothing else."""
import numpy as np
import pytest

from mpcholonavigation_amd import _abi as A
from tests import plan_scenes as S
from tests.harness import Smpc, last_kernel, scan_count  # noqa: F401
from tests.helpers import assert_parity
from tests.kernel_names import LANE_ROW, LANE_ROW_NO_OBST, lane, lane_nh, lane_pow, wave_at
from tests.plan_scenes import DEPLOYED, FIVE, NO_OBST, scene

gpu = pytest.mark.gpu
DIFF = A.SMPC_MODEL_DIFF_DRIVE


def lane_cases():
    """Parking form, the five critics: at, below and above the limit; every horizon form; both batches;
    the same without ObstaclesCritic at its own limit."""
    out = []
    for tag, names, rows, obst in (("five", FIVE, LANE_ROW, True), ("no-obst", NO_OBST, LANE_ROW_NO_OBST, False)):
        p = S.lane_limit(64, obst)
        for plan in ("long", "short"):
            out.append(scene(f"lane-{tag}-64-P*-1-{plan}", 2048, 64, p - 1, plan, names, kernel=rows[64]))
            out.append(scene(f"lane-{tag}-64-P*-{plan}", 2048, 64, p, plan, names, kernel=rows[64]))
            out.append(scene(f"lane-{tag}-64-P*+1-{plan}", 2048, 64, p + 1, plan, names, kind=0, kernel=wave_at(64, 0)))
        out.append(scene(f"lane-{tag}-64-P*-lethal", 2048, 64, p, "lethal", names, kernel=rows[64]))
        for plan in ("long", "short"):
            out.append(scene(f"lane-{tag}-64-P*-{plan}-70000", 70000, 64, p, plan, names, kernel=rows[64]))
        out.append(scene(f"lane-{tag}-64-P*+1-short-70000", 70000, 64, p + 1, "short", names, kind=0, kernel=wave_at(64, 0)))
        for T in (56, 40, 30):
            pt = S.lane_limit(T, obst)
            out.append(scene(f"lane-{tag}-{T}-P*-short", 2048, T, pt, "short", names, kernel=rows[T]))
            out.append(scene(f"lane-{tag}-{T}-P*+1-short", 2048, T, pt + 1, "short", names, kind=0, kernel=wave_at(T, 0)))
    return out


def row_cases():
    """The other rows of the lane tables at P*: GoalAngle, the deployed list, cost powers, no vy
    stream, the re-read form."""
    p = S.lane_limit(64)
    pow_row = lane_pow()
    nh_row = lane_nh()
    return [
        scene("lane-ga-64-P*", 2048, 64, p, "near", kernel=lane(ga=True)),
        scene("lane-ga-40-P*", 2048, 40, S.lane_limit(40), "near", kernel=lane(full=False, ga=True, quads=False)),
        scene("lane-dep-64-P*", 2048, 64, p, "short", DEPLOYED, kernel=lane(dep=True)),
        scene("lane-dep-64-P*-lethal", 2048, 64, p, "lethal", DEPLOYED, kernel=lane(dep=True)),
        scene("lane-dep-56-P*", 2048, 56, S.lane_limit(56), "short", DEPLOYED, kernel=lane(56, dep=True)),
        scene("lane-dep-64-P*+1", 2048, 64, p + 1, "short", DEPLOYED, kind=0, kernel=wave_at(64, 3)),
        scene("lane-pow-64-P*", 61440, 64, p, "short", powers={"path_align": 2}, kernel=pow_row),
        scene("lane-nh-64-P*", 61440, 64, p, "short", model=DIFF, kernel=nh_row),
        scene("lane-rr-128-P*", 2048, 128, S.lane_limit(128, rr=True, window=S.WIN_WIDE), "long",
              kernel=lane(128)),
        scene("lane-rr-64-P*", 2048, 64, S.lane_limit(64, rr=True), "short", env=(("SMPC_LANE_REREAD", "1"),),
              kernel=lane(rr=True)),
    ]


def split_cases():
    two = (("SMPC_PASS", "split"), ("SMPC_SPLIT_NSEG", "2"))
    out = []
    for tag, B, T, nseg, env, kernel in (("4-full", 16384, 64, 4, (), "smpc_pass_split<4, true>"),
                                         ("4-masked", 20000, 60, 4, (), "smpc_pass_split<4, false>"),
                                         ("2-full", 4096, 64, 2, two, "smpc_pass_split<2, true>")):
        p = S.split_limit(T, nseg)
        out.append(scene(f"split-{tag}-P*-short", B, T, p, "short", flags=0, env=env, kind=2, kernel=kernel))
        out.append(scene(f"split-{tag}-P*-lethal", B, T, p, "lethal", flags=0, env=env, kind=2, kernel=kernel))
        out.append(scene(f"split-{tag}-P*+1-short", B, T, p + 1, "short", flags=0, env=env, kind=0, kernel=wave_at(T, 0)))
    return out


# the wave pass at SMPC_MAX_PATH points, the costmap scored: per horizon four PathAlign steps (the
# sample counts of the module docstring), each with every scoring mode
WAVE_STEPS = {100: (7, 6, 4, 3), 128: (8, 7, 4, 3), 200: (13, 12, 7, 6), 256: (17, 15, 8, 7)}
WAVE_MODES = {0: dict(names=FIVE), 2: dict(names=FIVE, powers={"path_follow": 2}), 3: dict(names=DEPLOYED),
              4: dict(names=DEPLOYED, footprint=("cost",))}


def wave_cases():
    out = []
    for T, steps in WAVE_STEPS.items():
        for step in steps:
            for mode in WAVE_MODES:
                P = S.plan_limit(S.KIND_WAVE, S.WIN_WIDE, T, (T - 1) // step)
                out.append(scene(f"wave-{T}-mode-{mode}-nsamp-{(T - 1) // step}", 500, T, P, "long", flags=0, step=step,
                                 kind=0, kernel=wave_at(T, mode), **WAVE_MODES[mode]))
    return out


BUILDERS = (lane_cases, row_cases, split_cases, wave_cases)
# (collected without the library: the ids are written out, the scenes are built inside the tests)
IDS = {
    lane_cases: [f"lane-{tag}-{rest}" for tag in ("five", "no-obst") for rest in (
        "64-P*-1-long", "64-P*-long", "64-P*+1-long", "64-P*-1-short", "64-P*-short", "64-P*+1-short", "64-P*-lethal",
        "64-P*-long-70000", "64-P*-short-70000", "64-P*+1-short-70000", "56-P*-short", "56-P*+1-short", "40-P*-short",
        "40-P*+1-short", "30-P*-short", "30-P*+1-short")],
    row_cases: ["lane-ga-64-P*", "lane-ga-40-P*", "lane-dep-64-P*", "lane-dep-64-P*-lethal", "lane-dep-56-P*",
                "lane-dep-64-P*+1", "lane-pow-64-P*", "lane-nh-64-P*", "lane-rr-128-P*", "lane-rr-64-P*"],
    split_cases: [f"split-{tag}-{rest}" for tag in ("4-full", "4-masked", "2-full")
                  for rest in ("P*-short", "P*-lethal", "P*+1-short")],
    wave_cases: [f"wave-{T}-mode-{mode}-nsamp-{(T - 1) // step}"
                 for T, steps in WAVE_STEPS.items() for step in steps for mode in WAVE_MODES],
}
ALL_IDS = [(b, name) for b in BUILDERS for name in IDS[b]]


def find(builder, name):
    scenes = builder()
    assert [s.name for s in scenes] == IDS[builder], "the written-out ids and the scenes differ"
    return next(s for s in scenes if s.name == name)


def judge(g, sc, u, out, label=None, kernel=None):
    ref = S.oracle_tick(sc)
    label = label or sc.name
    print(f"[plan length] {label}: {sc.B} x {sc.T}, P {sc.P} ({sc.plan}); pass_kind {out.pass_kind}, passes {out.passes}, "
          f"kernel {kernel or last_kernel(g)}; furthest {out.furthest_reached_path_point} (oracle "
          f"{ref.out.furthest_reached_path_point}), non-colliding {out.non_colliding} (oracle {ref.out.non_colliding})")
    assert out.non_colliding == ref.out.non_colliding, label
    assert_parity(u, out, ref.u, ref.out, g.get_costs(), ref.costs, max_flips=1, label=label)


@gpu
@pytest.mark.parametrize("builder,name", ALL_IDS, ids=[n for _, n in ALL_IDS])
def test_pass_at_its_longest_plan(Smpc, monkeypatch, builder, name):
    """One tick, and a second, speculated one on the same inputs (the first has no furthest-point
    prediction): both are the oracle's tick."""
    monkeypatch.delenv("SMPC_PASS", raising=False)
    sc = find(builder, name)
    if sc.plan in ("short", "lethal"):
        S.lands_at_the_end(sc)
    if builder is wave_cases:
        L = S.lds_layout(S.KIND_WAVE, S.WIN_WIDE, sc.P, sc.T, (sc.T - 1) // sc.step)
        print(f"[plan length] {name}: {(sc.T - 1) // sc.step} samples, segment of {1 << L['seg_shift']} lanes, "
              f"{L['group']} rollouts per flush, {L['total']} bytes of LDS")
    g, scn, tick = S.gpu_context(Smpc, monkeypatch, sc)
    for k in range(2):
        u, out = g.optimize(tick, scn.u0)
        assert (out.pass_kind, last_kernel(g)) == (sc.kind, sc.kernel), (name, k, out.pass_kind, last_kernel(g))
        judge(g, sc, u, out, f"{name} tick {k}")
    g.close()


def lane_group_scenes():
    return [scene("group-lane-P*", 2048, 64, S.lane_limit(64), "short", noise_seed=950),
            scene("group-lane-3", 2048, 64, 3, "long", noise_seed=951),
            scene("group-lane-60", 2048, 64, 60, "long", noise_seed=952)]


def wave_group_scenes():
    p = S.plan_limit(S.KIND_WAVE, S.WIN, 64, 15)
    return [scene("group-wave-P*", 500, 64, p, "short", flags=0, kind=0, noise_seed=960),
            scene("group-wave-2", 500, 64, 2, "long", flags=0, kind=0, noise_seed=961),
            scene("group-wave-56", 500, 64, 56, "long", flags=0, kind=0, noise_seed=962)]


def prune_scene(P):
    return scene(f"prune-edge-{P}", 70000, 64, P, "long", env=(("SMPC_LANE_TIMELINE", "1"),), kernel=LANE_ROW[64])


def twins_and_members(Smpc, scenes):
    """Per scene a context for the group and a lone twin (full-size blocks, as a group's lane members launch)."""
    members, twins = [], []
    for sc in scenes:
        members.append(S.gpu_context(Smpc, pytest.MonkeyPatch(), sc)[0])
        mp = pytest.MonkeyPatch()
        mp.setenv("SMPC_NO_HALF_BLOCKS", "1")
        try:
            twins.append(S.gpu_context(Smpc, mp, sc)[0])
        finally:
            mp.undo()
    return members, twins


def same_bits(member, twin, res_g, res_t, label):
    (ug, og), (ut, ot) = res_g, res_t
    assert np.array_equal(ug.view(np.uint32), ut.view(np.uint32)), label
    for f in ("min_cost", "sum_w", "furthest_valid", "furthest_reached_path_point", "non_colliding", "fail_flag", "pass_kind"):
        assert getattr(og, f) == getattr(ot, f), (label, f, getattr(og, f), getattr(ot, f))
    assert np.array_equal(member.get_costs().view(np.uint32), twin.get_costs().view(np.uint32)), label


def group_round(Smpc, monkeypatch, scenes, kind, kernel):
    from mpcholonavigation_amd.optimizer import SmpcGroup
    monkeypatch.delenv("SMPC_PASS", raising=False)
    for sc in scenes:
        if sc.plan == "short":
            S.lands_at_the_end(sc)
    members, twins = twins_and_members(Smpc, scenes)
    grp = SmpcGroup(members)
    ins = [S.inputs(sc) for sc in scenes]
    ticks, us = [t for _, t in ins], [scn.u0 for scn, _ in ins]
    batched = []
    for k in range(3):       # the same tick three times: alone (no prediction yet), then batched
        before = grp.stats().batched_launches
        res = grp.optimize(ticks, us)
        batched.append(grp.stats().batched_launches - before)
        seen = last_kernel(members[0])
        for i, sc in enumerate(scenes):
            rt = twins[i].optimize(ticks[i], us[i])
            same_bits(members[i], twins[i], res[i], rt, f"{sc.name} tick {k}")
            assert res[i][1].pass_kind == kind, (sc.name, k)
            judge(members[i], sc, *res[i], label=f"{sc.name} tick {k}", kernel=seen)
        if k == 2:
            assert batched[k] == 1 and seen == kernel and all(o.passes == 1 for _, o in res), (batched, seen)
    grp.close()
    for g in members + twins:
        g.close()


@gpu
def test_lane_group_of_unequal_plans(Smpc, monkeypatch):
    """smpc_group_optimize sizes ONE lane layout from the longest member's plan; the members' own P differ."""
    scenes = lane_group_scenes()
    group_round(Smpc, monkeypatch, scenes, 1, lane(many=True))


@gpu
def test_wave_group_of_unequal_plans(Smpc, monkeypatch):
    """smpc_pass_many carries one layout per member."""
    scenes = wave_group_scenes()
    group_round(Smpc, monkeypatch, scenes, 0, wave_at(64, 0, many=True))


@gpu
@pytest.mark.parametrize("P", [256, 257])
def test_prune_table_edge(Smpc, monkeypatch, P):
    """kPruneMaxPath = 256 (prepare_tick): at 256 points the furthest-point prune table is built and
    read from the second tick on, at 257 the tick gets the empty header and every group scans.  Three
    closed-loop ticks (the oracle's sequence, shifted, feeds both sides)."""
    monkeypatch.delenv("SMPC_PASS", raising=False)
    sc = prune_scene(P)
    g, scn, tick = S.gpu_context(Smpc, monkeypatch, sc)
    o = S._oracle(sc, scn)
    u = scn.u0
    for k in range(3):
        ug, og = g.optimize(tick, u)
        uo, oo = o.optimize(tick, u)
        scanned, groups = scan_count(g)
        print(f"[plan length] {sc.name} tick {k}: pass_kind {og.pass_kind}, passes {og.passes}, kernel {last_kernel(g)}, "
              f"furthest {og.furthest_reached_path_point} (oracle {oo.furthest_reached_path_point}), "
              f"{scanned} of {groups} groups scanned")
        assert (og.pass_kind, last_kernel(g)) == (1, sc.kernel), k
        assert oo.furthest_valid and og.furthest_reached_path_point == oo.furthest_reached_path_point, k
        assert og.non_colliding == oo.non_colliding, k
        assert_parity(ug, og, uo, oo, g.get_costs(), o.get_costs(), max_flips=1, label=f"{sc.name} tick {k}")
        assert groups == (sc.B + 63) // 64
        if k >= 1:
            assert og.passes == 1, (k, og.passes)       # (the same plan, pose and noise: the prediction holds)
            if P <= 256:
                assert scanned < groups, (k, scanned, groups)
            else:
                assert scanned == groups, (k, scanned, groups)
        u = np.concatenate([uo[:, 1:], uo[:, -1:]], axis=1)
    o.close()
    g.close()


def test_scenes_are_no_knife_edges():
    """Not a GPU test.  The strict oracle and the -ffast-math oracle agree on every scene above: on
    fail_flag, furthest_reached_path_point and non_colliding, and within assert_parity's bar."""
    scenes = ([sc for b in BUILDERS for sc in b()] + lane_group_scenes() + wave_group_scenes() +
              [prune_scene(256), prune_scene(257)])
    for sc in scenes:
        strict, fast = S.oracle_tick(sc), S.oracle_tick(sc, fast=True)
        for f in ("fail_flag", "furthest_valid", "furthest_reached_path_point", "non_colliding"):
            assert getattr(strict.out, f) == getattr(fast.out, f), (sc.name, f, getattr(strict.out, f), getattr(fast.out, f))
        assert_parity(fast.u, fast.out, strict.u, strict.out, fast.costs, strict.costs, max_flips=1, label=sc.name,
                      report=False)
        # ... and no lookup that assert_parity cannot see (a neighbouring cell's cost below its 2e-4)
        # accounts for more than a tenth of its tight bound: plan_scenes.hidden_flip_influence
        infl, bound = S.hidden_flip_influence(sc)
        assert np.all(infl <= 0.1 * bound), (sc.name, infl, bound)
        if sc.plan in ("short", "lethal"):
            S.lands_at_the_end(sc)
        if sc.plan == "lethal":
            _, tick = S.inputs(sc)
            assert np.hypot(tick.path_x[-11] - tick.pose_x, tick.path_y[-11] - tick.pose_y) > 0.5, sc.name
