"""The footprint outline walk on the GPU, held to an exact model: every route, zero flips.

smpc_footprint_walk.inc and its two call sites in smpc_wave_pass.inc (the general pass's block and
the lean form of MODE 4) restate nav2's footprintCostAtPose, lineCost and LineIterator and add
rules of their own: when the walk is entered, which half of the footprint table a cost goes
through, what collides, outline cells from the LDS window or from global memory.  The parity tests
score an inflated wall with a flip allowance, under which a line walk that is off by one cell
passes.  On the scenes of tests/footprint_walk_scenes.py every pose is known bit for bit
(tests/test_footprint_walk_cpu.py pins that, and that the scenes tell every distinguishable
mutant of the model from the model), the costmaps are flat fields with isolated cells, and so

  * fail_flag and non_colliding equal the judge's (tests/footprint_walk_model.py),
  * EVERY rollout collides or not as the judge says, read off its cost,
  * EVERY non-colliding rollout's cost is within tol of the judge's, a colliding one's within tol
    and two float ulps of its collision cost: no flip allowance, nothing skipped,
  * tol = 0.25 * single_pose_shift, a quarter of the least that reclassifying one pose's footprint
    cost moves a rollout's cost (ten times clear of the oracle's own distance from the judge:
    asserted in the CPU file),

on three routes: the lean pass smpc_pass<R, 4, FULL>, the general pass (SMPC_FOOTPRINT_PASS=general)
and the breakdown's rows (smpc_pass_stats).  With num = 0 in place of num = delta / 2 in the
device's walk this file fails on every route: DESIGN.md section 7 has the counts."""
import numpy as np
import pytest

from mpcholonavigation_amd import _abi as A
from tests import edge_scenes as E
from tests import footprint_walk_model as M
from tests import footprint_walk_scenes as S
from tests.harness import Smpc, create_with_env, last_kernel  # noqa: F401
from tests.kernel_names import wave_at

pytestmark = pytest.mark.gpu

ROW = {"cost": "CostCritic", "obstacles": "ObstaclesCritic"}
GENERAL = {"SMPC_FOOTPRINT_PASS": "general"}
SINGLE = [(n, c) for n in S.SCENES for c in ("obstacles", "cost")]

_judge = {}


def judge(name, critic):
    """(the judge's result, tol, the collision cost) of one critic alone on a scene; computed once."""
    if (name, critic) not in _judge:
        scn = S.scene(name)
        cr = S.critics_of((critic,), (critic,))
        _judge[(name, critic)] = (M.model(scn, cr, critic), 0.25 * M.single_pose_shift(scn, cr, critic),
                                  E._weights(cr, critic, scn.T)[2])
    return _judge[(name, critic)]


def hold(label, costs, m, tol, collision):
    """One row of per-rollout costs against the judge's."""
    c = costs.astype(np.float64)
    d = np.abs(c - m["costs"])
    collided = c > 0.5 * collision
    wrong = int(np.sum(collided != m["collided"]))
    ok = np.where(m["collided"], d <= tol + 2.0 ** -22 * m["costs"], d <= tol)
    bad = int(np.sum(~ok & (collided == m["collided"])))
    print(f"[walk] {label}: rollouts colliding otherwise {wrong}, beyond tol {bad} of {c.size}; "
          f"max |cost - judge| over the others {d[~m['collided']].max(initial=0.0):.3e} (tol {tol:.3e})")
    assert wrong == 0, f"{label}: {wrong} rollouts collide where the judge's do not, or the reverse"
    assert bad == 0, f"{label}: {bad} rollouts beyond tol (worst {d[ok == 0].max():.3e})"


def hold_out(label, out, j):
    assert (out.fail_flag, out.non_colliding) == (j["fail_flag"], j["non_colliding"]), \
        (label, out.fail_flag, out.non_colliding, j["fail_flag"], j["non_colliding"])


@pytest.mark.parametrize("name,critic", SINGLE, ids=[f"{n}/{c}" for n, c in SINGLE])
def test_three_routes_against_the_judge(Smpc, monkeypatch, name, critic):
    scn = S.scene(name)
    m, tol, collision = judge(name, critic)
    cr = S.critics_of((critic,), (critic,))
    for route, env, mode in (("lean", {}, 4), ("general", GENERAL, 2)):
        g = create_with_env(Smpc, monkeypatch, scn.config(), env)
        try:
            scn.configure(g, cr)
            _, out = g.optimize(scn.tick, scn.u0)
            label = f"{name} {critic} {route}"
            assert (out.pass_kind, last_kernel(g)) == (0, wave_at(scn.T, mode)), label
            hold_out(label, out, m)
            hold(label, g.get_costs(), m, tol, collision)
            if route == "lean":
                st = g.critic_stats(scn.tick, scn.u0, per_rollout=True)
                label = f"{name} {critic} breakdown"
                assert st.scored(ROW[critic]) and bool(st.fail_flag) == bool(m["fail_flag"]), label
                hold(label, st.per_rollout[st.names.index(ROW[critic])], m, tol, collision)
        finally:
            g.close()


@pytest.mark.parametrize("name", list(S.SCENES))
def test_stored_trajectories_are_the_designed_poses(Smpc, monkeypatch, name):
    """The premise, pinned on the device: with the trajectory write-out (the general pass) x, y
    and yaw of every point equal the designed ones bit for bit; and the tick is judged again."""
    scn = S.scene(name)
    m, tol, collision = judge(name, "obstacles")
    g = create_with_env(Smpc, monkeypatch, scn.config(flags=A.SMPC_FLAG_STORE_TRAJECTORIES), GENERAL)
    try:
        scn.configure(g, S.critics_of(("obstacles",), ("obstacles",)))
        _, out = g.optimize(scn.tick, scn.u0)
        assert (out.pass_kind, last_kernel(g)) == (0, wave_at(scn.T, 2))
        x, y, yaw = g.get_generated_trajectories()
        assert np.array_equal(x, scn.x) and np.array_equal(y, scn.y), name
        assert np.array_equal(yaw, scn.yaw), name
        hold_out(name, out, m)
        hold(f"{name} obstacles stored", g.get_costs(), m, tol, collision)
    finally:
        g.close()


@pytest.mark.parametrize("fp", [("cost", "obstacles"), ("cost",), ("obstacles",)], ids=["both", "cost", "obstacles"])
@pytest.mark.parametrize("name", [n for n in S.SCENES if S.SCENES[n][0] in "abcde"])
def test_both_collision_critics_each_with_its_own_first_collision(Smpc, name, fp):
    """CostCritic and ObstaclesCritic in one list, consider_footprint on either: the general pass
    only.  Each critic keeps its own first collision and its own entry rule; the tick's cost is
    the sum of the two terms, each of which the judge restates.  (The breakdown refuses this
    configuration, so the two terms are held through their sum: it is within the smaller of the two
    critics' tolerances of the judge's sum, and a collision of either critic, worth hundreds or
    more, cannot hide in it.)"""
    scn = S.scene(name)
    cr = S.critics_of(("cost", "obstacles"), fp)
    j = M.both(scn, cr)
    tol = min(0.25 * M.single_pose_shift(scn, cr, c) for c in ("cost", "obstacles"))
    g = Smpc(scn.config())
    try:
        scn.configure(g, cr)
        _, out = g.optimize(scn.tick, scn.u0)
        label = f"{name} both, footprint on {fp}"
        assert (out.pass_kind, last_kernel(g)) == (0, wave_at(scn.T, 2)), label
        hold_out(label, out, j)
        d = np.abs(g.get_costs().astype(np.float64) - j["costs"])
        # (with the switch on one critic only the other scores in point mode: centre-cost sums in
        # the hundreds, whose float32 summation error is allowed for on top of tol)
        slack = 2.0 ** -21 * j["costs"] if len(fp) == 2 else S.float_sum_error(scn.T, j["costs"])
        free = ~(j["cost"]["collided"] | j["obstacles"]["collided"])
        print(f"[walk] {label}: max |cost - judge| over rollouts that do not collide {d[free].max(initial=0.0):.3e}, "
              f"rollouts beyond tol {int(np.sum(d > tol + slack))} of {d.size} (tol {tol:.3e})")
        assert np.all(d <= tol + slack), label
    finally:
        g.close()
