"""The lane pass's furthest-point prune test (smpc_lane_furthest.inc, build_prune_table): a group
none of whose live rollouts can raise the maximum skips the nearest-point scan.  The result must
not move by a bit: SMPC_FURTHEST_PRUNE=0 makes the host write the empty table ("never prune"), the
same kernel then scans every group, and that context is the unpruned answer from the same binary.

Batch: plan_launch gives the parking form one block of eight waves per CU, 256 x 8 = 2048 waves on
the full grid, and every wave takes groups gw, gw + 2048, ...: every wave runs three groups from
3 x 2048 x 64 = 393 216 rollouts.  A wave's first group has no bound of its own yet: wave 0 of a
block scans it, the other seven leave its endpoints in LDS and judge them behind their second
group against wave 0's maximum; second and third groups have the wave's own bound."""
import numpy as np
import pytest

from mpcholonavigation_amd.synthetic import make_noise, make_scenario
from mpcholonavigation_amd.tick import Tick, default_config
from tests.harness import DEPLOYED, LANE, Oracle, Smpc, critics_of, furthest_f, scan_count, shifted  # noqa: F401
from tests.helpers import assert_parity, configure, make_case

pytestmark = pytest.mark.gpu

B3 = 393216


def pair(Smpc, monkeypatch, B, T, scn, critics=None, flags=LANE, seed=77, timeline=False):
    """Two contexts on the same stored noise: knob on (the product) and knob off."""
    ctxs = []
    for knob in ("1", "0"):
        monkeypatch.setenv("SMPC_FURTHEST_PRUNE", knob)
        if timeline:
            monkeypatch.setenv("SMPC_LANE_TIMELINE", "1")
        g = Smpc(default_config(batch_size=B, time_steps=T, flags=flags))
        configure(g, scn, critics=critics)
        g.seed(seed)
        ctxs.append(g)
    monkeypatch.delenv("SMPC_FURTHEST_PRUNE")
    monkeypatch.delenv("SMPC_LANE_TIMELINE", raising=False)
    return ctxs


def same_ticks(on, off, ticks, u0, label, kind=1):
    """Every tick of the sequence on both contexts: control sequence, costs, non-colliding count,
    the float F and the number of scoring passes are equal bit for bit."""
    u = u0
    seen = []
    for k, tk in enumerate(ticks):
        ua, oa = on.optimize(tk, u)
        ub, ob = off.optimize(tk, u)
        assert oa.pass_kind == ob.pass_kind and (kind is None or oa.pass_kind == kind), (label, k)
        assert np.array_equal(ua.view(np.uint32), ub.view(np.uint32)), (label, k)
        assert np.array_equal(on.get_costs().view(np.uint32), off.get_costs().view(np.uint32)), (label, k)
        assert oa.non_colliding == ob.non_colliding, (label, k)
        assert oa.furthest_reached_path_point == ob.furthest_reached_path_point, (label, k)
        fa, fb = furthest_f(on), furthest_f(off)
        assert np.float32(fa).view(np.uint32) == np.float32(fb).view(np.uint32) or (fa != fa and fb != fb), (label, k, fa, fb)
        assert oa.passes == ob.passes, (label, k, oa.passes, ob.passes)
        assert oa.fail_flag == ob.fail_flag
        seen.append((int(oa.furthest_reached_path_point), round(fa, 3), int(oa.passes)))
        u = shifted(ua)
    print(f"[furthest prune] {label}: (furthest point, F, passes) per tick: {seen}")
    return seen


def plans(scn):
    """The U-turn and the coarse plan of test_windowed_furthest_scan_falls_back_exactly."""
    t = scn.tick
    P = len(t.path_x)
    res = float(t.path_x[1] - t.path_x[0])
    k = np.arange(P)
    ux = (t.path_x[0] + res * np.minimum(k, 33) - res * np.maximum(k - 33, 0)).astype(np.float32)
    uy = (t.path_y[0] + np.where(k > 33, 0.05, 0.0)).astype(np.float32)
    uturn = Tick(t.pose_x, t.pose_y, t.pose_yaw, t.speed, ux, uy, np.zeros(P, np.float32), float(ux[-1]), float(uy[-1]))
    cx = (t.path_x[0] + 3.0 * res * k).astype(np.float32)
    coarse = Tick(t.pose_x, t.pose_y, t.pose_yaw, t.speed, cx, t.path_y.copy(), np.zeros(P, np.float32), float(cx[-1]),
                  float(t.path_y[-1]))
    return uturn, coarse


def moving(scn, n):
    """The pose advances 0.02 m per tick along the plan, which is pruned to the robot."""
    t = scn.tick
    res = float(t.path_x[1] - t.path_x[0])
    out = []
    for k in range(n):
        adv = 0.02 * k
        cut = int(adv / res)
        out.append(Tick(t.pose_x + adv, t.pose_y, t.pose_yaw, t.speed, t.path_x[cut:].copy(), t.path_y[cut:].copy(),
                        np.zeros(len(t.path_x) - cut, np.float32), float(t.path_x[-1]), float(t.path_y[-1])))
    return out


def short(scn, P):
    """A plan that ends where the rollouts' endpoints are: the furthest point is its last point."""
    t = scn.tick
    return Tick(t.pose_x, t.pose_y, t.pose_yaw, t.speed, t.path_x[:P].copy(), t.path_y[:P].copy(), np.zeros(P, np.float32),
                float(t.path_x[P - 1]), float(t.path_y[P - 1]))


@pytest.mark.parametrize("T", [64, 56])
def test_knob_on_and_off_are_bit_identical(Smpc, monkeypatch, T):
    scn = make_scenario(T)
    on, off = pair(Smpc, monkeypatch, B3, T, scn)
    t = scn.tick
    uturn, coarse = plans(scn)
    same_ticks(on, off, [t] * 4, scn.u0, f"frozen T={T}")
    same_ticks(on, off, moving(scn, 12), scn.u0, f"moving T={T}")
    same_ticks(on, off, [t, t, uturn, uturn, t, coarse, coarse, t], scn.u0, f"u-turn and coarse T={T}")
    same_ticks(on, off, [short(scn, 22)] * 3 + [short(scn, 12)] * 3, scn.u0, f"plan's last point T={T}", kind=None)
    on.close()
    off.close()


def test_parity_with_the_oracle(Smpc, Oracle):
    """As test_windowed_furthest_scan_falls_back_exactly: the plans on which the window and the
    prune table are most likely to be wrong, against the oracle, tick after tick."""
    B, T = 4096, 64
    cfg, scn, noise = make_case(B, T)
    cfg.flags |= LANE
    g, o = Smpc(cfg), Oracle(cfg)
    for obj in (g, o):
        configure(obj, scn, noise=noise)
    t = scn.tick
    uturn, coarse = plans(scn)
    u = scn.u0
    for label, tk in (("straight", t), ("straight", t), ("u-turn", uturn), ("u-turn", uturn), ("straight", t),
                      ("coarse", coarse), ("coarse", coarse), ("straight", t), ("end", short(scn, 22)),
                      ("end", short(scn, 22))):
        ug, og = g.optimize(tk, u)
        uo, oo = o.optimize(tk, u)
        assert og.pass_kind == 1
        assert og.furthest_reached_path_point == oo.furthest_reached_path_point, label
        assert_parity(ug, og, uo, oo, g.get_costs(), o.get_costs(), max_flips=1, label=f"prune {label}", report=False)
        u = shifted(uo)
    g.close()


def test_share_of_groups_that_scan(Smpc, monkeypatch):
    """On the straight plan fewer than a quarter of the groups take the scan; with the knob off
    every group does (the developer timeline buffer carries the count)."""
    T = 64
    scn = make_scenario(T)
    on, off = pair(Smpc, monkeypatch, B3, T, scn, timeline=True)
    n = 4
    counts = []
    for g in (on, off):
        u = scn.u0
        for _ in range(3):                  # the first tick has no prediction: it does not speculate
            un, out = g.optimize(scn.tick, u)
            u = shifted(un)
        scan_count(g)                       # (clears)
        passes = 0
        for _ in range(n):
            un, out = g.optimize(scn.tick, u)
            u = shifted(un)
            passes += out.passes
        got, groups = scan_count(g)
        assert groups == B3 // 64 and passes == n
        counts.append(got)
    print(f"[furthest prune] groups that scanned over {n} ticks of {B3 // 64} groups: on {counts[0]}, off {counts[1]}")
    assert counts[1] == n * (B3 // 64)
    assert counts[0] < 0.25 * n * (B3 // 64)
    on.close()
    off.close()


def test_goal_angle_instance_is_untouched(Smpc, monkeypatch):
    T = 64
    scn = make_scenario(T, near_goal=True)
    on, off = pair(Smpc, monkeypatch, 8192, T, scn)
    same_ticks(on, off, [scn.tick] * 4, scn.u0, "GoalAngle instance")


def test_deployed_list_instance_is_untouched(Smpc, monkeypatch):
    T = 56
    scn = make_scenario(T)
    on, off = pair(Smpc, monkeypatch, 70000, T, scn, critics=critics_of(DEPLOYED, power=None))
    same_ticks(on, off, [scn.tick] * 4, scn.u0, "deployed-list instance")


def test_reread_instance_is_untouched(Smpc, monkeypatch):
    T = 128
    scn = make_scenario(T)
    on, off = pair(Smpc, monkeypatch, 8192, T, scn)
    same_ticks(on, off, [scn.tick] * 4, scn.u0, "T = 128 instance")


def test_grouped_instances_are_untouched(Smpc, monkeypatch):
    from mpcholonavigation_amd.optimizer import SmpcGroup
    B, T, n = 8192, 64, 2
    scns = [make_scenario(T, seed=70 + i) for i in range(n)]
    results = []
    for knob in ("1", "0"):
        monkeypatch.setenv("SMPC_FURTHEST_PRUNE", knob)
        members = []
        for i in range(n):
            g = Smpc(default_config(batch_size=B, time_steps=T, flags=LANE))
            configure(g, scns[i])
            g.seed(500 + i)
            members.append(g)
        grp = SmpcGroup(members)
        us = [s.u0 for s in scns]
        seen = []
        for _ in range(4):
            res = grp.optimize([s.tick for s in scns], us)
            us = [shifted(u) for u, _ in res]
            seen.append([(u.copy(), int(o.furthest_reached_path_point), int(o.non_colliding), int(o.passes)) for u, o in res] +
                        [m.get_costs() for m in members])
        results.append(seen)
        grp.close()
        for m in members:
            m.close()
    monkeypatch.delenv("SMPC_FURTHEST_PRUNE")
    for ta, tb in zip(*results):
        for a, b in zip(ta, tb):
            if isinstance(a, tuple):
                assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and a[1:] == b[1:]
            else:
                assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
