"""The time loop of the lane-per-rollout pass (smpc_lane_pass.inc), pinned shape by shape.

The loop walks the horizon in quads of four steps, two quads per iteration, the odd quad behind its
loop, steps [0, 32) and [32, 64) parked in two register tuples; PathAlign samples the trajectory at the
first step of every quad but the very first, guesses the closest path point from the mean spacing and
falls back to a binary search; the costmap lookup is a pipeline two steps deep that is primed per
group; a group whose yaw leaves the fast sin/cos reduction's range is redone by the checked body.
Every case forces the lane pass on a small batch, asserts which instance ran and compares control
sequence, tick output and per-rollout costs with the CPU oracle at assert_parity's default bounds
(no flip allowance: the default synthetic scene needs none at these sizes); where cheap, also with a
wave-per-rollout context on the same inputs.
"""
import numpy as np
import pytest

from mpcholonavigation_amd import _abi as A
from mpcholonavigation_amd.tick import Tick
from tests.harness import FIVE, Oracle, Smpc, copy_of, critics_of, last_kernel, oracle_tick  # noqa: F401
from tests.helpers import assert_parity, configure, make_case
from tests.kernel_names import lane

pytestmark = pytest.mark.gpu

FULL64 = lane()
QUADS = lane(full=False)
TC56 = lane(56)
RAGGED = lane(full=False, quads=False)
NO_PATH_ALIGN = tuple(n for n in FIVE if n != "path_align")


def five(path_align=True, pa_offset=None):
    """The five critics of the lane pass at their defaults; PathAlign off or with another
    offset_from_furthest on request."""
    over = {} if pa_offset is None else {"path_align__offset_from_furthest": pa_offset}
    return critics_of(FIVE if path_align else NO_PATH_ALIGN, power=None, **over)


def with_plan(tick, path_x):
    """The tick with another (straight) plan along its own line; the goal is the plan's last point."""
    px = np.asarray(path_x, np.float32)
    py = np.full(px.size, tick.path_y[0], np.float32)
    return Tick(tick.pose_x, tick.pose_y, tick.pose_yaw, tick.speed, px, py, np.zeros(px.size, np.float32),
                float(px[-1]), float(py[-1]))


def lane_tick(Smpc, cfg, scn, noise, critics=None, tick=None, wave=False):
    """One tick on a context of its own: the forced lane pass, or the wave-per-rollout pass."""
    c2 = copy_of(cfg)
    c2.flags |= A.SMPC_FLAG_WAVE_PER_ROLLOUT if wave else A.SMPC_FLAG_LANE_PER_ROLLOUT
    g = Smpc(c2)
    configure(g, scn, critics=critics, noise=noise)
    u, out = g.optimize(tick or scn.tick, scn.u0)
    costs, kernel = g.get_costs().copy(), last_kernel(g)
    g.close()
    return u, out, costs, kernel


def check(Smpc, Oracle, cfg, scn, noise, kernel, label, critics=None, tick=None, wave=True, max_flips=0):
    """Lane pass against the oracle (and the wave pass) on the same inputs; returns the lane pass's
    and the oracle's per-rollout costs."""
    ug, og, cg, ran = lane_tick(Smpc, cfg, scn, noise, critics, tick)
    uo, oo, co = oracle_tick(Oracle, cfg, scn, noise, critics, tick)
    print(f"[lane loop] {label}: kernel {ran}, pass_kind {og.pass_kind}, non_colliding {og.non_colliding} "
          f"(oracle {oo.non_colliding}), furthest {og.furthest_reached_path_point}")
    assert og.pass_kind == 1 and ran == kernel, (label, ran)
    assert og.non_colliding == oo.non_colliding, label
    assert_parity(ug, og, uo, oo, cg, co, max_flips=max_flips, label=label)
    if wave:
        uw, ow, cw, ran_w = lane_tick(Smpc, cfg, scn, noise, critics, tick, wave=True)
        assert ow.pass_kind == 0, (label, ran_w)
        assert_parity(ug, og, uw, ow, cg, cw, max_flips=max_flips, label=label + " (against the wave pass)")
    return cg, co


# ---- the two-quads loop and its remainders ----------------------------------------------------------

HORIZONS = [(4, QUADS),     # the quad of step 0 only: no sample at all
            (8, QUADS),     # ... plus one
            (12, QUADS),    # the odd quad behind the loop
            (36, QUADS),    # crosses into the second register tuple with an odd count
            (56, TC56),     # the compile-time instance
            (64, FULL64),   # the full horizon
            (6, RAGGED)]    # the ragged instance


@pytest.mark.parametrize("T,kernel", HORIZONS, ids=[str(h[0]) for h in HORIZONS])
def test_horizons(Smpc, Oracle, T, kernel):
    cfg, scn, noise = make_case(192, T)
    check(Smpc, Oracle, cfg, scn, noise, kernel, f"192x{T}")


# ---- PathAlign live, disabled, gated off by the host ------------------------------------------------

def test_path_align_live_disabled_and_gated(Smpc, Oracle):
    """T = 64, B = 192.  Live: the default scene (the costs differ from those without the critic).
    Gated: a 15-point plan — the furthest reached point stays below offset_from_furthest (20), the host
    switches the critic off for the tick and the costs are those of the context without it, bit for bit."""
    cfg, scn, noise = make_case(192, 64)
    c_live, _ = check(Smpc, Oracle, cfg, scn, noise, FULL64, "PathAlign live")
    c_off, _ = check(Smpc, Oracle, cfg, scn, noise, FULL64, "PathAlign disabled", critics=five(path_align=False))
    assert np.max(np.abs(c_live - c_off)) > 1e-3, "PathAlign does not score on the default scene"
    short = with_plan(scn.tick, scn.tick.path_x[:15])
    c_gated, _ = check(Smpc, Oracle, cfg, scn, noise, FULL64, "PathAlign gated", tick=short)
    _, _, c_gated_off, _ = lane_tick(Smpc, cfg, scn, noise, five(path_align=False), short)
    assert np.array_equal(c_gated, c_gated_off)


# ---- the sample's exceptions ------------------------------------------------------------------------

def test_plan_whose_spacing_changes(Smpc, Oracle):
    """0.05 m for 30 points, then 0.5 m: the guess from the mean spacing is unconfirmed in most lanes
    and the binary search runs."""
    cfg, scn, noise = make_case(192, 64)
    x0 = float(scn.tick.path_x[0])
    px = np.concatenate([x0 + 0.05 * np.arange(30), x0 + 0.05 * 29 + 0.5 * np.arange(1, 7)])
    tick = with_plan(scn.tick, px)
    c, _ = check(Smpc, Oracle, cfg, scn, noise, FULL64, "spacing 0.05 then 0.5", tick=tick)
    _, _, c_off, _ = lane_tick(Smpc, cfg, scn, noise, five(path_align=False), tick)
    assert np.max(np.abs(c - c_off)) > 1e-3, "PathAlign is not live on this plan"


def test_short_plan_clamps_the_guess(Smpc, Oracle):
    """Fourteen points 0.05 m apart (the goal stays beyond the goal critics' 0.5 m) and PathAlign live
    from the third (offset_from_furthest 2): the first samples guess index 0 (the sentinel below), and
    the rollouts, which cover about 1.1 m, overshoot the plan and clamp at its last segment (the
    sentinel above)."""
    cfg, scn, noise = make_case(192, 64)
    tick = with_plan(scn.tick, scn.tick.path_x[:14])
    cr = five(pa_offset=2)
    c, _ = check(Smpc, Oracle, cfg, scn, noise, FULL64, "fourteen-point plan", critics=cr, tick=tick)
    off = five(path_align=False)
    _, _, c_off, _ = lane_tick(Smpc, cfg, scn, noise, off, tick)
    assert np.max(np.abs(c - c_off)) > 1e-3, "PathAlign is not live on this plan"


# ---- shadow lanes ------------------------------------------------------------------------------------

def test_ragged_last_group(Smpc, Oracle):
    cfg, scn, noise = make_case(100, 64)
    check(Smpc, Oracle, cfg, scn, noise, FULL64, "100x64")


# ---- a wave that runs two groups ---------------------------------------------------------------------

def test_wave_with_two_groups(Smpc, Oracle):
    """One group more than the grid has waves (one block of eight waves per CU): wave 0 of block 0
    runs a second group, whose sample state and lookup pipeline must start afresh.  The last group's
    costs against the oracle's, one by one."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    B = 64 * (8 * cus + 1)
    cfg, scn, noise = make_case(B, 64)
    cg, co = check(Smpc, Oracle, cfg, scn, noise, FULL64, f"{B}x64 ({cus} CUs)", wave=False)
    d = np.abs(cg[-64:].astype(np.float64) - co[-64:].astype(np.float64))
    assert np.all(d <= 2e-4 * np.maximum(np.abs(co[-64:]), 1.0)), d.max()


# ---- the redo path -----------------------------------------------------------------------------------

@pytest.mark.parametrize("path_align", [True, False], ids=["path-align", "no-path-align"])
def test_group_redone_by_the_checked_body(Smpc, Oracle, path_align):
    """A few absurd wz samples: |yaw| leaves the fast reduction's range (65 536) in all three groups,
    early, in the middle and in the last steps; each group is redone by the checked body.

    That the redo ran shows in the three rollouts themselves: the fast sin/cos reduces by a multiple of
    pi held in 22 bits of a float and is only specified below 65 536 rad (test_device_sincos_accuracy),
    so a yaw of 1.5e6 or -1.25e7 rad carried through steps 4..63 or 11..63 by the fast body puts the
    rest of the rollout somewhere else; their costs are held to the oracle's one by one, at the bound
    assert_parity calls tight, on top of the batch-wide check (which would let one of them go: at
    this size its default max_soft is 1 — the comparison with the wave pass uses it on the parent
    too, one rollout 2.4e-4 apart, where lane and wave pass round a sum differently)."""
    cfg, scn, noise = make_case(192, 64)
    nvx, nvy, nwz = [n.copy() for n in noise]
    absurd = {5: (3, 3.0e7), 70: (10, -2.5e8), 150: (62, 9.0e6)}
    for b, (t, v) in absurd.items():
        nwz[b, t] = v
    cg, co = check(Smpc, Oracle, cfg, scn, (nvx, nvy, nwz), FULL64, f"huge yaw, PathAlign {path_align}",
                   critics=five(path_align=path_align))
    for b in absurd:
        d = abs(float(cg[b]) - float(co[b]))
        print(f"[lane loop] rollout {b}: cost {cg[b]!r}, oracle {co[b]!r}")
        assert d <= 2e-4 * max(abs(float(co[b])), 1.0), (b, cg[b], co[b])
