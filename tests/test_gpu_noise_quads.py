"""The group-major noise in quads of steps (smpc_dev.h SMPC_GM_INDEX): element (b, t) of a tensor sits
at (((b / 64) (T4 / 4) + t / 4) 64 + b % 64) 4 + t % 4, T4 = T rounded up to a multiple of four, so that a
lane's four steps of a quad are one 16-byte load.  Writers (smpc_fill_noise_tm, smpc_relayout both
ways) and readers (the three lane kernels in their parking, re-read and ragged forms, smpc_pass_split)
must agree on it; every case here is a small batch with the lane pass forced.

  a. layout round trip: what a lane-pass context drew or was given comes back as [B, T];
  b. parity with the CPU oracle at 197 rollouts (three full groups and a tail of five lanes) for every
     form that reads the copy, at assert_parity's default bounds;
  c. the lane pass against the wave pass on the same stored noise, at the bounds test_gpu_lane_loop.py
     holds the pair to (assert_parity's defaults, costs included), and a redrawn epoch against a fresh
     context seeded to it, bit for bit.

The rows of smpc_pass_lane_pow and smpc_pass_lane_nh are reached from 61 440 rollouts up only
(smpc_prepare.cpp plan_launch): at 197 rollouts a cost_power = 2 tick and a DiffDrive tick take the
route the host gives them there, and the two rows proper are run once each at 61 440 x 40.
"""
import numpy as np
import pytest

from mpcholonavigation_amd import _abi as A
from mpcholonavigation_amd.synthetic import make_noise, make_scenario
from mpcholonavigation_amd.tick import default_config
from tests import harness as H
from tests import noise_model as nm
from tests.harness import DEPLOYED, FIVE, LANE, Oracle, Smpc, last_kernel, oracle_tick  # noqa: F401
from tests.helpers import assert_parity, configure, make_case
from tests.kernel_names import LANE_ROW, lane, lane_nh, lane_pow

pytestmark = pytest.mark.gpu

B_PARITY = 197
ROUND_TRIP = [(130, 64), (130, 56), (130, 40), (130, 30), (130, 128), (64, 4)]


KERNEL = LANE_ROW


def critics_of(names=FIVE, power=1):
    return H.critics_of(names, power, constraint_band=True)


def copy_cfg(cfg, flags=0, **fields):
    c2 = H.copy_of(cfg, **fields)
    c2.flags |= flags
    return c2


def gpu_tick(Smpc, cfg, scn, noise, critics=None):
    g = Smpc(cfg)
    configure(g, scn, critics=critics, noise=noise)
    u, out = g.optimize(scn.tick, scn.u0)
    costs, ran = g.get_costs().copy(), last_kernel(g)
    g.close()
    return u, out, costs, ran


def check(Smpc, Oracle, cfg, scn, noise, label, kernel=None, critics=None, wave=False, kind=1):
    """One tick of a forced lane-pass context against the oracle (and, on request, against a
    wave-per-rollout context) on the same stored noise."""
    ug, og, cg, ran = gpu_tick(Smpc, copy_cfg(cfg, LANE), scn, noise, critics)
    uo, oo, co = oracle_tick(Oracle, cfg, scn, noise, critics)
    print(f"[noise quads] {label}: kernel {ran}, pass_kind {og.pass_kind}, non_colliding {og.non_colliding} "
          f"(oracle {oo.non_colliding})")
    assert og.pass_kind == kind, (label, ran)
    if kernel is not None:
        assert ran == kernel, (label, ran)
    assert og.non_colliding == oo.non_colliding, label
    assert_parity(ug, og, uo, oo, cg, co, label=label)
    if wave:
        uw, ow, cw, ran_w = gpu_tick(Smpc, copy_cfg(cfg, A.SMPC_FLAG_WAVE_PER_ROLLOUT), scn, noise, critics)
        assert ow.pass_kind == 0, (label, ran_w)
        assert_parity(ug, og, uw, ow, cg, cw, label=label + " (against the wave pass)")


# ---- a. layout round trip ---------------------------------------------------------------------------

def _noise_cfg(B, T, flags=0):
    return default_config(batch_size=B, time_steps=T, flags=flags, global_batch_size=B, **nm.STDS)


@pytest.mark.parametrize("B,T", ROUND_TRIP)
def test_drawn_noise_comes_back_as_rows(Smpc, monkeypatch, B, T):
    """A device-RNG draw of a lane-pass context (straight into the quad layout where T is a multiple
    of four, else [B, T] and smpc_relayout), read back with smpc_get_noise: the model's stream
    (tests/noise_model.py, at its own bound for the device's Box-Muller), and bit for bit the draw of
    a context without the flag, whose fill writes [B, T] and touches no group-major copy."""
    monkeypatch.delenv("SMPC_NO_FUSED_FILL", raising=False)
    seed = nm.SEEDS[1]
    got = []
    for flags in (LANE, 0):
        cfg = _noise_cfg(B, T, flags)
        g = Smpc(cfg)
        g.seed(seed)
        noise = [n.copy() for n in g.get_noise()]
        nm.check_noise(noise, cfg, seed, 0, label=f"{B}x{T} flags {flags:#x}")
        g.close()
        got.append(noise)
    for a, b in zip(*got):
        assert a.shape == (B, T)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("B,T", ROUND_TRIP)
def test_given_noise_comes_back_after_a_tick(Smpc, B, T):
    """smpc_set_noise of tensors whose element (b, t) is the integer b T + t (exact in float), a tick
    of the forced lane pass, smpc_get_noise: the same integers."""
    cfg = default_config(batch_size=B, time_steps=T, flags=LANE)
    scn = make_scenario(T)
    v = (np.arange(B, dtype=np.float32)[:, None] * T + np.arange(T, dtype=np.float32)[None, :]).astype(np.float32)
    g = Smpc(cfg)
    configure(g, scn, noise=(v, v.copy(), v.copy()))
    _, out = g.optimize(scn.tick, scn.u0)
    assert out.pass_kind == 1, last_kernel(g)
    for n in g.get_noise():
        assert np.array_equal(n, v)
    g.close()


# ---- b. parity with the oracle ----------------------------------------------------------------------

@pytest.mark.parametrize("T", [64, 56, 40, 30])
def test_parking_form_against_oracle_and_wave_pass(Smpc, Oracle, T):
    cfg, scn, noise = make_case(B_PARITY, T)
    check(Smpc, Oracle, cfg, scn, noise, f"{B_PARITY}x{T}", kernel=KERNEL[T], wave=True)


def test_reread_form_against_oracle(Smpc, Oracle):
    cfg, scn, noise = make_case(B_PARITY, 128)
    check(Smpc, Oracle, cfg, scn, noise, f"{B_PARITY}x128 re-read", kernel=KERNEL[128])


def test_near_goal_tick_against_oracle(Smpc, Oracle):
    """GoalAngle live: the T = 64 row that issues the next quad's loads in front of the quad's last step."""
    cfg, scn, noise = make_case(B_PARITY, 64, near_goal=True)
    check(Smpc, Oracle, cfg, scn, noise, "near goal", kernel=lane(ga=True))


def test_deployed_list_against_oracle(Smpc, Oracle):
    cfg, scn, noise = make_case(B_PARITY, 56)
    check(Smpc, Oracle, cfg, scn, noise, "deployed list, T = 56", kernel=lane(56, dep=True),
          critics=critics_of(DEPLOYED))


def test_cost_power_2_against_oracle(Smpc, Oracle):
    """197 rollouts: below the power rows' batch rule, the general wave pass scores the tick."""
    cfg, scn, noise = make_case(B_PARITY, 64)
    check(Smpc, Oracle, cfg, scn, noise, "cost_power 2", critics=critics_of(FIVE, power=2), kind=0)


def test_diff_drive_against_oracle(Smpc, Oracle):
    """197 rollouts: below the _nh rows' batch rule, the Omni-form row with a zero vy tensor."""
    cfg, scn, noise = make_case(B_PARITY, 64)
    cfg = copy_cfg(cfg, motion_model=A.SMPC_MODEL_DIFF_DRIVE)
    check(Smpc, Oracle, cfg, scn, noise, "DiffDrive", kernel=KERNEL[64])


@pytest.mark.parametrize("what", ["cost-power-2", "diff-drive"])
def test_power_and_no_vy_rows_at_their_smallest_batch(Smpc, Oracle, what):
    """61 440 x 40: smpc_pass_lane_pow and smpc_pass_lane_nh proper, the whole-quads rows."""
    cfg, scn, noise = make_case(61440, 40)
    if what == "cost-power-2":
        check(Smpc, Oracle, cfg, scn, noise, what, critics=critics_of(FIVE, power=2),
              kernel=lane_pow(full=False))
    else:
        check(Smpc, Oracle, copy_cfg(cfg, motion_model=A.SMPC_MODEL_DIFF_DRIVE), scn, noise, what,
              kernel=lane_nh(full=False))


def test_group_of_two_against_oracle(Smpc, Oracle):
    """Two contexts in one launch (the grouped rows), two ticks each against its own oracle."""
    from mpcholonavigation_amd.optimizer import SmpcGroup
    T = 64
    cases = []
    for i in range(2):
        cfg = default_config(batch_size=B_PARITY, time_steps=T, flags=LANE)
        cases.append((cfg, make_scenario(T, seed=60 + i, path_points=40 + 5 * i), make_noise(B_PARITY, T, seed=900 + i)))
    members, oracles = [], []
    for cfg, scn, noise in cases:
        g, o = Smpc(cfg), Oracle(cfg)
        for obj in (g, o):
            configure(obj, scn, noise=noise)
        members.append(g)
        oracles.append(o)
    grp = SmpcGroup(members)
    us = [scn.u0 for _, scn, _ in cases]
    for k in range(2):
        res = grp.optimize([scn.tick for _, scn, _ in cases], us)
        for i, (o, (ug, og)) in enumerate(zip(oracles, res)):
            uo, oo = o.optimize(cases[i][1].tick, us[i])
            assert og.pass_kind == 1
            assert og.non_colliding == oo.non_colliding
            assert_parity(ug, og, uo, oo, members[i].get_costs(), o.get_costs(), label=f"group member {i} tick {k}")
            us[i] = np.concatenate([uo[:, 1:], uo[:, -1:]], axis=1)
    grp.close()
    for obj in members + oracles:
        obj.close()


def test_split_pass_at_its_smallest_batch_against_oracle(Smpc, Oracle):
    """12 288 x 64, default flags: the smallest batch the host gives smpc_pass_split (kSplitMinBatch)."""
    cfg, scn, noise = make_case(12288, 64)
    ug, og, cg, ran = gpu_tick(Smpc, cfg, scn, noise)
    uo, oo, co = oracle_tick(Oracle, cfg, scn, noise)
    assert og.pass_kind == 2, ran
    assert og.non_colliding == oo.non_colliding
    assert_parity(ug, og, uo, oo, cg, co, label="split 12288x64")


# ---- c. a redrawn epoch -----------------------------------------------------------------------------

@pytest.mark.parametrize("T", [64, 40])
def test_redrawn_epoch_equals_a_fresh_context_at_that_epoch(Smpc, monkeypatch, T):
    """A tick, smpc_redraw_noise, a second tick — against a fresh context brought to epoch 1 the same
    way before its only tick, on the second tick's inputs: noise, control sequence and costs bit for bit."""
    monkeypatch.delenv("SMPC_NO_FUSED_FILL", raising=False)
    cfg = default_config(batch_size=B_PARITY, time_steps=T, flags=LANE)
    scn = make_scenario(T)
    seed = nm.SEEDS[0]
    a = Smpc(cfg)
    configure(a, scn)
    a.seed(seed)
    u1, _ = a.optimize(scn.tick, scn.u0)
    a.redraw_noise()
    u2, o2 = a.optimize(scn.tick, u1)
    b = Smpc(cfg)
    configure(b, scn)
    b.seed(seed)
    b.redraw_noise()
    ub, ob = b.optimize(scn.tick, u1)
    assert o2.pass_kind == ob.pass_kind == 1
    for x, y in zip(a.get_noise(), b.get_noise()):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    assert np.array_equal(u2.view(np.uint32), ub.view(np.uint32))
    assert np.array_equal(a.get_costs().view(np.uint32), b.get_costs().view(np.uint32))
    assert o2.non_colliding == ob.non_colliding and o2.min_cost == ob.min_cost
    a.close()
    b.close()
