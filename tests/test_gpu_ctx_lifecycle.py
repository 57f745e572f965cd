"""The context's life: everything it allocates late — the background noise set, the limiter's
buffers, the moving-obstacle table, the breakdown's buffers — goes with it and comes back the same,
and a context's per-tick block is its own before, inside and after a group.

The contexts own their device memory through holders (csrc/smpc_own.h) and a group lends its
members a slot of its arena for their tick block.  Nothing here can see an allocation; what it can
see is that a context created after another one was destroyed, with every late buffer in use,
computes the same bits, and that a member ticks like a context that was never grouped at every
stage of joining and leaving.

Shapes: the smallest the suite uses for the two noise layouts — a wave context 130 x 64 ([B, T]
noise, a half block at the end) and a SMPC_FLAG_LANE_PER_ROLLOUT context 192 x 64 (group-major
noise), as tests/test_gpu_group_critic_stats.py."""
import numpy as np
import pytest

from tests import moving_model as mm
from tests.footprint_scenes import same_bits
from tests.harness import FIVE, LANE, OUT_FIELDS, close, copy_of, critics_of, mod, moved, shifted  # noqa: F401
from tests.helpers import configure
from tests.stats_scenes import scene

pytestmark = pytest.mark.gpu

T = 64
SHAPES = [(130, 0), (192, LANE)]
LIMITS = (0.6, -0.8, 0.5, 1.2)
DISCS = dict(collision_cost=50.0, repulsion_weight=5.0, margin=0.5)
STRUCT_FIELDS = ("scored_mask", "fail_flag", "batch", "best_rollout", "best_cost", "effective_samples")
ROW_FIELDS = ("sum", "min", "max", "weighted", "at_best")


def case(B, flags):
    cfg, scn, _ = scene(B, T, "wall")
    return copy_of(cfg, flags=cfg.flags | flags), scn


def same_stats(a, b, label):
    for f in STRUCT_FIELDS:
        assert getattr(a, f) == getattr(b, f), (label, f, getattr(a, f), getattr(b, f))
    for f in ROW_FIELDS:
        assert np.array_equal(getattr(a, f), getattr(b, f)), (label, f)
    assert np.array_equal(a.per_rollout, b.per_rollout), label


# ---- 1. destroy and create, every late buffer in use -------------------------------------------------

def one_round(mod, cfg, scn, discs):
    g = mod.Smpc(cfg)
    configure(g, scn, critics=critics_of(FIVE))
    g.seed(11)
    g.set_acceleration_limits(*LIMITS)
    g.set_moving_obstacles(discs[0], discs[1], **DISCS)
    g.redraw_noise_async()
    u1, o1 = g.optimize(scn.tick, scn.u0)
    u2, o2 = g.optimize(moved(scn.tick, 0.015), shifted(u1))
    st = g.critic_stats(moved(scn.tick, 0.03), shifted(u2), per_rollout=True)
    limited = g.get_limited_noise()
    m, hit = g.moving_obstacle_costs()
    g.close()
    return dict(u=(u1, u2), out=[tuple(getattr(o, f) for f in OUT_FIELDS) for o in (o1, o2)], stats=st,
                limited=limited, m=m, hit=hit)


@pytest.mark.parametrize("B,flags", SHAPES, ids=["wave-130x64", "lane-192x64"])
def test_every_late_buffer_survives_destroy_and_create(mod, B, flags):
    """Three rounds of create .. close with the same seed; a round uses the background noise set, the
    limiter, two moving discs, the breakdown with its rows, the limited noise and m / hit.  Rounds 2
    and 3 are round 1 bit for bit."""
    cfg, scn = case(B, flags)
    discs = mm.make_discs(scn.tick, T, cfg.model_dt, 2, 5)
    first = one_round(mod, cfg, scn, discs)
    assert first["hit"].any() or first["m"].any(), "the discs scored nothing"
    assert not np.array_equal(first["u"][0], scn.u0)
    for k in (2, 3):
        r = one_round(mod, cfg, scn, discs)
        for i in range(2):
            assert np.array_equal(r["u"][i], first["u"][i]), f"round {k} tick {i}: u"
            assert r["out"][i] == first["out"][i], f"round {k} tick {i}: {dict(zip(OUT_FIELDS, r['out'][i]))}"
        same_stats(r["stats"], first["stats"], f"round {k}")
        for a, b in zip(r["limited"], first["limited"]):
            assert np.array_equal(a, b), f"round {k}: limited noise"
        assert np.array_equal(r["m"], first["m"]) and np.array_equal(r["hit"], first["hit"]), f"round {k}: m / hit"


# ---- 2. alone, grouped, alone, grouped again ------------------------------------------------------------

def test_a_member_ticks_alike_before_inside_and_after_a_group(mod):
    """The two contexts, each beside a lone twin with the same seed and inputs that is ticked with
    optimize throughout: one tick alone, a group (two rounds and a grouped breakdown), a tick alone,
    a second group of the same members (one round).  Every tick is the twin's bit for bit, the grouped
    statistics are the twin's own."""
    members, twins, ticks0, us = [], [], [], []
    for B, flags in SHAPES:
        cfg, scn = case(B, flags)
        for lst in (members, twins):
            g = mod.Smpc(cfg)
            configure(g, scn, critics=critics_of(FIVE))
            g.seed(7 + B)
            lst.append(g)
        ticks0.append(scn.tick)
        us.append(scn.u0)
    step = [0]

    def tick_all(grp, label):
        nonlocal us
        ticks = [moved(t, 0.015 * step[0]) for t in ticks0]
        res = grp.optimize(ticks, us) if grp else [m.optimize(t, u) for m, t, u in zip(members, ticks, us)]
        for i in range(2):
            same_bits(members[i], twins[i], res[i], twins[i].optimize(ticks[i], us[i]), f"{label}, member {i}")
        us = [shifted(u) for u, _ in res]
        step[0] += 1

    tick_all(None, "alone before")
    grp = mod.SmpcGroup(members)
    tick_all(grp, "first group, round 1")
    tick_all(grp, "first group, round 2")
    ticks = [moved(t, 0.015 * step[0]) for t in ticks0]
    res = grp.critic_stats(ticks, us, per_rollout=True)
    for i in range(2):
        same_stats(res[i], twins[i].critic_stats(ticks[i], us[i], per_rollout=True), f"grouped breakdown, member {i}")
    grp.close()
    tick_all(None, "alone between")
    grp = mod.SmpcGroup(members)
    tick_all(grp, "second group")
    grp.close()
    tick_all(None, "alone after")
    close(*members, *twins)
