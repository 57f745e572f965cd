"""What the test modules share, each piece once: the critic lists and their one builder, the
fixtures that hand out the library's classes, the set / create / delete pattern for the knobs a
context reads from the environment, and the readers of the developer entry points
(include/smpc_debug.h).  The parity bar stays in tests/helpers.py, the expected kernel names in
tests/kernel_names.py, scenes in the *_scenes.py modules.

Not a conftest: a test module imports the fixtures it uses by name (`# noqa: F401`)."""
import ctypes as C

import numpy as np
import pytest

from mpcholonavigation_amd import _abi as A
from mpcholonavigation_amd.tick import Tick, default_critics
from tests.helpers import configure

# ---- names -----------------------------------------------------------------------------------------

# the sub-structs of smpc_critic_params, in declaration order
ALL_CRITICS = ("obstacles", "path_align", "path_follow", "goal_angle", "prefer_forward", "cost", "goal",
               "constraint", "twirling", "path_angle", "velocity_deadband", "path_align_legacy")
FIVE = ALL_CRITICS[:5]               # the north star's list
NO_OBST = FIVE[1:]
DEPLOYED = ("constraint", "cost", "goal", "goal_angle", "path_align", "path_follow", "path_angle",
            "prefer_forward", "twirling")      # robot_bringup/config/nav2_params.yaml:222
LANE = A.SMPC_FLAG_LANE_PER_ROLLOUT
# a tick's result block without its two timings
OUT_FIELDS = tuple(n for n, _ in A.SmpcTickOut._fields_ if n not in ("device_ms", "score_pass_ms"))


# ---- the critic builder -------------------------------------------------------------------------------

def critics_of(names, power=1, footprint=(), *, constraint_band=False, deadband=False, **over):
    """default_critics() with exactly `names` enabled.

    power: every critic's cost_power — an int, a {name: power} dict (1 where it says nothing), or
      None to leave the defaults alone.
    footprint: the collision critics that get consider_footprint.
    constraint_band: ConstraintCritic's vx_max / vy_max / vx_min = 0.35 / 0.2 / -0.1, inside what
      the sampled controls reach, so that the critic has something to score.
    deadband: VelocityDeadband's three velocities = 0.08, likewise.
    over: single fields, spelled sub__field=value (path_align__trajectory_point_step=3)."""
    cr = default_critics()
    for n in ALL_CRITICS:
        sub = getattr(cr, n)
        sub.enabled = 1 if n in names else 0
        if power is not None:
            sub.cost_power = power.get(n, 1) if isinstance(power, dict) else power
    if deadband:
        for k in range(3):
            cr.velocity_deadband.deadband_velocities[k] = 0.08
    if constraint_band:
        cr.constraint.vx_max, cr.constraint.vy_max, cr.constraint.vx_min = 0.35, 0.2, -0.1
    for n in footprint:
        getattr(cr, n).consider_footprint = 1
    for path, v in over.items():
        sub, field = path.split("__")
        setattr(getattr(cr, sub), field, v)
    return cr


def dressed_critics(names, power=1, footprint=(), **over):
    """critics_of with both dressings on: the parameters under which all twelve critics score."""
    return critics_of(names, power, footprint, constraint_band=True, deadband=True, **over)


# ---- fixtures -----------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def Smpc():
    from mpcholonavigation_amd.optimizer import Smpc as S
    return S


@pytest.fixture(scope="module")
def Oracle():
    from oracle.loader import Oracle as O, build
    build()
    return O


@pytest.fixture(scope="module")
def mod():
    from mpcholonavigation_amd import optimizer
    return optimizer


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from mpcholonavigation_amd.optimizer import load_library
    return load_library()


def create_with_env(Smpc, monkeypatch, cfg, env):
    """Smpc(cfg) with the knobs of `env` (a dict or a sequence of pairs) in the environment: they
    are read when the context is created, and gone again when this returns."""
    env = dict(env or ())
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    g = Smpc(cfg)
    for k in env:
        monkeypatch.delenv(k)
    return g


# ---- the developer entry points (bound by optimizer.load_library) ---------------------------------------

def _library():
    from mpcholonavigation_amd.optimizer import load_library
    return load_library()


def last_kernel(g):
    """The scoring-pass instance launched last, as rocprofv3's kernel trace spells it."""
    return g.last_pass_kernel()


def furthest_f(g):
    """The float F = index + fraction the last tick's pass reported (tuple slot 2)."""
    f = C.c_float(0)
    if g.lib.smpc_debug_furthest_f(g.h, C.byref(f)) != 0:      # no critic of the tick consumed the furthest point
        return float("nan")
    return f.value


def scan_count(g):
    """(groups of the lane pass that took the furthest-point scan since the last call, groups of
    one launch) of a context created under SMPC_LANE_TIMELINE=1."""
    n, groups = C.c_ulonglong(0), C.c_uint32(0)
    assert g.lib.smpc_debug_lane_scan_count(g.h, C.byref(n), C.byref(groups)) == 0
    return n.value, groups.value


def bar_tick(g):
    return g.lib.smpc_debug_bar_tick(g.h)


def debug_lds_layout(kind, window_bytes, P, T, arg):
    """The 16 words of the LDS layout a scoring pass is launched with (smpc_debug_lds_layout)."""
    out = np.zeros(16, np.uint32)
    assert _library().smpc_debug_lds_layout(kind, window_bytes, P, T, arg, out.ctypes.data) == 0
    return out


def debug_prune_table(px, py, k0, on, floats):
    """The prune table a tick would write for this plan and first index (smpc_debug_prune_table)."""
    px = np.ascontiguousarray(px, np.float32)
    py = np.ascontiguousarray(py, np.float32)
    out = np.zeros(floats, np.float32)
    assert _library().smpc_debug_prune_table(px.ctypes.data, py.ctypes.data, len(px), k0, on, out.ctypes.data) == 0
    return out


# ---- small helpers ------------------------------------------------------------------------------------

def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def shifted(u):
    """shiftControlSequence: every column one step earlier, the last one kept."""
    return np.concatenate([u[:, 1:], u[:, -1:]], axis=1)


def moved(t, dx):
    return Tick(t.pose_x + dx, t.pose_y, t.pose_yaw, t.speed, t.path_x, t.path_y, t.path_yaw, t.goal_x, t.goal_y)


def close(*objs):
    for o in objs:
        o.close()


def copy_of(cfg, **kw):
    c2 = type(cfg)()
    C.memmove(C.byref(c2), C.byref(cfg), C.sizeof(cfg))
    for k, v in kw.items():
        setattr(c2, k, v)
    return c2


def oracle_tick(Oracle, cfg, scn, noise, critics=None, tick=None, u0=None):
    """One tick of a fresh oracle on the scene: (u, out, per-rollout costs)."""
    o = Oracle(cfg)
    configure(o, scn, critics=critics, noise=noise)
    uo, oo = o.optimize(tick or scn.tick, scn.u0 if u0 is None else u0)
    co = o.get_costs().copy()
    o.close()
    return uo, oo, co
