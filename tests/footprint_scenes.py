"""Shared inputs of the consider_footprint tests: the inflated wall beside the path, the
rectangular footprint, the two critic lists, and one oracle result per case.

The scene is the one of test_gpu_parity.py::test_consider_footprint_parity (a wall 0.35 m beside
the path, inscribed radius 0.1 m, inflation 0.55 m, scaling 10), rebuilt with NumPy only
(mpcholonavigation_amd.synthetic.wall_beside_path).  On it the CPU oracle counts these
non-colliding rollouts with the footprint off -> on, the same for CostCritic in the deployed list
and for ObstaclesCritic among the five:

    256 x 56: 249 -> 186    192 x 64: 184 -> 149    128 x 100: 111 -> 84    64 x 200: 53 -> 38

so the footprint decides tens of rollouts and neither none nor all collide."""
import functools
from types import SimpleNamespace

import numpy as np

from mpcholonavigation_amd.synthetic import wall_beside_path
from mpcholonavigation_amd.tick import default_critics
from tests.helpers import configure, make_case

FOOTPRINT = np.array([[0.25, 0.18], [0.25, -0.18], [-0.25, -0.18], [-0.25, 0.18]])   # 0.5 x 0.36 m
CIRCUMSCRIBED = float(np.hypot(0.25, 0.18))
LAYER_SCALING = 10.0

FIVE = ("obstacles", "path_align", "path_follow", "goal_angle", "prefer_forward")
DEPLOYED = ("constraint", "cost", "goal", "goal_angle", "path_align", "path_follow", "path_angle",
            "prefer_forward", "twirling")      # robot_bringup/config/nav2_params.yaml:222
LISTS = {"deployed": (DEPLOYED, "cost"), "five": (FIVE, "obstacles")}

# (B, T): every instance R x FULL of the wave pass, more than one block, ragged and full horizons
SHAPES = [(256, 56), (192, 64), (128, 100), (128, 128), (64, 200), (64, 256)]


def critics_of(names, footprint=(), power=1):
    """The named critics enabled (parameters as test_gpu_parity.py::_extra_critics sets them),
    consider_footprint on for the collision critics in `footprint`."""
    cr = default_critics()
    for n in ("obstacles", "path_align", "path_follow", "goal_angle", "prefer_forward", "cost", "goal",
              "constraint", "twirling", "path_angle", "velocity_deadband", "path_align_legacy"):
        sub = getattr(cr, n)
        sub.enabled = 1 if n in names else 0
        sub.cost_power = power
    for k in range(3):
        cr.velocity_deadband.deadband_velocities[k] = 0.08
    cr.constraint.vx_max, cr.constraint.vy_max, cr.constraint.vx_min = 0.35, 0.2, -0.1
    for n in footprint:
        getattr(cr, n).consider_footprint = 1
    return cr


def list_critics(which, footprint=True):
    names, collision = LISTS[which]
    return critics_of(names, (collision,) if footprint else ())


def wall_case(B, T, near_goal=False, closed_in=False):
    """make_case on the wall scene.  closed_in: walls on both sides 0.15 m from the centre line and
    reaching back past the robot, so that the outline (half width 0.18 m) lies on them from the
    first pose on while a centre that keeps to the path never does."""
    cfg, scn, noise = make_case(B, T, near_goal=near_goal)
    if closed_in:
        scn.cells = wall_beside_path(scn, offset=0.15, x_from=-0.5, x_to=1.5, both_sides=True)
    else:
        scn.cells = wall_beside_path(scn)
    return cfg, scn, noise


def setup(obj, scn, critics, noise, footprint=True):
    configure(obj, scn, critics=critics, noise=noise)
    if footprint:
        obj.set_footprint(FOOTPRINT, circumscribed_radius=CIRCUMSCRIBED, layer_cost_scaling_factor=LAYER_SCALING)
    return obj


def keep(u, out, costs):
    """A tick's result detached from the object that produced it."""
    return SimpleNamespace(u=u.copy(), costs=costs.copy(), out=SimpleNamespace(
        fail_flag=int(out.fail_flag), non_colliding=int(out.non_colliding),
        furthest_valid=int(out.furthest_valid),
        furthest_reached_path_point=int(out.furthest_reached_path_point)))


@functools.lru_cache(maxsize=None)
def oracle_tick(which, B, T, footprint=True, near_goal=False):
    """The oracle's first tick of a case, computed once per session and shared (read only)."""
    from oracle.loader import Oracle, build
    build()
    cfg, scn, noise = wall_case(B, T, near_goal=near_goal)
    o = setup(Oracle(cfg), scn, list_critics(which, footprint), noise, footprint)
    u, out = o.optimize(scn.tick, scn.u0)
    return keep(u, out, o.get_costs())
