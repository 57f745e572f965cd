"""Python face of the C++ host optimizer (libsortham_host.so, include/smpc_host.h):
sortham::Optimizer of the reference with the [batch, time] work on the GPU.

Method names follow the reference (src/optimizer.cpp): eval_control = evalControl,
set_speed_limit = setSpeedLimit, reset = reset, get_optimized_trajectory =
getOptimizedTrajectory.  Where the reference throws std::runtime_error this
raises RuntimeError with the same message."""
import ctypes as C
import os

import numpy as np

from . import _abi as A

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libsortham_host.so")
SORTHAM_ERR_THROWN = -10
SORTHAM_FLEET_NOT_TAKEN = 1
_lib = None
_fleet_bound = False


class SorthamOptimizerConfig(C.Structure):
    _fields_ = [
        ("base", A.SmpcConfig),
        ("controller_frequency", C.c_double),
        ("retry_attempt_limit", C.c_uint32),
        ("regenerate_noises", C.c_int32),
        ("visualize", C.c_int32),
        ("noise_seed", C.c_uint64),
        ("critics", C.c_char_p * 16),
        ("n_critics", C.c_uint32),
        ("cost_scaling_factor", C.c_float),
        ("inflation_radius", C.c_float),
        ("motion_model", C.c_char_p),
    ]


_ctx = C.c_void_p
PROTOTYPES = {
    "sortham_optimizer_create": (C.c_int, [C.POINTER(SorthamOptimizerConfig),
                                           C.POINTER(A.SmpcCriticParams), C.POINTER(_ctx)]),
    "sortham_optimizer_initialize": (C.c_int, [_ctx, C.POINTER(SorthamOptimizerConfig),
                                               C.POINTER(A.SmpcCriticParams)]),
    "sortham_optimizer_destroy": (None, [_ctx]),
    "sortham_optimizer_last_error": (C.c_char_p, [_ctx]),
    "sortham_optimizer_set_costmap": (C.c_int, [_ctx, C.c_void_p, C.c_uint32, C.c_uint32,
                                                C.c_double, C.c_double, C.c_double, C.c_int,
                                                C.c_float, C.c_int]),
    "sortham_optimizer_set_footprint": (C.c_int, [_ctx, C.c_void_p, C.c_uint32, C.c_double, C.c_double]),
    "sortham_optimizer_set_noise": (C.c_int, [_ctx, C.c_void_p, C.c_void_p, C.c_void_p]),
    "sortham_optimizer_eval_control": (C.c_int, [_ctx, C.POINTER(A.SmpcTickIn), C.c_void_p,
                                                 C.POINTER(A.SmpcTickOut)]),
    "sortham_optimizer_critic_stats": (C.c_int, [_ctx, C.POINTER(A.SmpcTickIn),
                                                 C.POINTER(A.SmpcCriticStats), C.c_void_p]),
    "sortham_optimizer_last_tick": (C.c_int, [_ctx, C.POINTER(A.SmpcTickOut)]),
    "sortham_optimizer_set_speed_limit": (C.c_int, [_ctx, C.c_double, C.c_int]),
    "sortham_optimizer_set_acceleration_limits": (C.c_int, [_ctx, C.c_float, C.c_float, C.c_float, C.c_float]),
    "sortham_optimizer_set_moving_obstacles": (C.c_int, [_ctx, C.POINTER(A.SmpcMovingObstaclesParams), C.c_void_p,
                                                         C.c_void_p, C.c_uint32, C.c_uint32]),
    "sortham_optimizer_moving_obstacle_costs": (C.c_int, [_ctx, C.c_void_p, C.c_void_p, C.c_uint32]),
    "sortham_optimizer_set_trajectory_validation": (C.c_int, [_ctx, C.POINTER(A.SmpcValidationParams)]),
    "sortham_optimizer_last_validation": (C.c_int, [_ctx, C.POINTER(A.SmpcValidation), C.POINTER(C.c_uint64),
                                                    C.POINTER(C.c_uint64)]),
    "sortham_optimizer_reset": (C.c_int, [_ctx]),
    "sortham_optimizer_get_control_sequence": (C.c_int, [_ctx, C.c_void_p]),
    "sortham_optimizer_set_control_sequence": (C.c_int, [_ctx, C.c_void_p]),
    "sortham_optimizer_get_constraints": (C.c_int, [_ctx, C.c_void_p, C.POINTER(C.c_int32)]),
    "sortham_optimizer_get_optimized_trajectory": (C.c_int, [_ctx, C.c_void_p]),
    "sortham_utils_savitsky_golay": (None, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_int]),
    "sortham_run_ticks": (C.c_int, [_ctx, C.POINTER(A.SmpcTickIn), C.c_void_p, C.c_uint32, C.c_uint32,
                                    C.c_uint32, C.POINTER(A.SmpcTickOut), C.POINTER(C.c_uint32)]),
}

# the fleet's entry points: bound when the first FleetOptimizer is made
FLEET_PROTOTYPES = {
    "sortham_fleet_create": (C.c_int, [C.POINTER(_ctx), C.c_uint32, C.POINTER(_ctx)]),
    "sortham_fleet_destroy": (None, [_ctx]),
    "sortham_fleet_last_error": (C.c_char_p, [_ctx]),
    "sortham_fleet_eval_control": (C.c_int, [_ctx, C.POINTER(A.SmpcTickIn), C.c_void_p, C.c_void_p,
                                             C.POINTER(A.SmpcTickOut), C.c_void_p]),
    "sortham_fleet_stats": (C.c_int, [_ctx, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                                      C.POINTER(C.c_uint64)]),
    "sortham_fleet_run_rounds": (C.c_int, [_ctx, C.POINTER(A.SmpcTickIn), C.c_void_p, C.c_uint32, C.c_int,
                                           C.c_void_p, C.POINTER(A.SmpcTickOut), C.c_void_p,
                                           C.POINTER(C.c_uint32)]),
}

# the fleet's critic statistics (FleetOptimizer::getCriticStats): bound with the fleet's entry points
FLEET_STATS_PROTOTYPES = {
    "sortham_fleet_critic_stats": (C.c_int, [_ctx, C.POINTER(A.SmpcTickIn), C.c_void_p,
                                             C.POINTER(A.SmpcCriticStats), C.POINTER(C.c_void_p), C.c_void_p]),
}

# mutual avoidance (FleetOptimizer::setMutualAvoidance) and its table function: bound with them
FLEET_AVOIDANCE_PROTOTYPES = {
    "sortham_fleet_set_mutual_avoidance": (C.c_int, [_ctx, C.POINTER(A.SmpcMovingObstaclesParams), C.c_void_p,
                                                     C.c_uint32]),
    "sortham_fleet_moving_launches": (C.c_int, [_ctx, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "sortham_fleet_validation_counts": (C.c_int, [_ctx, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "sortham_fleet_avoidance_table": (C.c_int, [C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                                C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                C.POINTER(C.c_uint32)]),
}
FLEET_PEER_UNSEEN, FLEET_PEER_STANDING, FLEET_PEER_MOVING = 0, 1, 2

TICKS_SHIFT, TICKS_REDRAW_ASYNC, TICKS_SHARD, TICKS_SHARD_SPECULATE = 1, 2, 4, 8

DEFAULT_CRITICS = ["ObstaclesCritic", "PathAlignCritic", "PathFollowCritic", "GoalAngleCritic",
                   "PreferForwardCritic"]


def load_library():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"{LIB_PATH} not found: run `make -C mpcholonavigation_amd/csrc`")
        _lib = A.bind(C.CDLL(LIB_PATH), PROTOTYPES)
    return _lib


def load_fleet_library():
    global _fleet_bound
    lib = load_library()
    if not _fleet_bound:
        A.bind(lib, FLEET_PROTOTYPES)
        A.bind(lib, FLEET_STATS_PROTOTYPES)
        A.bind(lib, FLEET_AVOIDANCE_PROTOTYPES)
        _fleet_bound = True
    return lib


def moving_params(collision_cost=None, repulsion_weight=None, margin=None):
    """smpc_moving_obstacles_params: the library's defaults with the given fields replaced."""
    from .optimizer import load_library as load_smpc
    p = A.SmpcMovingObstaclesParams()
    load_smpc().smpc_moving_obstacles_params_default(C.byref(p))
    for name, v in (("collision_cost", collision_cost), ("repulsion_weight", repulsion_weight), ("margin", margin)):
        if v is not None:
            setattr(p, name, v)
    return p


def mutual_avoidance_table(i, state, pose, u, model_dt, holonomic, robot_radius):
    """sortham_fleet_avoidance_table: the moving-obstacle table FleetOptimizer gives member i.
    state [n] (FLEET_PEER_*), pose [n, 3], u [n, 3, T], model_dt [n], holonomic [n], robot_radius [n]
    -> (xy [discs, T, 2], radius [discs])."""
    lib = load_fleet_library()
    u = np.ascontiguousarray(u, np.float32)
    n, _, T = u.shape
    state = np.ascontiguousarray(state, np.uint8)
    pose = np.ascontiguousarray(pose, np.float64)
    model_dt = np.ascontiguousarray(model_dt, np.float32)
    holonomic = np.ascontiguousarray(holonomic, np.uint8)
    robot_radius = np.ascontiguousarray(robot_radius, np.float32)
    xy = np.zeros((max(n - 1, 1), T, 2), np.float32)
    radius = np.zeros(max(n - 1, 1), np.float32)
    discs = C.c_uint32(0)
    rc = lib.sortham_fleet_avoidance_table(i, n, T, _ptr(state), _ptr(pose), _ptr(u), _ptr(model_dt), _ptr(holonomic),
                                           _ptr(robot_radius), _ptr(xy), _ptr(radius), C.byref(discs))
    if rc != 0:
        raise ValueError(f"sortham_fleet_avoidance_table: error {rc}")
    return xy[:discs.value], radius[:discs.value]


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def run_ticks(smpc, tick, u, n, flags=TICKS_SHIFT):
    """sortham_run_ticks: n closed-loop ticks of the low-level context `smpc` (optimizer.Smpc) issued
    by the compiled loop of host/tick_loop.cpp -> (u after the last tick [and shift], [SmpcTickOut] * n).
    Raises SmpcError with the ticks completed in the message."""
    lib = load_library()
    u = np.array(u, dtype=np.float32, order="C")
    if u.shape != (3, smpc.T):
        raise ValueError(f"u must be [3, {smpc.T}]")
    outs = (A.SmpcTickOut * n)()
    done = C.c_uint32(0)
    rc = lib.sortham_run_ticks(smpc.h, C.byref(tick.c), _ptr(u), smpc.T, n, flags, outs, C.byref(done))
    if rc != 0:
        from .optimizer import SmpcError
        raise SmpcError(rc, f"after {done.value} of {n} ticks: " + (smpc.lib.smpc_last_error(smpc.h) or b"").decode())
    return u, outs


class Optimizer:
    def __init__(self, cfg: A.SmpcConfig, critic_params: A.SmpcCriticParams,
                 controller_frequency, critics=None, motion_model="Omni", retry_attempt_limit=1,
                 regenerate_noises=False, visualize=False, noise_seed=0,
                 cost_scaling_factor=10.0, inflation_radius=0.55):
        self.lib = load_library()
        c = self._config(cfg, controller_frequency, critics, motion_model, retry_attempt_limit,
                         regenerate_noises, visualize, noise_seed, cost_scaling_factor, inflation_radius)
        h = _ctx()
        rc = self.lib.sortham_optimizer_create(C.byref(c), C.byref(critic_params), C.byref(h))
        if rc != 0:
            raise RuntimeError(self.lib.sortham_optimizer_last_error(None).decode() or f"error {rc}")
        self.h = h

    def initialize(self, cfg: A.SmpcConfig, critic_params: A.SmpcCriticParams, controller_frequency,
                   critics=None, motion_model="Omni", retry_attempt_limit=1, regenerate_noises=False,
                   visualize=False, noise_seed=0, cost_scaling_factor=10.0, inflation_radius=0.55):
        """Optimizer::initialize() again on the live object (the plugin's reset()): an unchanged
        configuration keeps the device context, anything else rebuilds it."""
        c = self._config(cfg, controller_frequency, critics, motion_model, retry_attempt_limit,
                         regenerate_noises, visualize, noise_seed, cost_scaling_factor, inflation_radius)
        self._ck(self.lib.sortham_optimizer_initialize(self.h, C.byref(c), C.byref(critic_params)))

    def _config(self, cfg, controller_frequency, critics, motion_model, retry_attempt_limit,
                regenerate_noises, visualize, noise_seed, cost_scaling_factor, inflation_radius):
        self.T, self.B = cfg.time_steps, cfg.batch_size
        c = SorthamOptimizerConfig()
        c.base = cfg
        c.controller_frequency = controller_frequency
        c.retry_attempt_limit = retry_attempt_limit
        c.regenerate_noises = int(regenerate_noises)
        c.visualize = int(visualize)
        c.noise_seed = noise_seed
        names = DEFAULT_CRITICS if critics is None else critics
        for i, n in enumerate(names):
            c.critics[i] = n.encode()
        c.n_critics = len(names)
        c.cost_scaling_factor, c.inflation_radius = cost_scaling_factor, inflation_radius
        c.motion_model = motion_model.encode()
        self._keep = c       # (the name strings stay alive with the struct)
        return c

    def close(self):
        if getattr(self, "h", None):
            self.lib.sortham_optimizer_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc):
        if rc != 0:
            raise RuntimeError(self.lib.sortham_optimizer_last_error(self.h).decode())

    def set_costmap(self, cells, origin_x, origin_y, resolution, track_unknown=False,
                    inscribed_radius=0.1, has_inflation_layer=True):
        cells = np.ascontiguousarray(cells, dtype=np.uint8)
        h, w = cells.shape
        self._ck(self.lib.sortham_optimizer_set_costmap(
            self.h, _ptr(cells), w, h, origin_x, origin_y, resolution, int(track_unknown),
            inscribed_radius, int(has_inflation_layer)))

    def set_footprint(self, xy, circumscribed_radius, layer_cost_scaling_factor=10.0):
        """The robot footprint for consider_footprint = true: [n, 2] points in the robot frame, the
        layered costmap's circumscribed radius, the inflation layer's cost_scaling_factor (< 0: no
        inflation layer).  Applies from the next tick on and survives initialize()."""
        xy = np.ascontiguousarray(xy, dtype=np.float64)
        if xy.ndim != 2 or xy.shape[1] != 2:
            raise ValueError("xy must be [n, 2]")
        if not 1 <= xy.shape[0] <= A.SMPC_MAX_FOOTPRINT:
            raise ValueError(f"a footprint has 1 to {A.SMPC_MAX_FOOTPRINT} points")
        self._ck(self.lib.sortham_optimizer_set_footprint(
            self.h, _ptr(xy), xy.shape[0], float(circumscribed_radius), float(layer_cost_scaling_factor)))

    def set_noise(self, nvx, nvy, nwz):
        a = [np.ascontiguousarray(x, dtype=np.float32) for x in (nvx, nvy, nwz)]
        self._ck(self.lib.sortham_optimizer_set_noise(self.h, _ptr(a[0]), _ptr(a[1]), _ptr(a[2])))

    def eval_control(self, tick):
        """-> (twist [vx, vy, wz] float64, SmpcTickOut); raises where the reference throws."""
        tw = np.zeros(3, np.float64)
        out = A.SmpcTickOut()
        self._ck(self.lib.sortham_optimizer_eval_control(self.h, C.byref(tick.c), _ptr(tw),
                                                         C.byref(out)))
        return tw, out

    def critic_stats(self, tick, per_rollout=False):
        """Optimizer::getCriticStats: the per-critic breakdown (optimizer.CriticStats) of the tick
        eval_control(tick) would run next; eval_control afterwards is unaffected."""
        from .optimizer import critic_names, critic_stats_from_c, load_library as load_smpc
        st = A.SmpcCriticStats()
        rows = None
        if per_rollout:
            rows = np.empty((A.SMPC_STATS_ROWS, self.B), np.float32)
        self._ck(self.lib.sortham_optimizer_critic_stats(self.h, C.byref(tick.c), C.byref(st),
                                                         _ptr(rows) if rows is not None else None))
        return critic_stats_from_c(st, critic_names(load_smpc()), rows)

    def last_tick(self):
        """The SmpcTickOut of the last tick the object ran (the last retry's when eval_control raised)."""
        out = A.SmpcTickOut()
        self._ck(self.lib.sortham_optimizer_last_tick(self.h, C.byref(out)))
        return out

    def set_acceleration_limits(self, ax_max, ax_min, ay_max, az_max):
        """Bounds on how fast a sampled control may change (all zero: off); kept across reset()."""
        self._ck(self.lib.sortham_optimizer_set_acceleration_limits(self.h, ax_max, ax_min, ay_max, az_max))

    def set_moving_obstacles(self, xy=None, radius=None, collision_cost=None, repulsion_weight=None, margin=None):
        """Optimizer::setMovingObstacles: xy [n, T, 2], radius [n] (optimizer.Smpc.set_moving_obstacles);
        xy None or empty: clearMovingObstacles.  Kept across reset() and a re-initialize."""
        p = moving_params(collision_cost, repulsion_weight, margin)
        if xy is None or len(xy) == 0:
            self._ck(self.lib.sortham_optimizer_set_moving_obstacles(self.h, C.byref(p), None, None, 0, self.T))
            return
        xy = np.ascontiguousarray(xy, dtype=np.float32)
        radius = np.ascontiguousarray(radius, dtype=np.float32).reshape(-1)
        if xy.ndim != 3 or xy.shape[1:] != (self.T, 2) or radius.shape[0] != xy.shape[0]:
            raise ValueError("xy must be [n, time_steps, 2] and radius [n]")
        self._ck(self.lib.sortham_optimizer_set_moving_obstacles(self.h, C.byref(p), _ptr(xy), _ptr(radius),
                                                                 xy.shape[0], self.T))

    def moving_obstacle_costs(self):
        """(m [B] float32, hit [B] bool) of the last tick's last iteration."""
        m = np.empty(self.B, np.float32)
        hit = np.empty(self.B, np.uint8)
        self._ck(self.lib.sortham_optimizer_moving_obstacle_costs(self.h, _ptr(m), _ptr(hit), self.B))
        return m, hit.astype(bool)

    def set_trajectory_validation(self, on=True, collision_lookahead_time=None, consider_footprint=None,
                                  moving_obstacles=None):
        """Optimizer::setTrajectoryValidation (on false: clearTrajectoryValidation): eval_control then
        validates the trajectory of every optimize()'s result (optimizer.Smpc.validate_trajectory) and
        a colliding one is reset and retried like a tick whose rollouts all collide.  Arguments left
        None keep the library's defaults.  Kept across reset() and a re-initialize."""
        if not on:
            self._ck(self.lib.sortham_optimizer_set_trajectory_validation(self.h, None))
            return
        from .optimizer import load_library as load_smpc, validation_params
        p = validation_params(load_smpc(), collision_lookahead_time, consider_footprint, moving_obstacles)
        self._ck(self.lib.sortham_optimizer_set_trajectory_validation(self.h, C.byref(p)))

    def last_validation(self):
        """The verdict of the last validation (optimizer.Validation) with `run` and `invalid`: how many
        validations the object has run and how many of them found a collision."""
        from .optimizer import validation_from_c
        v, run, bad = A.SmpcValidation(), C.c_uint64(0), C.c_uint64(0)
        self._ck(self.lib.sortham_optimizer_last_validation(self.h, C.byref(v), C.byref(run), C.byref(bad)))
        out = validation_from_c(v)
        out.run, out.invalid = run.value, bad.value
        return out

    def set_speed_limit(self, speed_limit, percentage):
        self._ck(self.lib.sortham_optimizer_set_speed_limit(self.h, speed_limit, int(percentage)))

    def reset(self):
        self._ck(self.lib.sortham_optimizer_reset(self.h))

    def get_control_sequence(self):
        u = np.zeros((3, self.T), np.float32)
        self._ck(self.lib.sortham_optimizer_get_control_sequence(self.h, _ptr(u)))
        return u

    def set_control_sequence(self, u):
        u = np.ascontiguousarray(u, np.float32)
        self._ck(self.lib.sortham_optimizer_set_control_sequence(self.h, _ptr(u)))

    def get_constraints(self):
        c = np.zeros(4, np.float32)
        s = C.c_int32(0)
        self._ck(self.lib.sortham_optimizer_get_constraints(self.h, _ptr(c), C.byref(s)))
        return c, bool(s.value)

    def get_optimized_trajectory(self):
        t = np.zeros((self.T, 3), np.float32)
        self._ck(self.lib.sortham_optimizer_get_optimized_trajectory(self.h, _ptr(t)))
        return t


class FleetError(RuntimeError):
    """A round (or the creation) of a fleet failed as a whole: .code is the SMPC_ERR_*."""

    def __init__(self, code, msg):
        super().__init__(f"[{code}] {msg}")
        self.code = code


class FleetOptimizer:
    """sortham::FleetOptimizer (host/fleet.hpp): Optimizer.eval_control for N robots through one
    grouped tick.  members: Optimizer objects, which the caller keeps and goes on using through their
    own methods between rounds; members and fleet may be closed in any order."""

    def __init__(self, members):
        self.lib = load_fleet_library()
        self.members = list(members)
        n = len(self.members)
        arr = (_ctx * max(n, 1))(*[m.h for m in self.members])
        h = _ctx()
        rc = self.lib.sortham_fleet_create(arr, n, C.byref(h))
        if rc != 0:
            raise FleetError(rc, (self.lib.sortham_fleet_last_error(None) or b"").decode())
        self.h = h
        self._ins = (A.SmpcTickIn * n)()
        self._outs = (A.SmpcTickOut * n)()
        self._tw = np.zeros((n, 3), np.float64)
        self._st = np.zeros(n, np.int32)

    def close(self):
        if getattr(self, "h", None):
            self.lib.sortham_fleet_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _fill(self, ticks, take):
        n = len(self.members)
        if len(ticks) != n or (take is not None and len(take) != n):
            raise ValueError("one tick (and one take entry) per member")
        on = [True] * n if take is None else [bool(v) for v in take]
        self._keep = list(ticks)        # (the plans the structs point to stay alive over the call)
        for i, t in enumerate(ticks):
            if on[i]:
                self._ins[i] = t.c
        mask = None if take is None else np.array(on, np.uint8)
        return on, mask

    def _results(self, on):
        from types import SimpleNamespace
        res = []
        for i, m in enumerate(self.members):
            st = int(self._st[i])
            if not on[i] or st == SORTHAM_FLEET_NOT_TAKEN:
                res.append(SimpleNamespace(twist=None, out=None, status=SORTHAM_FLEET_NOT_TAKEN, error=""))
                continue
            err = m.lib.sortham_optimizer_last_error(m.h).decode() if st == SORTHAM_ERR_THROWN else ""
            res.append(SimpleNamespace(twist=self._tw[i].copy(), out=A.SmpcTickOut.from_buffer_copy(self._outs[i]),
                                       status=st, error=err))
        return res

    def eval_control(self, ticks, take=None):
        """One round.  ticks: one Tick per member (None for a member that is not taken); take: one
        truth value per member, None = everybody.  -> one result per member with .twist (float64
        [vx, vy, wz]), .out (SmpcTickOut), .status (0, SORTHAM_FLEET_NOT_TAKEN, or SORTHAM_ERR_THROWN
        where that member's eval_control would have raised, the text in .error).  Raises FleetError
        when the round failed as a whole: no member's host state has moved then."""
        on, mask = self._fill(ticks, take)
        rc = self.lib.sortham_fleet_eval_control(self.h, self._ins, None if mask is None else _ptr(mask),
                                                 _ptr(self._tw), self._outs, _ptr(self._st))
        if rc != 0:
            raise FleetError(rc, self.lib.sortham_fleet_last_error(self.h).decode())
        return self._results(on)

    def critic_stats(self, ticks, take=None, per_rollout=False):
        """FleetOptimizer::getCriticStats: Optimizer.critic_stats for the members taken, the fleet staying
        grouped.  -> per member what Optimizer.critic_stats returns (optimizer.CriticStats) for the tick
        the next eval_control round would run first; None for a member that is not taken; the
        FleetError (not raised) with that member's code and text where its own call would have failed.
        The next round is unaffected.  Raises FleetError when the call failed as a whole."""
        from .optimizer import critic_names, critic_stats_from_c, load_library as load_smpc
        on, mask = self._fill(ticks, take)
        n = len(self.members)
        st = (A.SmpcCriticStats * n)()
        status = np.zeros(n, np.int32)
        rows = [np.empty((A.SMPC_STATS_ROWS, m.B), np.float32) if per_rollout and on[i] else None
                for i, m in enumerate(self.members)]
        rptr = (C.c_void_p * n)(*[r.ctypes.data if r is not None else None for r in rows])
        rc = self.lib.sortham_fleet_critic_stats(self.h, self._ins, None if mask is None else _ptr(mask), st,
                                                 rptr if per_rollout else None, _ptr(status))
        if rc != 0:
            raise FleetError(rc, self.lib.sortham_fleet_last_error(self.h).decode())
        names = critic_names(load_smpc())
        res = []
        for i, m in enumerate(self.members):
            if not on[i] or status[i] == SORTHAM_FLEET_NOT_TAKEN:
                res.append(None)
            elif status[i] != 0:
                res.append(FleetError(int(status[i]), m.lib.sortham_optimizer_last_error(m.h).decode()))
            else:
                res.append(critic_stats_from_c(A.SmpcCriticStats.from_buffer_copy(st[i]), names, rows[i]))
        return res

    def set_mutual_avoidance(self, robot_radius=None, collision_cost=None, repulsion_weight=None, margin=None):
        """FleetOptimizer::setMutualAvoidance: from the next round on every member taken scores the other
        members as moving obstacles.  robot_radius: one per member; None or empty: off."""
        p = moving_params(collision_cost, repulsion_weight, margin)
        r = np.zeros(0, np.float32) if robot_radius is None else np.ascontiguousarray(robot_radius, np.float32).reshape(-1)
        rc = self.lib.sortham_fleet_set_mutual_avoidance(self.h, C.byref(p), _ptr(r) if len(r) else None, len(r))
        if rc != 0:
            raise FleetError(rc, self.lib.sortham_fleet_last_error(self.h).decode())

    def run_rounds(self, ticks, n_rounds, take=None, alone=False):
        """sortham_fleet_run_rounds: n_rounds rounds on the same inputs from the compiled loop of
        host/tick_loop.cpp; alone: the members' own eval_control one after the other instead.
        -> the last round's results."""
        on, mask = self._fill(ticks, take)
        done = C.c_uint32(0)
        rc = self.lib.sortham_fleet_run_rounds(self.h, self._ins, None if mask is None else _ptr(mask), n_rounds,
                                               int(bool(alone)), _ptr(self._tw), self._outs, _ptr(self._st),
                                               C.byref(done))
        if rc != 0:
            raise FleetError(rc, f"after {done.value} of {n_rounds} rounds: "
                             + self.lib.sortham_fleet_last_error(self.h).decode())
        return self._results(on)

    def stats(self):
        """batched_launches / single_ticks of the fleet's groups (smpc_group_stats) and retries: the
        ticks the fleet ran alone in a member's fallback loop."""
        from types import SimpleNamespace
        a, b, c = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        rc = self.lib.sortham_fleet_stats(self.h, C.byref(a), C.byref(b), C.byref(c))
        if rc != 0:
            raise FleetError(rc, "sortham_fleet_stats")
        return SimpleNamespace(batched_launches=a.value, single_ticks=b.value, retries=c.value)

    def set_trajectory_validation(self, on=True, **kw):
        """Optimizer.set_trajectory_validation on every member: a round then validates the members'
        results in one grouped call, and an invalid member retries alone."""
        for m in self.members:
            m.set_trajectory_validation(on, **kw)

    def last_validation(self):
        """Optimizer.last_validation of every member."""
        return [m.last_validation() for m in self.members]

    def validation_counts(self):
        """(launches, members) of the fleet's grouped validation calls so far (smpc_group_validation_counts,
        summed over the fleet's groups): one launch per round, and one per retry of a member alone."""
        from types import SimpleNamespace
        a, b = C.c_uint64(0), C.c_uint64(0)
        rc = self.lib.sortham_fleet_validation_counts(self.h, C.byref(a), C.byref(b))
        if rc != 0:
            raise FleetError(rc, "sortham_fleet_validation_counts")
        return SimpleNamespace(launches=a.value, members=b.value)

    def moving_launches(self):
        """Mutual avoidance on the grouped route so far (smpc_debug_group_moving_launches, summed over
        the fleet's groups): grouped_launches of the grouped moving-obstacle kernels, table_uploads of
        a group's table buffer.  Both stay 0 under SMPC_FLEET_AVOID=per_member."""
        from types import SimpleNamespace
        a, b = C.c_uint64(0), C.c_uint64(0)
        rc = self.lib.sortham_fleet_moving_launches(self.h, C.byref(a), C.byref(b))
        if rc != 0:
            raise FleetError(rc, "sortham_fleet_moving_launches")
        return SimpleNamespace(grouped_launches=a.value, table_uploads=b.value)
