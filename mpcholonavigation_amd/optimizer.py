"""Python face of libsmpc.so (include/smpc.h): the hot path of
sortham::Optimizer::optimize() (reference src/optimizer.cpp:157-164) on MI355X.

There is no fallback: if the HIP library is missing or no GPU is present, the
constructor raises.  Names follow the reference: `optimize` is
Optimizer::optimize, `get_generated_trajectories` is
Optimizer::getGeneratedTrajectories, `reset` is Optimizer::reset's
device half.
"""
import ctypes as C
import dataclasses
import os
import sys
import types
from typing import Optional

import numpy as np

from . import _abi as A

_HERE = os.path.dirname(os.path.abspath(__file__))
# SMPC_LIB: developer override (kernel experiments build variants of the library side by side)
LIB_PATH = os.environ.get("SMPC_LIB") or os.path.join(_HERE, "libsmpc.so")
_lib = None


class SmpcError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"smpc error {code}: {msg}")
        self.code = code


def load_library():
    """dlopen libsmpc.so and bind every prototype of include/smpc.h and of the developer entry
    points (include/smpc_debug.h).  Raises if the library was not built (no silent fallback)."""
    global _lib
    if _lib is None:
        # libsmpc and PyTorch-ROCm both link libamdhip64.so.7 and the first copy loaded serves
        # the whole process.  torch only finds its GPUs with its own bundled runtime, while
        # libsmpc runs on either, so when torch is installed it goes first.
        if "torch" not in sys.modules and not os.environ.get("SMPC_NO_TORCH_PRELOAD"):
            try:
                import torch  # noqa: F401
            except ImportError:
                pass
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} not found: build it with `make -C mpcholonavigation_amd/csrc` "
                "(or __graft_entry__.build()); the sampling-MPC path has no CPU fallback")
        _lib = A.bind(A.bind(C.CDLL(LIB_PATH)), A.DEBUG_PROTOTYPES)
        if _lib.smpc_abi_version() != A.SMPC_ABI_VERSION:
            raise ImportError("libsmpc.so ABI version mismatch")
    return _lib


@dataclasses.dataclass
class CriticStats:
    """smpc_critic_stats with the names attached (Smpc.critic_stats).  The arrays have one entry per
    row of `names`: the twelve critics in scoring order, then "ControlCost" (the gamma term)."""
    names: tuple
    scored_mask: int
    fail_flag: bool
    batch: int
    best_rollout: int
    best_cost: float
    effective_samples: float
    sum: np.ndarray
    min: np.ndarray
    max: np.ndarray
    weighted: np.ndarray
    at_best: np.ndarray
    per_rollout: Optional[np.ndarray] = None   # [13, B] float32 when asked for

    def scored(self, name):
        """Whether the row called `name` ("PathAlignCritic", ...) was scored on this tick."""
        return bool(self.scored_mask >> self.names.index(name) & 1)

    def as_dict(self):
        """{name: {"sum", "min", "max", "mean", "weighted", "at_best"}} of the scored rows."""
        return {n: {"sum": float(self.sum[k]), "min": float(self.min[k]), "max": float(self.max[k]),
                    "mean": float(self.sum[k]) / max(self.batch, 1), "weighted": float(self.weighted[k]),
                    "at_best": float(self.at_best[k])}
                for k, n in enumerate(self.names) if self.scored_mask >> k & 1}


def critic_names(lib=None):
    """The rows of a breakdown: smpc_critic_name(0 .. SMPC_STATS_ROWS - 1)."""
    lib = lib or load_library()
    return tuple(lib.smpc_critic_name(k).decode() for k in range(A.SMPC_STATS_ROWS))


def critic_stats_from_c(st, names, per_rollout=None):
    rows = {f: np.array(getattr(st, f), np.float32) for f in ("sum", "min", "max", "weighted", "at_best")}
    return CriticStats(names=names, scored_mask=int(st.scored_mask), fail_flag=bool(st.fail_flag),
                       batch=int(st.batch), best_rollout=int(st.best_rollout), best_cost=float(st.best_cost),
                       effective_samples=float(st.effective_samples), per_rollout=per_rollout, **rows)


@dataclasses.dataclass
class Validation:
    """smpc_validation (Smpc.validate_trajectory): the verdict on one control sequence's trajectory."""
    valid: bool
    checked: int
    first_bad: int
    cause: int                  # 0, 1 costmap, 2 moving obstacle
    disc: int
    cost: float
    xyyaw: Optional[np.ndarray] = None   # [T, 3] float32 poses when asked for


def validation_params(lib, collision_lookahead_time=None, consider_footprint=None, moving_obstacles=None):
    """smpc_validation_params with the library's defaults where an argument is None."""
    p = A.SmpcValidationParams()
    lib.smpc_validation_params_default(C.byref(p))
    if collision_lookahead_time is not None:
        p.collision_lookahead_time = collision_lookahead_time
    if consider_footprint is not None:
        p.consider_footprint = int(bool(consider_footprint))
    if moving_obstacles is not None:
        p.moving_obstacles = int(bool(moving_obstacles))
    return p


def validation_from_c(v, xyyaw=None):
    return Validation(valid=bool(v.valid), checked=int(v.checked), first_bad=int(v.first_bad), cause=int(v.cause),
                      disc=int(v.disc), cost=float(v.cost), xyyaw=xyyaw)


def _ptr(a):
    if a is None:
        return None
    assert a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(C.c_void_p)


class Smpc:
    """One optimizer context on one GPU (smpc_ctx)."""

    def __init__(self, cfg: A.SmpcConfig):
        self.lib = load_library()
        self.cfg = cfg
        self.B, self.T = cfg.batch_size, cfg.time_steps
        h = C.c_void_p()
        rc = self.lib.smpc_create(C.byref(cfg), C.byref(h))
        if rc != 0:
            raise SmpcError(rc, self.lib.smpc_last_error(None).decode())
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.lib.smpc_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc):
        if rc != 0:
            raise SmpcError(rc, self.lib.smpc_last_error(self.h).decode())

    # ---- configuration ---------------------------------------------------
    def reset(self):
        self._ck(self.lib.smpc_reset(self.h))

    def set_constraints(self, vx_max, vx_min, vy_max, wz_max):
        self._ck(self.lib.smpc_set_constraints(self.h, vx_max, vx_min, vy_max, wz_max))

    def set_acceleration_limits(self, ax_max, ax_min, ay_max, az_max):
        """Bounds on how fast a sampled control may change (m/s^2, m/s^2, rad/s^2); all zero: off."""
        self._ck(self.lib.smpc_set_acceleration_limits(self.h, ax_max, ax_min, ay_max, az_max))

    def get_acceleration_limits(self):
        out = (C.c_float * 4)()
        self._ck(self.lib.smpc_get_acceleration_limits(self.h, out))
        return tuple(float(v) for v in out)

    def get_limited_noise(self):
        """The limited noise [B, T] x 3 the last tick's last iteration scored with."""
        out = [np.empty((self.B, self.T), np.float32) for _ in range(3)]
        self._ck(self.lib.smpc_get_limited_noise(self.h, _ptr(out[0]), _ptr(out[1]), _ptr(out[2])))
        return out

    def set_moving_obstacles(self, xy=None, radius=None, collision_cost=None, repulsion_weight=None, margin=None):
        """Discs that move with the trajectory index: xy [n, T, 2] (costmap world frame: where disc k
        is when the robot is at trajectory point t), radius [n] (centre-to-centre collision distance).
        Parameters left None keep the library's defaults.  xy None or empty: off."""
        p = A.SmpcMovingObstaclesParams()
        self.lib.smpc_moving_obstacles_params_default(C.byref(p))
        for name, v in (("collision_cost", collision_cost), ("repulsion_weight", repulsion_weight), ("margin", margin)):
            if v is not None:
                setattr(p, name, v)
        if xy is None or len(xy) == 0:
            self._ck(self.lib.smpc_set_moving_obstacles(self.h, C.byref(p), None, None, 0))
            return
        xy = np.ascontiguousarray(xy, dtype=np.float32)
        radius = np.ascontiguousarray(radius, dtype=np.float32).reshape(-1)
        if xy.ndim != 3 or xy.shape[1:] != (self.T, 2) or radius.shape[0] != xy.shape[0]:
            raise ValueError("xy must be [n, time_steps, 2] and radius [n]")
        self._ck(self.lib.smpc_set_moving_obstacles(self.h, C.byref(p), _ptr(xy), _ptr(radius), xy.shape[0]))

    def moving_obstacle_costs(self):
        """(m [B] float32, hit [B] bool) of the last tick's last iteration."""
        m = np.empty(self.B, np.float32)
        hit = np.empty(self.B, np.uint8)
        self._ck(self.lib.smpc_get_moving_obstacle_costs(self.h, _ptr(m), _ptr(hit)))
        return m, hit.astype(bool)

    def set_critics(self, p: A.SmpcCriticParams):
        self._ck(self.lib.smpc_set_critics(self.h, C.byref(p)))

    def set_costmap(self, cells, origin_x, origin_y, resolution, track_unknown=False,
                    inscribed_radius=0.1, cost_scaling_factor=10.0, inflation_radius=0.55):
        cells = np.ascontiguousarray(cells, dtype=np.uint8)
        if cells.ndim != 2:
            raise ValueError("cells must be [height, width]")
        h, w = cells.shape
        self._ck(self.lib.smpc_set_costmap(
            self.h, _ptr(cells), w, h, origin_x, origin_y, resolution, int(track_unknown),
            inscribed_radius, cost_scaling_factor, inflation_radius))

    def update_costmap_region(self, cells, x0, y0, width, height):
        """Hand over the window [y0:y0+height, x0:x0+width] of the caller's full map `cells`."""
        cells = np.ascontiguousarray(cells, dtype=np.uint8)
        if cells.ndim != 2:
            raise ValueError("cells must be the full [height, width] map")
        first = cells[y0:, x0:]          # a view: the pointer of the window's first cell
        self._ck(self.lib.smpc_update_costmap_region(
            self.h, C.c_void_p(first.ctypes.data), cells.shape[1], x0, y0, width, height))

    def costmap_upload_bytes(self):
        """(bytes uploaded by the last set_costmap / update_costmap_region, total so far)."""
        last, total = C.c_uint64(0), C.c_uint64(0)
        self._ck(self.lib.smpc_costmap_upload_bytes(self.h, C.byref(last), C.byref(total)))
        return last.value, total.value

    def set_footprint(self, xy, circumscribed_radius, layer_cost_scaling_factor=10.0):
        """Robot footprint [n, 2] (robot frame) for consider_footprint=true."""
        xy = np.ascontiguousarray(xy, dtype=np.float64).reshape(-1, 2)
        self._ck(self.lib.smpc_set_footprint(self.h, xy.ctypes.data_as(C.c_void_p), len(xy),
                                             float(circumscribed_radius), float(layer_cost_scaling_factor)))

    def set_noise(self, nvx, nvy, nwz):
        a = [np.ascontiguousarray(x, dtype=np.float32) for x in (nvx, nvy, nwz)]
        for x in a:
            if x.shape != (self.B, self.T):
                raise ValueError(f"noise must be [{self.B}, {self.T}]")
        self._ck(self.lib.smpc_set_noise(self.h, _ptr(a[0]), _ptr(a[1]), _ptr(a[2])))

    def seed(self, seed):
        self._ck(self.lib.smpc_seed(self.h, seed))

    def redraw_noise(self):
        self._ck(self.lib.smpc_redraw_noise(self.h))

    def redraw_noise_async(self):
        """The next epoch drawn in the background; the next tick takes it (smpc_redraw_noise_async)."""
        self._ck(self.lib.smpc_redraw_noise_async(self.h))

    def get_noise(self):
        out = [np.empty((self.B, self.T), np.float32) for _ in range(3)]
        self._ck(self.lib.smpc_get_noise(self.h, _ptr(out[0]), _ptr(out[1]), _ptr(out[2])))
        return out

    # ---- hot path ----------------------------------------------------------
    def optimize(self, tick, u):
        """u: float32 [3, T] (vx, vy, wz) -> (u_new, SmpcTickOut)."""
        u = np.array(u, dtype=np.float32, order="C")      # a copy: the call updates it in place
        if u.shape != (3, self.T):
            raise ValueError(f"u must be [3, {self.T}]")
        out = A.SmpcTickOut()
        rc = self.lib.smpc_optimize(self.h, C.byref(tick.c), u.ctypes.data, C.byref(out))
        if rc != 0:
            self._ck(rc)
        return u, out

    def get_generated_trajectories(self):
        out = [np.empty((self.B, self.T), np.float32) for _ in range(3)]
        self._ck(self.lib.smpc_get_trajectories(self.h, _ptr(out[0]), _ptr(out[1]),
                                                _ptr(out[2])))
        return out

    def get_costs(self):
        c = np.empty(self.B, np.float32)
        self._ck(self.lib.smpc_get_costs(self.h, _ptr(c)))
        return c

    def critic_stats(self, tick, u, per_rollout=False):
        """Per-critic costs and effective samples of the tick optimize(tick, u) would run next
        (smpc_critic_breakdown): its first iteration, scored without changing anything the next
        tick depends on.  per_rollout: also every rollout's rows, float32 [13, B]."""
        u = np.ascontiguousarray(u, dtype=np.float32)
        if u.shape != (3, self.T):
            raise ValueError(f"u must be [3, {self.T}]")
        st = A.SmpcCriticStats()
        rows = np.empty((A.SMPC_STATS_ROWS, self.B), np.float32) if per_rollout else None
        self._ck(self.lib.smpc_critic_breakdown(self.h, C.byref(tick.c), _ptr(u), C.byref(st), _ptr(rows)))
        return critic_stats_from_c(st, critic_names(self.lib), rows)

    def validate_trajectory(self, pose, u, collision_lookahead_time=None, consider_footprint=None,
                            moving_obstacles=None, poses=False):
        """Collision check of the trajectory the control sequence u [3, T] drives from pose (x, y,
        yaw) (smpc_validate_trajectory): the costmap under the first lookahead / model_dt poses,
        with the footprint if asked, and the moving obstacles set on the context.  Arguments left
        None keep the library's defaults (2.0 s, no footprint, moving obstacles on).  poses: also
        the [T, 3] poses.  Changes nothing a tick depends on."""
        u = np.ascontiguousarray(u, dtype=np.float32)
        if u.shape != (3, self.T):
            raise ValueError(f"u must be [3, {self.T}]")
        p = validation_params(self.lib, collision_lookahead_time, consider_footprint, moving_obstacles)
        out = A.SmpcValidation()
        xyyaw = np.empty((self.T, 3), np.float32) if poses else None
        self._ck(self.lib.smpc_validate_trajectory(self.h, C.byref(p), float(pose[0]), float(pose[1]), float(pose[2]),
                                                   _ptr(u), C.byref(out), _ptr(xyyaw)))
        return validation_from_c(out, xyyaw)

    def selftest_sincos(self, x):
        x = np.ascontiguousarray(x, dtype=np.float32)
        s, c = np.empty_like(x), np.empty_like(x)
        self._ck(self.lib.smpc_selftest_sincos(self.h, _ptr(x), x.size, _ptr(s), _ptr(c)))
        return s, c

    def selftest_philox(self, ctr, key):
        """The noise generator's Philox4x32-10: ctr uint32 [n, 4], key (k0, k1) -> uint32 [n, 4]."""
        ctr = np.ascontiguousarray(ctr, dtype=np.uint32).reshape(-1, 4)
        key = np.ascontiguousarray(key, dtype=np.uint32).reshape(2)
        out = np.empty_like(ctr)
        self._ck(self.lib.smpc_selftest_philox(self.h, _ptr(ctr), _ptr(key), ctr.shape[0], _ptr(out)))
        return out

    def selftest_box_muller(self, r0, r1):
        """The noise generator's Box-Muller on pairs of Philox words -> (radius cos, radius sin)."""
        r0 = np.ascontiguousarray(r0, dtype=np.uint32).reshape(-1)
        r1 = np.ascontiguousarray(r1, dtype=np.uint32).reshape(-1)
        if r0.shape != r1.shape:
            raise ValueError("one second word per first word")
        z0, z1 = np.empty(r0.size, np.float32), np.empty(r0.size, np.float32)
        self._ck(self.lib.smpc_selftest_box_muller(self.h, _ptr(r0), _ptr(r1), r0.size, _ptr(z0), _ptr(z1)))
        return z0, z1

    def selftest_lane_reduce(self, v, w):
        """out[t] = sum_b w[b] v[b, t] through the lane pass's in-register transpose-reduce."""
        v = np.ascontiguousarray(v, dtype=np.float32).reshape(64, 64)
        w = np.ascontiguousarray(w, dtype=np.float32).reshape(64)
        out = np.empty(64, np.float32)
        self._ck(self.lib.smpc_selftest_lane_reduce(self.h, _ptr(v), _ptr(w), _ptr(out)))
        return out

    # ---- batch-sharded phases (device pointers are plain ints) ------------------
    def selftest_row_reduce(self, v):
        """smpc_split.hip's N x N transpose-reduce per group of N lanes: v [64 lanes][N] -> [64], N = 16 or 32."""
        v = np.ascontiguousarray(v, dtype=np.float32)
        out = np.empty(64, np.float32)
        self._ck(self.lib.smpc_selftest_row_reduce(self.h, _ptr(v), v.shape[1], _ptr(out)))
        return out

    def last_pass_kernel(self) -> str:
        """The scoring-pass instance this thread launched last, as a kernel trace spells it
        (smpc_debug_last_pass_kernel: a developer aid, include/smpc_debug.h)."""
        return self.lib.smpc_debug_last_pass_kernel().decode()

    def set_stream(self, hip_stream):
        self._ck(self.lib.smpc_set_stream(self.h, C.c_void_p(hip_stream)))

    def set_profile(self, enable):
        """SMPC_FLAG_PROFILE on/off: HIP events around the scoring pass (costs ~15 us/tick)."""
        self._ck(self.lib.smpc_set_profile(self.h, int(bool(enable))))

    @property
    def tuple_len(self):
        return self.lib.smpc_tuple_len(self.h)

    def shard_begin(self, tick, u):
        u = np.ascontiguousarray(u, dtype=np.float32)
        self._ck(self.lib.smpc_shard_begin(self.h, C.byref(tick.c), _ptr(u)))

    def shard_predicted_furthest(self):
        """The index this tick is expected to have (after shard_begin), or None."""
        h = C.c_uint32(0)
        return int(h.value) if self.lib.smpc_shard_predicted_furthest(self.h, C.byref(h)) else None

    def shard_furthest(self, d_furthest):
        self._ck(self.lib.smpc_shard_furthest(self.h, C.c_void_p(d_furthest)))

    def shard_score(self, d_furthest, furthest_hint, d_tuple):
        self._ck(self.lib.smpc_shard_score(
            self.h, C.c_void_p(d_furthest) if d_furthest else None, int(furthest_hint),
            C.c_void_p(d_tuple)))

    def shard_rescore_failed(self, d_tuple):
        self._ck(self.lib.smpc_shard_rescore_failed(self.h, C.c_void_p(d_tuple)))

    # ---- the sharded tick with the exchanges inside the library (RCCL) ------------
    def shard_comm_id(self):
        """A fresh RCCL unique id (bytes); rank 0 makes it and ships it to every rank."""
        buf = (C.c_ubyte * A.SMPC_COMM_ID_BYTES)()
        rc = self.lib.smpc_shard_comm_id(buf, A.SMPC_COMM_ID_BYTES)
        if rc != 0:
            raise SmpcError(rc, self.lib.smpc_last_error(None).decode())
        return bytes(buf)

    def shard_comm_init(self, comm_id, rank, world):
        buf = (C.c_ubyte * A.SMPC_COMM_ID_BYTES).from_buffer_copy(comm_id)
        self._ck(self.lib.smpc_shard_comm_init(self.h, buf, int(rank), int(world)))

    def shard_p2p_handle(self):
        """IPC handle (bytes) of this context's mailbox for the collective-free exchange."""
        buf = C.create_string_buffer(64)
        self._ck(self.lib.smpc_shard_p2p_handle(self.h, buf, 64))
        return buf.raw

    def shard_p2p_init(self, handles, rank, world):
        """handles: the mailbox handles of all ranks, in rank order."""
        if len(handles) != world or any(len(h) != 64 for h in handles):
            raise ValueError("one 64-byte handle per rank")
        blob = b"".join(handles)
        self._ck(self.lib.smpc_shard_p2p_init(self.h, C.c_char_p(blob), rank, world))

    def shard_p2p_set_timeout(self, milliseconds):
        """Wall-clock bound of the in-kernel wait for the peers' tuples (default 10 000 ms)."""
        self._ck(self.lib.smpc_shard_p2p_set_timeout(self.h, int(milliseconds)))

    def shard_tick(self, tick, u, speculate=True):
        """One batch-sharded tick, ncclAllGather / ncclAllReduce included (collective)."""
        u = np.ascontiguousarray(u, dtype=np.float32).copy()
        out = A.SmpcTickOut()
        self._ck(self.lib.smpc_shard_tick(self.h, C.byref(tick.c), _ptr(u), C.byref(out),
                                          1 if speculate else 0))
        return u, out

    def shard_combine(self, d_tuples, n_tuples):
        u = np.zeros((3, self.T), np.float32)
        out = A.SmpcTickOut()
        self._ck(self.lib.smpc_shard_combine(self.h, C.c_void_p(d_tuples), n_tuples, _ptr(u),
                                             C.byref(out)))
        return u, out


class SmpcGroup:
    """Several Smpc contexts ticked with one launch (include/smpc.h: smpc_group_*)."""

    def __init__(self, members):
        self.members = list(members)
        self.lib = self.members[0].lib
        n = len(self.members)
        arr = (A._ctx * n)(*[m.h for m in self.members])
        h = A._ctx()
        rc = self.lib.smpc_group_create(arr, n, C.byref(h))
        if rc != 0:
            raise SmpcError(rc, self.lib.smpc_last_error(None).decode())
        self.h = h

    def optimize(self, ticks, us, take=None):
        """ticks, us: one per member; returns [(u_new, SmpcTickOut)] in member order.
        take (smpc_group_optimize_some): one truth value per member; a member left out is not
        ticked at all — its entries of ticks and us may be None, and its result is None."""
        n = len(self.members)
        if getattr(self, "_ins", None) is None or len(ticks) != n:
            if len(ticks) != n:
                raise ValueError("one tick per member")
            self._ins = (A.SmpcTickIn * n)()
            self._src = [None] * n
            self._bufs = np.empty((n, 3, self.members[0].T), np.float32)
            self._ptrs = (C.c_void_p * n)(*[self._bufs[i].ctypes.data for i in range(n)])
            self._outs = (A.SmpcTickOut * n)()
        if take is not None and len(take) != n:
            raise ValueError("one take entry per member")
        on = [True] * n if take is None else [bool(v) for v in take]
        for i, t in enumerate(ticks):
            if not on[i]:
                continue
            # Tick.c is rebuilt whenever a field of the tick was assigned: copy it again when
            # it is not the struct object this slot was filled from (an identity check per member)
            c = t.c
            if self._src[i] is not c:
                self._ins[i] = c
                self._src[i] = c
        for i, u in enumerate(us):
            if on[i]:
                self._bufs[i] = u
        if take is None:
            rc = self.lib.smpc_group_optimize(self.h, self._ins, self._ptrs, self._outs)
        else:
            mask = (C.c_uint8 * n)(*[int(v) for v in on])
            rc = self.lib.smpc_group_optimize_some(self.h, self._ins, self._ptrs, self._outs, mask)
        if rc != 0:
            msg = next((m.lib.smpc_last_error(m.h).decode() for m in self.members
                        if m.lib.smpc_last_error(m.h)), "")
            raise SmpcError(rc, msg)
        res = self._bufs.copy()
        return [(res[i], A.SmpcTickOut.from_buffer_copy(self._outs[i])) if on[i] else None for i in range(n)]

    def stats(self):
        """How the group's ticks went so far (smpc_group_stats): batched_launches — scoring launches
        that carried two or more members; single_ticks — members ticked through smpc_optimize."""
        launches, singles = C.c_uint64(0), C.c_uint64(0)
        rc = self.lib.smpc_group_stats(self.h, C.byref(launches), C.byref(singles))
        if rc != 0:
            raise SmpcError(rc, "smpc_group_stats")
        return types.SimpleNamespace(batched_launches=launches.value, single_ticks=singles.value)

    def set_moving_obstacles(self, tables, take=None):
        """Smpc.set_moving_obstacles for the members in one call (smpc_group_set_moving_obstacles): one
        staging fill, one upload and one event for the whole group.  tables: one entry per member —
        None (the member's term off) or (xy [n, T, 2], radius [n][, params]) with params a dict of
        collision_cost / repulsion_weight / margin (what is left out keeps the library's default).
        take: one truth value per member; a member left out keeps its table.  All or nothing: on
        an error no member has changed."""
        n = len(self.members)
        if len(tables) != n:
            raise ValueError("one table (or None) per member")
        if take is not None and len(take) != n:
            raise ValueError("one take entry per member")
        on = [True] * n if take is None else [bool(v) for v in take]
        T = self.members[0].T
        params = (A.SmpcMovingObstaclesParams * n)()
        xys, radii = [None] * n, [None] * n
        counts = (C.c_uint32 * n)()
        for i in range(n):
            self.lib.smpc_moving_obstacles_params_default(C.byref(params[i]))
            if not on[i] or tables[i] is None:
                continue
            xy, radius = tables[i][0], tables[i][1]
            for name, v in (tables[i][2] if len(tables[i]) > 2 and tables[i][2] else {}).items():
                if name not in ("collision_cost", "repulsion_weight", "margin"):
                    raise ValueError(f"unknown moving-obstacle parameter {name!r}")
                setattr(params[i], name, v)
            if xy is None or len(xy) == 0:
                continue
            xy = np.ascontiguousarray(xy, dtype=np.float32)
            radius = np.ascontiguousarray(radius, dtype=np.float32).reshape(-1)
            if xy.ndim != 3 or xy.shape[1:] != (T, 2) or radius.shape[0] != xy.shape[0]:
                raise ValueError(f"member {i}: xy must be [n, time_steps, 2] and radius [n]")
            xys[i], radii[i], counts[i] = xy, radius, xy.shape[0]
        xptr = (C.c_void_p * n)(*[a.ctypes.data if a is not None else None for a in xys])
        rptr = (C.c_void_p * n)(*[a.ctypes.data if a is not None else None for a in radii])
        mask = None if take is None else (C.c_uint8 * n)(*[int(v) for v in on])
        rc = self.lib.smpc_group_set_moving_obstacles(self.h, params, xptr, rptr, counts, mask)
        if rc != 0:
            raise SmpcError(rc, self.lib.smpc_last_error(None).decode())

    def moving_launches(self):
        """The grouped route of the moving obstacles so far (smpc_debug_group_moving_launches):
        grouped_launches — launches of the grouped moving-obstacle kernels (one per form and round,
        whatever the number of members); table_uploads — uploads of the group's table buffer."""
        launches, uploads = C.c_uint64(0), C.c_uint64(0)
        rc = self.lib.smpc_debug_group_moving_launches(self.h, C.byref(launches), C.byref(uploads))
        if rc != 0:
            raise SmpcError(rc, "smpc_debug_group_moving_launches")
        return types.SimpleNamespace(grouped_launches=launches.value, table_uploads=uploads.value)

    def critic_stats(self, ticks, us, take=None, per_rollout=False):
        """Smpc.critic_stats for the members, the group staying a group (smpc_group_critic_breakdown):
        ticks, us — one per member, as optimize takes them, us read only.  Returns one entry per
        member: what Smpc.critic_stats returns on an identical context outside any group, bit for
        bit; None for a member left out by take; the SmpcError (not raised: the others have their
        statistics) for a member the call refused on its own, e.g. both collision critics with a
        footprint.  Changes nothing the next optimize depends on."""
        n = len(self.members)
        if len(ticks) != n or len(us) != n:
            raise ValueError("one tick and one control sequence per member")
        if take is not None and len(take) != n:
            raise ValueError("one take entry per member")
        on = [True] * n if take is None else [bool(v) for v in take]
        ins = (A.SmpcTickIn * n)()
        T = self.members[0].T
        ubuf = np.zeros((n, 3, T), np.float32)
        rows = [np.empty((A.SMPC_STATS_ROWS, m.B), np.float32) if per_rollout and on[i] else None
                for i, m in enumerate(self.members)]
        for i in range(n):
            if on[i]:
                ins[i] = ticks[i].c
                u = np.asarray(us[i], dtype=np.float32)
                if u.shape != (3, T):
                    raise ValueError(f"u must be [3, {T}]")
                ubuf[i] = u
        uptr = (C.c_void_p * n)(*[ubuf[i].ctypes.data for i in range(n)])
        rptr = (C.c_void_p * n)(*[r.ctypes.data if r is not None else None for r in rows])
        st = (A.SmpcCriticStats * n)()
        status = (C.c_int32 * n)()
        mask = None if take is None else (C.c_uint8 * n)(*[int(v) for v in on])
        rc = self.lib.smpc_group_critic_breakdown(self.h, ins, uptr, mask, st, rptr if per_rollout else None, status)
        if rc != 0:
            msg = next((m.lib.smpc_last_error(m.h).decode() for m in self.members
                        if m.lib.smpc_last_error(m.h)), "") or self.lib.smpc_last_error(None).decode()
            raise SmpcError(rc, msg)
        names = critic_names(self.lib)
        res = []
        for i, m in enumerate(self.members):
            if not on[i]:
                res.append(None)
            elif status[i] != 0:
                res.append(SmpcError(int(status[i]), m.lib.smpc_last_error(m.h).decode()))
            else:
                res.append(critic_stats_from_c(A.SmpcCriticStats.from_buffer_copy(st[i]), names, rows[i]))
        return res

    def breakdown_counts(self):
        """Which way the member-breakdowns of critic_stats went so far (smpc_group_breakdown_counts):
        batched_members rode a grouped stats launch, single_members were scored one by one."""
        b, s = C.c_uint64(0), C.c_uint64(0)
        rc = self.lib.smpc_group_breakdown_counts(self.h, C.byref(b), C.byref(s))
        if rc != 0:
            raise SmpcError(rc, "smpc_group_breakdown_counts")
        return types.SimpleNamespace(batched_members=b.value, single_members=s.value)

    def validate_trajectories(self, poses, us, params=None, take=None, want_poses=False):
        """Smpc.validate_trajectory for the members in one upload, one launch and one wait
        (smpc_group_validate_trajectories).  poses: one (x, y, yaw) per member; us: one [3, T] per
        member; params: None, one dict of validate_trajectory's keywords for all, or one per member.
        Returns one entry per member: a Validation; None for a member left out by take; the
        SmpcError (not raised) for a member the call refused on its own."""
        n = len(self.members)
        if len(poses) != n or len(us) != n:
            raise ValueError("one pose and one control sequence per member")
        if take is not None and len(take) != n:
            raise ValueError("one take entry per member")
        if params is None or isinstance(params, dict):
            params = [params or {}] * n
        if len(params) != n:
            raise ValueError("one parameter dict per member")
        on = [True] * n if take is None else [bool(v) for v in take]
        T = self.members[0].T
        cp = (A.SmpcValidationParams * n)()
        pose = np.zeros((n, 3), np.float64)
        ubuf = np.zeros((n, 3, T), np.float32)
        for i in range(n):
            cp[i] = validation_params(self.lib, **(params[i] or {}))
            if on[i]:
                pose[i] = poses[i]
                u = np.asarray(us[i], dtype=np.float32)
                if u.shape != (3, T):
                    raise ValueError(f"u must be [3, {T}]")
                ubuf[i] = u
        xy = [np.empty((T, 3), np.float32) if want_poses and on[i] else None for i in range(n)]
        uptr = (C.c_void_p * n)(*[ubuf[i].ctypes.data for i in range(n)])
        xptr = (C.c_void_p * n)(*[a.ctypes.data if a is not None else None for a in xy])
        out = (A.SmpcValidation * n)()
        status = (C.c_int32 * n)()
        mask = None if take is None else (C.c_uint8 * n)(*[int(v) for v in on])
        rc = self.lib.smpc_group_validate_trajectories(self.h, cp, pose.ctypes.data_as(C.POINTER(C.c_double)), uptr, mask,
                                                       out, xptr if want_poses else None, status)
        if rc != 0:
            msg = next((m.lib.smpc_last_error(m.h).decode() for m in self.members
                        if m.lib.smpc_last_error(m.h)), "") or self.lib.smpc_last_error(None).decode()
            raise SmpcError(rc, msg)
        res = []
        for i, m in enumerate(self.members):
            if not on[i]:
                res.append(None)
            elif status[i] != 0:
                res.append(SmpcError(int(status[i]), m.lib.smpc_last_error(m.h).decode()))
            else:
                res.append(validation_from_c(A.SmpcValidation.from_buffer_copy(out[i]), xy[i]))
        return res

    def validation_counts(self):
        """(launches, members) of validate_trajectories so far (smpc_group_validation_counts)."""
        a, b = C.c_uint64(0), C.c_uint64(0)
        rc = self.lib.smpc_group_validation_counts(self.h, C.byref(a), C.byref(b))
        if rc != 0:
            raise SmpcError(rc, "smpc_group_validation_counts")
        return types.SimpleNamespace(launches=a.value, members=b.value)

    def close(self):
        if self.h:
            self.lib.smpc_group_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
