"""Scenes whose rollout points sit on costmap cell edges, and a float64 judge for them.

Every scoring pass decides which costmap cell a rollout point falls in, each kernel family with a
float fast path of its own and the reference's double arithmetic only inside a guard band.  The
parity tests cannot see a wrong cell: GPU and oracle positions differ in the last ulp (sinf, fma
contraction), so they tolerate a budget of flipped cells.  The scenes here make the positions
bit-identical on every side, so that ANY flip is a cell-index defect:

  * yaw 0, speed 0, warm start 0, no wz noise, model_dt = 2^-4: sin and cos are exactly 0 and 1,
    vx cos - vy sin is exactly vx;
  * the stored noise is diff(a) / dt for accumulated displacements a_t that are multiples of
    2^-20 m with |a| < 8 m: every partial sum is exact in float32, whatever the summation order
    (sequential, DPP scan, segment prefix), and x = (float)(pose + (double)a) is the same float;
  * a_t = round((origin + m res - pose) / 2^-20) 2^-20 + j d with j in {-1, 0, 1} and d the larger
    of 2^-20 and a float ulp of the map's coordinates: the point lands on the cell edge of index
    m, or on one of its float neighbours;
  * the costmap is a 2 x 2 checkerboard of four cost classes: all eight neighbours of a cell carry
    another cost, so one wrong lookup moves the rollout's cost by min_single_lookup_shift().

Not a conftest: plain helpers, imported by tests/test_cell_index_cpu.py (which pins the premise on
the oracle alone and checks that the scenes are adversarial) and tests/test_gpu_cell_index.py.
"""
from dataclasses import dataclass, field

import numpy as np

from mpcholonavigation_amd import _abi as A
from mpcholonavigation_amd.tick import Tick, default_config
from tests import harness as H
from tests.kernel_names import lane, wave

QUANTUM = 2.0 ** -20          # metres: the grid of the accumulated displacements
MODEL_DT = 0.0625             # 2^-4 s
MAX_DISPLACEMENT = 8.0        # metres: |a| below it, so that a and its increments fit 24 bits
CLASSES = (0, 60, 130, 220)   # cells[my, mx] = CLASSES[(mx & 1) + 2 (my & 1)]
# a near-goal tick drops ObstaclesCritic's repulsive term, which is all that tells 60 from 0:
# its scenes use four classes that the critical term separates
CLASSES_NEAR_GOAL = (0, 130, 175, 220)
ALL_CRITICS = H.ALL_CRITICS


@dataclass
class EdgeScene:
    cells: np.ndarray            # uint8 [H, W]
    origin_x: float
    origin_y: float
    resolution: float
    track_unknown: bool
    near_goal: bool
    holonomic: bool
    B: int
    T: int
    tick: Tick
    u0: np.ndarray               # float32 [3, T], zeros
    noise: tuple                 # (nvx, nvy, nwz) float32 [B, T]
    ax: np.ndarray               # float64 [B, T] intended accumulated displacements
    ay: np.ndarray
    x: np.ndarray                # float32 [B, T] expected trajectory points
    y: np.ndarray
    classes: tuple = CLASSES
    label: str = ""
    inscribed_radius: float = 0.1
    cost_scaling_factor: float = 10.0
    inflation_radius: float = 0.55
    extra: dict = field(default_factory=dict)

    def config(self, **kw):
        mm = A.SMPC_MODEL_OMNI if self.holonomic else A.SMPC_MODEL_DIFF_DRIVE
        return default_config(batch_size=self.B, time_steps=self.T, model_dt=MODEL_DT, motion_model=mm, **kw)

    def configure(self, obj, critics):
        """The same costmap, critics and noise on a Smpc or an Oracle."""
        obj.set_critics(critics)
        obj.set_costmap(self.cells, self.origin_x, self.origin_y, self.resolution,
                        track_unknown=self.track_unknown, inscribed_radius=self.inscribed_radius,
                        cost_scaling_factor=self.cost_scaling_factor, inflation_radius=self.inflation_radius)
        obj.set_noise(*self.noise)


def critics_of(names, **over):
    """Default parameters (every cost_power too), only the named critics enabled."""
    return H.critics_of(names, power=None, **over)


def checkerboard(W, H, classes=CLASSES):
    my, mx = np.mgrid[0:H, 0:W]
    return np.asarray(classes, np.uint8)[(mx & 1) + 2 * (my & 1)]


def _quantise(v):
    return np.rint(np.asarray(v, np.float64) / QUANTUM) * QUANTUM


def _walk(rng, kind, B, T, n, c0, aim, reach):
    """Integer walk [B, T] along one axis of n cells, from the robot's cell c0.
    local:  +-2 cells per step, at most 40 cells from the robot (inside the 96-cell LDS window);
    far:    1 or 2 cells per step (twice that below 48 steps) in one direction per rollout, up to
            `reach` cells: past the window, inside the map;
    border: 3 cells per step towards the border aim[b] (0: edge 0, 1: edge n); an even rollout
            touches that border edge for ONE step and comes back in (where the map's outside is a
            collision, it collides if and only if that one point is outside: nothing later hides
            a wrong decision); an odd one stays six steps ON the edge, then leaves the map, a
            cell per step for four cells; aim[b] < 0: a local walk."""
    if kind == "far":
        sign = rng.choice(np.array([-1, 1]), size=(B, 1))
        stride = 1 if T >= 48 else 2          # (a short horizon still has to get past the window)
        m = c0 + np.clip(np.cumsum(sign * stride * rng.integers(1, 3, size=(B, T)), axis=1), -reach, reach)
        return np.clip(m, 2, n - 2)
    m = c0 + np.clip(np.cumsum(rng.integers(-2, 3, size=(B, T)), axis=1), -40, 40)
    m = np.clip(m, 1, n - 1)
    if kind == "border":
        t = np.arange(T)[None, :]
        odd = (np.arange(B) & 1)[:, None] == 1
        to0 = np.maximum(c0 - 3 * (t + 1), 0)
        ton = np.minimum(c0 + 1 + 3 * (t + 1), n)
        stay = np.where(odd, 5, 0)
        after0 = np.clip(t - ((c0 + 2) // 3 - 1 + stay), 0, 4)
        aftern = np.clip(t - ((n - c0 - 1 + 2) // 3 - 1 + stay), 0, 4)
        m0 = to0 + np.where(odd, -after0, 3 * after0)
        mn = ton + np.where(odd, aftern, -3 * aftern)
        m = np.where(aim[:, None] == 0, m0, np.where(aim[:, None] == 1, mn, m))
    return m


def build_scene(origin=(0.0, 0.0), resolution=0.05, size=(200, 200), B=4096, T=64, phase=0.0, walk="local",
                border=None, track_unknown=False, near_goal=False, holonomic=True, seed=7, classes=None,
                label=""):
    """One edge scene.  origin, resolution, size = (W, H): the costmap; phase: metres added to the
    (2^-20-quantised) pose, it moves which float neighbour of each edge is hit; walk: "local",
    "far" or "border"; border: which map borders a border walk aims at, any of "x0", "x1", "y0",
    "y1" (default all four).
    Half of the rollouts keep y on cell centres (x alone lands on edges); the other half aim both
    axes at edges (cell corners).  A non-holonomic scene holds vy at 0: x edges only."""
    W, H = size
    res = float(resolution)
    ox, oy = float(origin[0]), float(origin[1])
    rng = np.random.Generator(np.random.PCG64(seed))
    if classes is None:
        classes = CLASSES_NEAR_GOAL if near_goal else CLASSES
    cells = checkerboard(W, H, classes)
    cx0, cy0 = W // 2, H // 2
    pose_x = float(_quantise(ox + (cx0 + 0.5) * res)) + phase
    pose_y = float(_quantise(oy + (cy0 + 0.5) * res)) + phase

    aim_x = np.full(B, -1)
    aim_y = np.full(B, -1)
    if walk == "border":
        sides = tuple(border) if border else ("x0", "x1", "y0", "y1")
        # each rollout aims at one border, every fourth one at a corner of the map as well
        pick = rng.integers(0, len(sides), size=B)
        for k, s in enumerate(sides):
            sel = pick == k
            (aim_x if s[0] == "x" else aim_y)[sel] = int(s[1])
        corner = (np.arange(B) % 4) == 3
        xs = [int(s[1]) for s in sides if s[0] == "x"]
        ys = [int(s[1]) for s in sides if s[0] == "y"]
        if xs and ys:
            need_x, need_y = corner & (aim_x < 0), corner & (aim_y < 0)
            aim_x[need_x] = rng.choice(np.array(xs), size=int(need_x.sum()))
            aim_y[need_y] = rng.choice(np.array(ys), size=int(need_y.sum()))
    reach = min(150, int(7.5 / res))
    mx = _walk(rng, walk, B, T, W, cx0, aim_x, reach)
    my = _walk(rng, walk, B, T, H, cy0, aim_y, reach)
    # the dither: one quantum, or one float ulp of the map's coordinates where that is coarser (a
    # power of two, so still on the 2^-20 grid): the float nearest the edge and its two neighbours
    du_x = max(QUANTUM, float(np.spacing(np.float32(max(abs(ox), abs(ox + W * res))))))
    du_y = max(QUANTUM, float(np.spacing(np.float32(max(abs(oy), abs(oy + H * res))))))
    jx = rng.choice(np.array([-1, 0, 0, 1]), size=(B, T))
    jy = rng.choice(np.array([-1, 0, 0, 1]), size=(B, T))
    ax = _quantise(ox + mx * res - pose_x) + jx * du_x
    # y: edges for the second half of the batch (and wherever a border is aimed at), else centres
    y_edges = (np.arange(B) >= B // 2) | (aim_y >= 0)
    ay = np.where(y_edges[:, None], _quantise(oy + my * res - pose_y) + jy * du_y,
                  _quantise(oy + (np.minimum(my, H - 1) + 0.5) * res - pose_y))
    if not holonomic:
        ay = np.zeros_like(ay)
    ax[:, 0] = 0.0       # trajectory point 0 is the pose: state.vx[0] is the robot's own speed, 0
    ay[:, 0] = 0.0
    assert max(np.abs(ax).max(), np.abs(ay).max()) < MAX_DISPLACEMENT, "walk leaves the exact range"

    def noise_of(a):
        n = np.zeros((B, T), np.float64)
        n[:, :-1] = np.diff(a, axis=1) / MODEL_DT       # control t moves the point t + 1
        return n
    n64 = (noise_of(ax), noise_of(ay))
    nvx, nvy = (n.astype(np.float32) for n in n64)
    exact = all(np.array_equal(n32.astype(np.float64), n) for n32, n in zip((nvx, nvy), n64))
    x = (pose_x + ax).astype(np.float32)
    y = (pose_y + ay).astype(np.float32)

    P = 9 if near_goal else int(min(60, (W - cx0 - 2) * res / 0.05))
    path_x = (pose_x + 0.05 * np.arange(P)).astype(np.float32)      # (near the goal: 0.4 m to it)
    path_y = np.full(P, pose_y, np.float32)
    path_yaw = np.zeros(P, np.float32)
    if near_goal:
        path_yaw[-1] = 0.7
    tick = Tick(pose_x=pose_x, pose_y=pose_y, pose_yaw=0.0, speed=(0.0, 0.0, 0.0), path_x=path_x,
                path_y=path_y, path_yaw=path_yaw, goal_x=float(path_x[-1]), goal_y=float(path_y[-1]))
    return EdgeScene(cells=cells, origin_x=ox, origin_y=oy, resolution=res, track_unknown=track_unknown,
                     near_goal=near_goal, holonomic=holonomic, B=B, T=T, tick=tick,
                     u0=np.zeros((3, T), np.float32), noise=(nvx, nvy, np.zeros((B, T), np.float32)),
                     ax=ax, ay=ay, x=x, y=y, classes=tuple(classes), label=label,
                     extra={"noise_exact": exact, "walk": walk, "phase": phase})


# ---- the judge: float64 / NumPy ----------------------------------------------------------------

def _class_terms(scn, critics, critic, consider_footprint=False, using_footprint=False):
    """Per cost value 0..255: (collides, what a lookup adds to the critical sum, to the repulsive
    sum), in float64 from the float32 parameters.  ObstaclesCritic: obstacles_critic.cpp:99-171;
    CostCritic: cost_critic.cpp:108-155.  consider_footprint: the critic's switch, under which 253
    is no collision (inCollision); using_footprint: the cost is a walked footprint cost, whose
    distance takes no inscribed-radius offset (obstacles_critic.cpp:106-108)."""
    c = np.arange(256, dtype=np.float64)
    collide = (c == 254) | ((c == 253) & (not consider_footprint)) | ((c == 255) & (not scn.track_unknown))
    crit = np.zeros(256)
    rep = np.zeros(256)
    if critic == "obstacles":
        p = critics.obstacles
        k, r_in, R = (float(np.float32(v)) for v in (scn.cost_scaling_factor, scn.inscribed_radius, scn.inflation_radius))
        margin = float(np.float32(p.collision_margin_distance))
        with np.errstate(divide="ignore"):
            d = (k * r_in - np.log(c) + np.log(253.0)) / k - (0.0 if using_footprint else r_in)
        live = c >= 1
        crit[live & (d < margin)] = (margin - d)[live & (d < margin)]
        if not scn.near_goal:
            rep[live & ~(d < margin)] = (R - d)[live & ~(d < margin)]
    else:
        p = critics.cost
        rep[c >= 253] = float(np.float32(p.critical_cost))
        if not scn.near_goal:
            rep[(c >= 1) & (c < 253)] = c[(c >= 1) & (c < 253)]
    return collide, crit, rep


def _weights(critics, critic, T):
    """(weight of the critical sum, weight of the repulsive sum, cost of a collision)."""
    if critic == "obstacles":
        p = critics.obstacles
        cw, rw = float(np.float32(p.critical_weight)), float(np.float32(p.repulsion_weight)) / T
        return cw, rw, cw * float(np.float32(p.collision_cost))
    p = critics.cost
    w = float(np.float32(p.cost_weight) / np.float32(254.0)) / T
    return 0.0, w, w * float(np.float32(p.collision_cost))


def _rollout_costs(hit, crit_t, rep_t, critics, critic, T):
    """A critic's loop over one rollout's poses, for all rollouts: hit / crit_t / rep_t [B, T] are
    each pose's collision and its two terms; the loop breaks at the first collision.
    Returns (costs [B] float64, collided [B], first colliding step [B], T where none)."""
    collided = hit.any(axis=1)
    first = np.where(collided, hit.argmax(axis=1), T)
    before = np.arange(T)[None, :] < first[:, None]           # lookups scored before the break
    crit = np.where(before, crit_t, 0.0).sum(axis=1)
    rep = np.where(before, rep_t, 0.0).sum(axis=1)
    cw, rw, collision = _weights(critics, critic, T)
    if critic == "obstacles":
        costs = np.where(collided, collision, cw * crit) + rw * rep
    else:
        costs = np.where(collided, collision, rw * rep)
    return costs, collided, first


def trajectories(scn):
    """integrateStateVelocities on the scene's stored noise: float32 cumsum of v dt, then
    x = float32(pose + float64(acc)).  Nothing of the builder's intent is read."""
    out = []
    for axis, pose in ((0, scn.tick.pose_x), (1, scn.tick.pose_y)):
        v = np.zeros((scn.B, scn.T), np.float32)      # v[:, 0]: the robot's own speed, 0
        if axis == 0 or scn.holonomic:                # (a non-holonomic model never writes vy)
            v[:, 1:] = scn.noise[axis][:, :-1]
        acc = np.cumsum(v * np.float32(MODEL_DT), axis=1, dtype=np.float32)
        out.append((pose + acc.astype(np.float64)).astype(np.float32))
    return out


def lookups(scn, x, y):
    """Costmap2D::worldToMap restated (the w < origin reject, truncation, the m < n reject) and
    getCost; off the map: NO_INFORMATION.  Returns (cost [B, T] int, on_map, qx, qy)."""
    wx, wy = x.astype(np.float64), y.astype(np.float64)
    H, W = scn.cells.shape
    qx = (wx - scn.origin_x) / scn.resolution
    qy = (wy - scn.origin_y) / scn.resolution
    ok = ~((wx < scn.origin_x) | (wy < scn.origin_y))
    mx = np.where(ok, qx, 0.0).astype(np.int64)
    my = np.where(ok, qy, 0.0).astype(np.int64)
    ok &= (mx < W) & (my < H)
    cost = np.where(ok, scn.cells[np.where(ok, my, 0), np.where(ok, mx, 0)], 255).astype(np.int64)
    return cost, ok, qx, qy


def model(scn, critics, critic="obstacles"):
    """The judge: per-rollout cost of ObstaclesCritic (or CostCritic) alone, in float64.
    Returns dict(x, y, costs, collided [B], reached [B, T], non_colliding, fail_flag)."""
    x, y = trajectories(scn)
    cost, _, _, _ = lookups(scn, x, y)
    collide_c, crit_c, rep_c = _class_terms(scn, critics, critic)
    costs, collided, first = _rollout_costs(collide_c[cost], crit_c[cost], rep_c[cost], critics, critic, scn.T)
    reached = np.arange(scn.T)[None, :] <= first[:, None]
    return dict(x=x, y=y, costs=costs, collided=collided, reached=reached,
                non_colliding=int((~collided).sum()), fail_flag=int(collided.all()))


def min_single_lookup_shift(critics, T, scn, critic="obstacles"):
    """The least a rollout's cost moves when ONE lookup reads another of the scene's cost classes
    (or NO_INFORMATION where the scene can leave the map and that is no collision), from the
    class table."""
    collide_c, crit_c, rep_c = _class_terms(scn, critics, critic)
    cw, rw, _ = _weights(critics, critic, T)
    values = list(scn.classes) + ([255] if scn.track_unknown else [])
    assert not any(collide_c[v] for v in values)
    per = sorted(cw * crit_c[v] + rw * rep_c[v] for v in values)
    shift = min(b - a for a, b in zip(per, per[1:]))
    assert shift > 0.0, "two cost classes of the scene score alike"
    return shift


def edge_stats(scn, x, y, reached):
    """How adversarial the scene is, over the lookups the critic makes (up to a rollout's first
    collision): per axis, lookups within one float ulp below / above a cell edge and exactly on
    one (q integral in float64); lookups within 1e-3 cell of each map border, per side."""
    H, W = scn.cells.shape
    st = {}
    for ax_name, v, o, n in (("x", x, scn.origin_x, W), ("y", y, scn.origin_y, H)):
        q = (v.astype(np.float64) - o) / scn.resolution
        dist = q - np.rint(q)
        ulp = np.spacing(np.abs(v)).astype(np.float64) / scn.resolution
        st[ax_name + "_below"] = int(np.sum(reached & (dist < 0) & (dist >= -ulp)))
        st[ax_name + "_above"] = int(np.sum(reached & (dist > 0) & (dist <= ulp)))
        st[ax_name + "_exact"] = int(np.sum(reached & (dist == 0)))
        w = v.astype(np.float64)
        for side, edge in (("0", o), ("1", o + n * scn.resolution)):
            near = reached & (np.abs(w - edge) <= 1e-3 * scn.resolution)
            st[f"{ax_name}{side}_outside"] = int(np.sum(near & ((w < edge) if side == "0" else (w >= edge))))
            st[f"{ax_name}{side}_inside"] = int(np.sum(near & ((w >= edge) if side == "0" else (w < edge))))
    return st


# ---- the scenes and the kernel forms that score them ------------------------------------------
# One table for both test files: tests/test_cell_index_cpu.py checks every scene named here on the
# oracle alone, tests/test_gpu_cell_index.py runs every (form, scene) pair on the GPU.

MAPS = {   # origin, resolution
    "o0": ((0.0, 0.0), 0.05),
    "o1": ((-3.7, 12.25), 0.03),
    "o2": ((-512.35, 1031.7), 0.1),          # a Nav2 map hundreds of metres from the frame origin
    "o3": ((100.1, -77.3), 0.025),
    "o4": ((-4.975, -4.975), 0.05),          # the map centred on the frame origin: x changes sign
}
# two pose phases per map (metres, on top of the quantised pose).  Where the coordinates are small
# a float ulp is a fraction of the 2^-20 quantum, and the phase decides how many points come within
# an ulp of their edge, on which side: chosen so that every scene meets the conditions of
# tests/test_cell_index_cpu.py (they are asserted there, for every scene, not assumed).
PHASES = {
    "o0": (0.0, 1.3e-7),
    "o1": (-0.2 * QUANTUM, 0.3 * QUANTUM),
    "o2": (0.0, 1.3e-7),                     # (far below an ulp of these coordinates: the same floats)
    "o3": (0.0, 1.3e-7),
    "o4": (-0.2 * QUANTUM, 0.2 * QUANTUM),
}
SIZES = {"local": (200, 200), "far": (400, 400), "border": (120, 110)}


def scene_key(m, phase=0, walk="local", tu=False, B=4096, T=64, size=None, near_goal=False, holonomic=True):
    return (m, phase, walk, bool(tu), B, T, tuple(size or SIZES[walk]), near_goal, holonomic)


def scene_name(key):
    m, phase, walk, tu, B, T, size, near_goal, holonomic = key
    return (f"{m}-p{phase}-{walk}{'-unknown' if tu else ''}-{size[0]}x{size[1]}-{B}x{T}"
            f"{'-near-goal' if near_goal else ''}{'' if holonomic else '-diff'}")


_scene_cache = {}


def scene(key):
    """The scene of a key (the last few are kept: several forms score the same scene)."""
    if key not in _scene_cache:
        while len(_scene_cache) >= 3:
            _scene_cache.pop(next(iter(_scene_cache)))
        m, phase, walk, tu, B, T, size, near_goal, holonomic = key
        origin, res = MAPS[m]
        _scene_cache[key] = build_scene(origin, res, size, B, T, PHASES[m][phase], walk, track_unknown=tu,
                                        near_goal=near_goal, holonomic=holonomic, label=scene_name(key))
    return _scene_cache[key]


def primary_scenes(B, T):
    """Every map at both phases on a local walk; the far walk where |a| < 8 m allows it; the
    border walk with the map's outside a collision and with it NO_INFORMATION at cost 255; a
    2000 x 2000 map; a map of odd width and height."""
    keys = [scene_key(m, ph, B=B, T=T) for m in MAPS for ph in (0, 1)]
    keys += [scene_key(m, 0, "far", B=B, T=T) for m in MAPS if MAPS[m][1] <= 0.05]
    keys += [scene_key(m, 0, "border", tu, B=B, T=T) for m in MAPS for tu in (False, True)]
    keys += [scene_key("o0", 1, B=B, T=T, size=(2000, 2000)), scene_key("o1", 0, B=B, T=T, size=(183, 197)),
             scene_key("o3", 1, "border", True, B=B, T=T, size=(183, 197))]
    return keys


def subset_scenes(B, T):
    """The large origin on a local walk, a far walk, a border walk each way.  From 100 steps on
    both border walks have the map's outside a collision: with it at cost 255 a rollout's cost
    passes 128 there, and the oracle's own float32 sums are then further from the float64 model
    than a tenth of the tolerance (tests/test_gpu_cell_index.py asserts that relation)."""
    return [scene_key("o2", 0, B=B, T=T), scene_key("o3", 0, "far", B=B, T=T),
            scene_key("o2", 0, "border", T < 100, B=B, T=T), scene_key("o1", 0, "border", False, B=B, T=T)]


WAVE, LANE = A.SMPC_FLAG_WAVE_PER_ROLLOUT, A.SMPC_FLAG_LANE_PER_ROLLOUT
STORE = A.SMPC_FLAG_STORE_TRAJECTORIES
FIVE = H.FIVE


@dataclass
class Form:
    """One kernel family and form: the tick shape, flags and knobs that select it, the critics
    scored, pass_kind and the instance's name as smpc_debug_last_pass_kernel() spells it (the
    spelling of tests/test_gpu_pass_selection.py), and the scenes it is run on."""
    B: int
    T: int
    flags: int
    env: dict
    critics: tuple
    kind: int
    kernel: str
    scenes: list
    critic: str = "obstacles"        # the critic the float64 model restates


_T, _F = True, False
FORMS = {
    # wave per rollout
    "wave-64": Form(4096, 64, WAVE, {}, ("obstacles",), 0, wave(1, 0, _T), primary_scenes(4096, 64)),
    "wave-30": Form(4096, 30, WAVE, {}, ("obstacles",), 0, wave(1, 0, _F), subset_scenes(4096, 30)),
    "wave-100": Form(4096, 100, WAVE, {}, ("obstacles",), 0, wave(2, 0, _F), subset_scenes(4096, 100)),
    "wave-64-cost": Form(4096, 64, WAVE, {}, ("cost",), 0, wave(1, 3, _T), subset_scenes(4096, 64), "cost"),
    # (trajectory write-out: the general pass; its trajectories are compared bit for bit)
    "wave-64-store": Form(4096, 64, WAVE | STORE, {}, ("obstacles",), 0, wave(1, 2, _T), subset_scenes(4096, 64)),
    # lane per rollout: parking form, whole and ragged horizon; re-read form; a partial last wave
    "lane-64": Form(4096, 64, LANE, {}, ("obstacles",), 1, lane(),
                    primary_scenes(4096, 64)),
    "lane-56": Form(4096, 56, LANE, {}, ("obstacles",), 1, lane(56),
                    subset_scenes(4096, 56)),
    "lane-rr-128": Form(4096, 128, LANE, {}, ("obstacles",), 1, lane(128),
                        subset_scenes(4096, 128)),
    "lane-rr-64": Form(4096, 64, LANE, {"SMPC_LANE_REREAD": "1"}, ("obstacles",), 1,
                       lane(rr=True), subset_scenes(4096, 64)),
    "lane-64-70001": Form(70001, 64, LANE, {}, ("obstacles",), 1, lane(),
                          [scene_key("o2", 0, "border", True, B=70001)]),
    # a near-goal tick: the GoalAngle instance, ObstaclesCritic's repulsive term off.  The default
    # five critics (GoalAngle must be on; the other three are gated off by the distance to the goal)
    "lane-64-near-goal": Form(4096, 64, LANE, {}, FIVE, 1, lane(ga=True),
                              [scene_key("o2", 0, near_goal=True), scene_key("o0", 1, "far", near_goal=True),
                               scene_key("o1", 0, "border", True, near_goal=True)]),
    # split horizon
    "split-4-16384": Form(16384, 64, 0, {"SMPC_PASS": "split"}, ("obstacles",), 2, "smpc_pass_split<4, true>",
                          primary_scenes(16384, 64)),
    "split-4-32768": Form(32768, 64, 0, {"SMPC_PASS": "split"}, ("obstacles",), 2, "smpc_pass_split<4, true>",
                          [scene_key("o2", 0, B=32768), scene_key("o3", 0, "far", B=32768)]),
    "split-2-16384": Form(16384, 64, 0, {"SMPC_PASS": "split", "SMPC_SPLIT_NSEG": "2"}, ("obstacles",), 2,
                          "smpc_pass_split<2, true>", subset_scenes(16384, 64)),
    "split-4-48": Form(16384, 48, 0, {"SMPC_PASS": "split"}, ("obstacles",), 2, "smpc_pass_split<4, false>",
                       subset_scenes(16384, 48)),
    # a non-holonomic model: vy held at 0, x edges only
    "lane-64-diff": Form(4096, 64, LANE, {}, ("obstacles",), 1, lane(),
                         [scene_key("o2", 0, holonomic=False), scene_key("o1", 1, holonomic=False)]),
}
# the grouped launch's instance (smpc_group_optimize), two members on different origins
GROUP_KERNEL = lane(many=True)
GROUP_SCENES = [scene_key("o2", 0), scene_key("o3", 1, "border", True)]
# the standard parity bar (tests/helpers.assert_parity) with a zero flip budget: the default five
PARITY_SCENES = [scene_key("o2", 0), scene_key("o4", 1, "far")]


def all_scene_keys():
    keys = []
    for f in FORMS.values():
        keys += f.scenes
    keys += GROUP_SCENES + PARITY_SCENES
    return sorted(set(keys), key=scene_name)
