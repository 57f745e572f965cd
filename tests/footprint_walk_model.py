"""The judge of the footprint outline walk: NumPy and integers, written from the definition.

consider_footprint makes a collision critic walk the robot's outline over the costmap
(nav2_costmap_2d's footprintCostAtPose, lineCost and nav2_util's LineIterator) wherever the
centre cost reaches the possibly-inscribed cost.  This module restates that walk and the critics'
rules around it (obstacles_critic.cpp:114-224, cost_critic.cpp:62-201) for the scenes of
tests/footprint_walk_scenes.py, whose poses are known bit for bit:

  vertices  vertex i = pose + R(yaw) footprint[i] in float64; its cell by Costmap2D::worldToMap
            (edge_scenes.lookups); a vertex off the map makes the footprint cost 254 at once;
  edges     (v0 -> v1), ..., (v[n-2] -> v[n-1]), the walk returning as soon as the running maximum
            is 254; then the closing edge from the FIRST vertex to the LAST;
  line      dx = |x1 - x0|, dy = |y1 - y0|; x is the major axis iff dx >= dy; den = the major
            delta, num = den // 2, numadd = the minor delta; den + 1 cells are visited; after a
            cell is read num += numadd, and if num >= den then num -= den and the minor axis
            steps; then the major axis steps.  The cost is the running maximum of the cells read,
            a cell of 254 returns 254 immediately, a cell of 255 is just the largest value;
  critics   the walk is entered where centre >= fp_pic or fp_pic < 1; ObstaclesCritic enters it
            for an on-map centre only and scores the walked cost with no inscribed-radius offset;
            CostCritic enters it for every scored centre (>= 1, off the map too), scores the
            centre cost and takes only the collision from the walk; 253 is no collision under a
            footprint.  The point-mode terms are edge_scenes._class_terms / _weights.

MUTANTS are single changes of that definition, switchable: the CPU test proves that the scenes
tell each of them from the judge, which is what makes a pass on the GPU mean something."""
import numpy as np

from tests import edge_scenes as E

MUTANTS = (
    "num0",          # 1. num starts at 0
    "gt",            # 2. > for >= in the minor-axis test
    "tie_y",         # 3. the tie dx == dy takes the y-major branch
    "skip_end",      # 4. the end cell is skipped
    "close_rev",     # 5. the closing edge runs last -> first
    "round",         # 6. vertex index rounded to nearest
    "enter_gt",      # 7. the walk is entered on > instead of >= fp_pic
    "c253",          # 8. 253 collides under a footprint
    "centre_half",   # 9. the walked cost goes through the centre half of the table (offset applied)
)
WALK_MUTANTS = MUTANTS[:6]
LETHAL = 254


# ---- poses -----------------------------------------------------------------------------------------

def poses(scn):
    """integrateStateVelocities on the stored noise, in float32 as the reference sums it:
    yaw = cumsum(wz dt), dx = vx cos(yaw[t-1]) - vy sin(yaw[t-1]), x = float32(pose + float64(cumsum)).
    Nothing of the builder's intent is read.  -> x, y, yaw float32 [B, T]."""
    B, T = scn.B, scn.T
    dt = np.float32(E.MODEL_DT)
    v = [np.zeros((B, T), np.float32) for _ in range(3)]
    for k in range(3):
        v[k][:, 1:] = scn.noise[k][:, :-1]           # v[:, 0]: the robot's own speed, 0
    yaw = np.cumsum(v[2] * dt, axis=1, dtype=np.float32) + np.float32(scn.tick.pose_yaw)
    prev = np.concatenate([np.full((B, 1), np.float32(scn.tick.pose_yaw)), yaw[:, :-1]], axis=1)
    c, s = np.cos(prev), np.sin(prev)
    dx = v[0] * c - v[1] * s
    dy = v[0] * s + v[1] * c
    x = (scn.tick.pose_x + np.cumsum(dx * dt, axis=1, dtype=np.float32).astype(np.float64)).astype(np.float32)
    y = (scn.tick.pose_y + np.cumsum(dy * dt, axis=1, dtype=np.float32).astype(np.float64)).astype(np.float32)
    return x, y, yaw


# ---- the walk, over N poses at once -------------------------------------------------------------------

def vertices(scn, x, y, yaw):
    """World coordinates of every vertex, float64 [N, n]."""
    x, y, th = (np.asarray(a, np.float64).reshape(-1) for a in (x, y, yaw))
    fx, fy = scn.footprint[:, 0][None, :], scn.footprint[:, 1][None, :]
    c, s = np.cos(th)[:, None], np.sin(th)[:, None]
    return x[:, None] + (fx * c - fy * s), y[:, None] + (fx * s + fy * c)


def vertex_cells(scn, wx, wy, mutant=None):
    """worldToMap of every vertex: (mx, my int64 [N, n], on the map [N, n])."""
    H, W = scn.cells.shape
    ok = ~((wx < scn.origin_x) | (wy < scn.origin_y))
    qx = np.where(ok, (wx - scn.origin_x) / scn.resolution, 0.0)
    qy = np.where(ok, (wy - scn.origin_y) / scn.resolution, 0.0)
    if mutant == "round":
        qx, qy = qx + 0.5, qy + 0.5
    mx, my = qx.astype(np.int64), qy.astype(np.int64)
    ok &= (mx < W) & (my < H)
    return np.where(ok, mx, 0), np.where(ok, my, 0), ok


def edge_margin(scn, wx, wy):
    """Distance of every vertex to the nearest cell edge, metres [N, n]."""
    d = np.inf
    for w, o in ((wx, scn.origin_x), (wy, scn.origin_y)):
        q = (w - o) / scn.resolution
        d = np.minimum(d, np.abs(q - np.rint(q)) * scn.resolution)
    return d


def _line(cells, x0, y0, x1, y1, live, mutant, record):
    """One LineIterator walk per row.  live: rows that walk.  -> (running maximum, lethal met)."""
    dx, dy = np.abs(x1 - x0), np.abs(y1 - y0)
    xmaj = (dx > dy) if mutant == "tie_y" else (dx >= dy)
    den = np.where(xmaj, dx, dy)
    numadd = np.where(xmaj, dy, dx)
    num = np.zeros_like(den) if mutant == "num0" else den // 2
    sx, sy = np.where(x1 >= x0, 1, -1), np.where(y1 >= y0, 1, -1)
    visits = den if mutant == "skip_end" else den + 1
    x, y = x0.copy(), y0.copy()
    cost = np.zeros(len(x0), np.int64)
    lethal = np.zeros(len(x0), bool)
    for k in range(int(visits[live].max(initial=0))):
        on = live & ~lethal & (k < visits)
        c = np.where(on, cells[np.where(on, y, 0), np.where(on, x, 0)], 0).astype(np.int64)
        if record is not None:
            record.append((on.copy(), x.copy(), y.copy()))
        lethal |= on & (c == LETHAL)
        cost = np.maximum(cost, c)
        num = num + numadd
        step = (num > den) if mutant == "gt" else (num >= den)
        num = num - np.where(step, den, 0)
        x = x + np.where(xmaj, sx, np.where(step, sx, 0))
        y = y + np.where(xmaj, np.where(step, sy, 0), sy)
    return np.where(lethal, LETHAL, cost), lethal


def walk(scn, x, y, yaw, mutant=None, record=False):
    """footprintCostAtPose for N poses.  -> walked cost int64 [N]; with record also the cells read,
    a list of (row mask, mx, my) per step, in the order they are read."""
    wx, wy = vertices(scn, x, y, yaw)
    mx, my, ok = vertex_cells(scn, wx, wy, mutant)
    N, n = mx.shape
    rec = [] if record else None
    cost = np.zeros(N, np.int64)
    done = np.zeros(N, bool)                   # the cost is final: a vertex off the map, or 254 met
    off = ~ok[:, 0]
    cost[off], done = LETHAL, done | off
    for i in range(n - 1):
        off = ~done & ~ok[:, i + 1]
        cost[off], done = LETHAL, done | off
        c, lethal = _line(scn.cells, mx[:, i], my[:, i], mx[:, i + 1], my[:, i + 1], ~done, mutant, rec)
        cost = np.where(done, cost, np.maximum(cost, c))
        done |= lethal
    a, b = (n - 1, 0) if mutant == "close_rev" else (0, n - 1)
    c, _ = _line(scn.cells, mx[:, a], my[:, a], mx[:, b], my[:, b], ~done, mutant, rec)
    cost = np.where(done, cost, np.maximum(cost, c))
    return (cost, rec) if record else cost


def cells_read(rec, row):
    """The cells one pose's walk read, in order: [(mx, my)]."""
    return [(int(x[row]), int(y[row])) for on, x, y in rec if on[row]]


def edge_kinds(scn, x, y, yaw):
    """How many outline edges (the closing one too) of the given poses are of each kind: the eight
    octants "+x+y" (x-major, both rising) ... , "h" and "v" (a zero minor delta), "tie" (dx = dy >
    0) and "point" (dx = dy = 0)."""
    wx, wy = vertices(scn, x, y, yaw)
    mx, my, ok = vertex_cells(scn, wx, wy)
    n = mx.shape[1]
    pairs = [(i, i + 1) for i in range(n - 1)] + [(0, n - 1)]
    out = {}
    for a, b in pairs:
        good = ok[:, a] & ok[:, b]
        ex, ey = (mx[:, b] - mx[:, a])[good], (my[:, b] - my[:, a])[good]
        dx, dy = np.abs(ex), np.abs(ey)
        kinds = {"point": (dx == 0) & (dy == 0), "tie": (dx == dy) & (dx > 0),
                 "h": (dy == 0) & (dx > 0), "v": (dx == 0) & (dy > 0)}
        for major, m in (("x", dx > dy), ("y", dy > dx)):
            for sa, ma in (("+", ex > 0), ("-", ex < 0)):
                for sb, mb in (("+", ey > 0), ("-", ey < 0)):
                    kinds[f"{major}{sa}{sb}"] = m & ma & mb
        for k, m in kinds.items():
            out[k] = out.get(k, 0) + int(m.sum())
    return out


# ---- the critics ---------------------------------------------------------------------------------------

def circumscribed_cost(scn):
    """findCircumscribedCost with InflationLayer::computeCost: the possibly-inscribed cost fp_pic;
    -1 without a layer."""
    if scn.layer_scaling < 0.0:
        return -1.0
    r_in = float(np.float32(scn.inscribed_radius))
    distance = scn.circumscribed / scn.resolution
    if distance == 0:
        return 254.0
    if distance * scn.resolution <= r_in:
        return 253.0
    return float(int(252 * np.exp(-1.0 * scn.layer_scaling * (distance * scn.resolution - r_in))))


def unique_poses(x, y, yaw):
    """(x, y, yaw of the distinct poses, the index of every [B, T] pose among them)."""
    key = np.stack([a.astype(np.float32).view(np.uint32).astype(np.uint64).reshape(-1) for a in (x, y, yaw)], axis=1)
    _, first, inv = np.unique(key, axis=0, return_index=True, return_inverse=True)
    flat = [a.reshape(-1)[first] for a in (x, y, yaw)]
    return flat[0], flat[1], flat[2], inv.reshape(x.shape)


def model(scn, critics, critic, mutant=None):
    """One collision critic alone, in float64, with consider_footprint as its parameters say.
    -> dict(x, y, yaw, costs, collided, first, centre, entered, walked (-1 where the walk is not
    entered), non_colliding, fail_flag)."""
    x, y, yaw = poses(scn)
    centre, on_map, _, _ = E.lookups(scn, x, y)
    pic = circumscribed_cost(scn)
    fp = bool(getattr(critics, critic).consider_footprint)
    reach = (centre > pic) if mutant == "enter_gt" else (centre >= pic)
    entered = fp & (reach | (pic < 1.0)) & (on_map if critic == "obstacles" else centre >= 1)
    ux, uy, uyaw, inv = unique_poses(x, y, yaw)
    walked = np.where(entered, walk(scn, ux, uy, uyaw, mutant)[inv], -1)
    seen = np.where(entered, walked, centre)         # the cost the collision switch sees
    fp253 = fp and mutant != "c253"
    col_c, crit_c, rep_c = E._class_terms(scn, critics, critic, consider_footprint=fp253)
    if critic == "obstacles":
        _, crit_w, rep_w = E._class_terms(scn, critics, critic, consider_footprint=fp253,
                                          using_footprint=mutant != "centre_half")
        crit_t = np.where(entered, crit_w[seen], crit_c[seen])
        rep_t = np.where(entered, rep_w[seen], rep_c[seen])
    else:
        crit_t, rep_t = crit_c[centre], rep_c[centre]           # scored on the centre cost regardless
    costs, collided, first = E._rollout_costs(col_c[seen], crit_t, rep_t, critics, critic, scn.T)
    return dict(x=x, y=y, yaw=yaw, costs=costs, collided=collided, first=first, centre=centre, entered=entered,
                walked=walked, non_colliding=int((~collided).sum()), fail_flag=int(collided.all()))


def both(scn, critics, mutant=None):
    """Both collision critics in one list: each keeps its own first collision, the costs add, and
    the manager stops behind the first critic that finds every rollout colliding: CostCritic is
    scored first, ObstaclesCritic assigns fail_flag last (critic_manager.cpp:70-73)."""
    c, o = model(scn, critics, "cost", mutant), model(scn, critics, "obstacles", mutant)
    last = c if c["fail_flag"] else o
    total = c["costs"] if c["fail_flag"] else c["costs"] + o["costs"]
    return dict(cost=c, obstacles=o, costs=total, non_colliding=last["non_colliding"], fail_flag=last["fail_flag"])


def single_pose_shift(scn, critics, critic):
    """The least a rollout's cost moves when ONE pose's footprint cost is reclassified among the
    values a walk can return on the scene, from the class table (as
    edge_scenes.min_single_lookup_shift).  ObstaclesCritic scores a walked value through the table
    without the offset.  A walk is entered at a centre of fp_pic or more (where fp_pic >= 1) and
    stays inside the flat field round its station, so what it returns is a field class of fp_pic
    or more or an isolated cell's value: those are the values.  CostCritic takes only the
    collision from the walk, so there the least move is the collision itself, and the bound kept
    is the smaller of that and a centre lookup's shift among all classes.  Where no two values
    score apart (a near-goal tick has no repulsion, and no walked cost comes nearer than the
    margin), a collision is again the least move."""
    walked = critic == "obstacles"
    pic = circumscribed_cost(scn)
    fields = [v for v in scn.classes if not walked or pic < 1.0 or v >= pic]
    values = sorted(set(fields) | (set(scn.specials) - {LETHAL}))
    cw, rw, collision = E._weights(critics, critic, scn.T)
    col, crit, rep = E._class_terms(scn, critics, critic, consider_footprint=True, using_footprint=walked)
    per = sorted({float(cw * crit[v] + rw * rep[v]) for v in values if not col[v]})
    gaps = [b - a for a, b in zip(per, per[1:])]
    gaps.append(collision - max(per) * scn.T)        # (the dearest rollout that does not collide)
    shift = min(gaps)
    assert shift > 0.0
    return shift
