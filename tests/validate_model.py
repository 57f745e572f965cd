"""The trajectory validator's definition (include/smpc.h: smpc_validate_trajectory) in NumPy, built
from the parts the suite already judges with:

  poses    tests/moving_model.py::integrate — the control sequence itself integrated from the pose;
  n        min(T, (uint32)floorf(collision_lookahead_time / model_dt)), the quotient in float32;
  costmap  CostCritic's rule per pose t < n: the centre cost by tests/edge_scenes.py::lookups (off
           the map 255), below 1 free; with consider_footprint, where it reaches the
           possibly-inscribed cost (footprint_walk_model.circumscribed_cost) or that cost is < 1, it
           becomes footprint_walk_model.walk at the pose; 254 collides, 253 unless consider_footprint,
           255 unless the costmap tracks unknown;
  discs    the disc rule of moving_model.costs: float32 d = sqrt(dx dx + dy dy) < radius[k];
  result   valid, checked = n, first_bad the least colliding t, cause (1 costmap, 2 disc; the costmap
           wins), cost (the costmap cost above at first_bad), disc (the least k hit at first_bad).

`scn` is any scene with cells, origin_x, origin_y, resolution, track_unknown and, for a footprint,
footprint, circumscribed, layer_scaling, inscribed_radius (tests/footprint_walk_scenes.py's).
verdict() judges given poses (the GPU tests hand it the poses the call returned); validate() makes
the poses itself."""
from types import SimpleNamespace

import numpy as np

from tests import edge_scenes as E
from tests import footprint_walk_model as W
from tests import moving_model as MM

CAUSE_COSTMAP, CAUSE_DISC = 1, 2


def checked(lookahead, model_dt, T):
    """n: the quotient and its floor in float32, as upstream forms it (2.0f / 0.05f is 40)."""
    q = np.floor(np.float32(lookahead) / np.float32(model_dt))
    assert q.dtype == np.float32
    return int(min(np.float32(T), max(q, np.float32(0))))


def costmap_costs(scn, xyyaw, consider_footprint):
    """c of every pose [T] (int64) and whether it collides [T]."""
    x, y, yaw = (np.ascontiguousarray(xyyaw[:, k], np.float32) for k in range(3))
    centre, _, _, _ = E.lookups(scn, x, y)
    c = centre.copy()
    if consider_footprint:
        pic = W.circumscribed_cost(scn)
        enter = (centre >= 1) & ((centre >= pic) | (pic < 1.0))
        if enter.any():
            c[enter] = W.walk(scn, x[enter], y[enter], yaw[enter])
    hit = (c == 254) | ((c == 253) & (not consider_footprint)) | ((c == 255) & (not scn.track_unknown))
    hit &= centre >= 1
    c[centre < 1] = 0
    return c, hit


def disc_hits(xyyaw, xy, radius):
    """hit [T, K], and the float32 distances d [T, K] they were decided on."""
    T = len(xyyaw)
    if xy is None or len(radius) == 0:
        return np.zeros((T, 0), bool), np.zeros((T, 0), np.float32)
    xy = np.asarray(xy, np.float32)
    radius = np.asarray(radius, np.float32)
    x = np.ascontiguousarray(xyyaw[:, 0], np.float32)[:, None]
    y = np.ascontiguousarray(xyyaw[:, 1], np.float32)[:, None]
    dx = x - xy[:, :, 0].T
    dy = y - xy[:, :, 1].T
    d = np.sqrt(dx * dx + dy * dy)
    assert d.dtype == np.float32
    return d < radius[None, :], d


def verdict(scn, xyyaw, n, consider_footprint=False, xy=None, radius=None):
    """The result for given poses float32 [T, 3].  xy [K, T, 2], radius [K]: the table in force
    (None: no discs, or moving_obstacles = 0).  Also `near`: some checked disc term lies within
    moving_model.NEAR of its radius (its hit may go either way on other poses)."""
    xyyaw = np.asarray(xyyaw, np.float32)
    c, map_hit = costmap_costs(scn, xyyaw, consider_footprint)
    hit, d = disc_hits(xyyaw, xy, radius)
    near = False
    if hit.shape[1]:
        r = np.asarray(radius, np.float64)[None, :]
        near = bool((np.abs(d[:n].astype(np.float64) - r) < MM.NEAR).any())
    bad_all = map_hit | hit.any(axis=1)          # every pose, checked or not: what the scenes' premises are stated on
    bad = bad_all.copy()
    bad[n:] = False
    if not bad.any():
        return SimpleNamespace(valid=1, checked=n, first_bad=0, cause=0, cost=0.0, disc=0, near=near, bad_all=bad_all)
    t = int(np.argmax(bad))
    cause = CAUSE_COSTMAP if map_hit[t] else CAUSE_DISC
    disc = int(np.argmax(hit[t])) if hit[t].any() else 0
    return SimpleNamespace(valid=0, checked=n, first_bad=t, cause=cause, cost=float(c[t]), disc=disc, near=near,
                           bad_all=bad_all)


def validate(scn, pose, u, model_dt, lookahead, consider_footprint=False, moving_obstacles=True, holonomic=True,
             xy=None, radius=None):
    """The definition end to end.  -> (verdict, poses float32 [T, 3])."""
    poses = MM.integrate(u, pose, model_dt, holonomic)
    n = checked(lookahead, model_dt, poses.shape[0])
    table = (xy, radius) if moving_obstacles else (None, None)
    return verdict(scn, poses, n, consider_footprint, *table), poses


def same(a, b):
    """Whether two results (a model's or a call's) agree in all six fields."""
    return all(getattr(a, f) == getattr(b, f) for f in ("valid", "checked", "first_bad", "cause", "disc")) and \
        float(a.cost) == float(b.cost)
