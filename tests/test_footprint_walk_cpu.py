"""The premises of tests/test_gpu_footprint_walk.py, pinned on the oracle and the judge alone (no GPU).

For every scene of tests/footprint_walk_scenes.py: the stored noise is exact in float32 and on its
grids, the oracle's trajectories equal the designed x, y and yaw bit for bit, the oracle and the
judge (tests/footprint_walk_model.py) agree on fail_flag, non_colliding and on who collides, for
ObstaclesCritic alone, CostCritic alone and both together, every non-colliding rollout's cost is
within tol, and tol stands ten times clear of the oracle's own distance from the judge.  And the
scenes ARE adversarial: every vertex is at least 1e-9 m from every cell edge, each family holds
its stated number of poses of its kind, neither all rollouts nor none collide, and every mutant
of the judge that can be told from it is told from it by at least 8 rollouts of some scene.
These are conditions, not measurements: a scene that misses one gets other stations
(footprint_walk_scenes.SCENES), the condition stays."""
import numpy as np
import pytest

from tests import footprint_walk_model as M
from tests import footprint_walk_scenes as S

MIN_EDGES = 200           # outline edges of each kind that family (a) sweeps: per octant, ties, h, v
MIN_POSES = 200           # poses of a family's kind
MIN_ENDING = 40           # poses of a kind that ends a rollout (at most one per rollout)
MIN_ROLLOUTS = 8          # rollouts a mutant must move
OCTANTS = tuple(f"{a}{b}{c}" for a in "xy" for b in "+-" for c in "+-")
# The tie mutant cannot be told from the judge by any costmap: with dx == dy both branches set
# den = numadd, so num >= den holds at every cell and both axes step at every cell either way.
EQUIVALENT = ("tie_y",)


def tolerance(scn, critic):
    cr = S.critics_of((critic,), (critic,))
    return 0.25 * M.single_pose_shift(scn, cr, critic), cr


@pytest.mark.parametrize("name", list(S.SCENES))
def test_oracle_poses_are_the_designed_ones(oracle_lib, name):
    scn = S.scene(name)
    assert scn.extra["noise_exact"], "a noise increment is not a float32"
    assert scn.unit_noise == (True, True, True), "noise off its grid: 2^-16 m/s, 2^-8 rad/s"
    x, y, yaw = M.poses(scn)
    assert np.array_equal(x, scn.x) and np.array_equal(y, scn.y) and np.array_equal(yaw, scn.yaw)
    r = S.oracle_run(name, "obstacles")
    assert np.array_equal(r["x"], scn.x) and np.array_equal(r["y"], scn.y) and np.array_equal(r["yaw"], scn.yaw)
    # travel only at yaw 0, spin only on the spot
    moved = (np.diff(scn.x, axis=1) != 0) | (np.diff(scn.y, axis=1) != 0)
    assert not np.any(moved & ((scn.yaw[:, 1:] != 0) | (scn.yaw[:, :-1] != 0)))


@pytest.mark.parametrize("config", list(S.CONFIGS))
@pytest.mark.parametrize("name", list(S.SCENES))
def test_oracle_equals_the_judge(oracle_lib, name, config):
    scn = S.scene(name)
    r = S.oracle_run(name, config)
    names, fp = S.CONFIGS[config]
    for critic in names:
        tol, _ = tolerance(scn, critic)
        cr = S.critics_of(names, fp)
        m = M.model(scn, cr, critic)
        row = r[critic]["costs"].astype(np.float64)
        d = np.abs(row - m["costs"])
        keep = ~m["collided"]
        worst = d[keep].max(initial=0.0)
        _, _, collision = M.E._weights(cr, critic, scn.T)
        print(f"[walk-cpu] {name} {config}/{critic}: oracle vs judge {worst:.2e} (tol {tol:.2e}), "
              f"colliding {int(m['collided'].sum())} of {scn.B}")
        assert np.array_equal(row > 0.5 * collision, m["collided"]), "another set of rollouts collides"
        if critic in fp:
            assert np.all(d[keep] <= tol)
            assert tol > 10.0 * worst, f"tol {tol:.3e} against oracle-vs-judge {worst:.3e}"
        else:
            # (the other critic in point mode: centre costs only, sums in the hundreds; the float32
            # error of such a sum, not a footprint tolerance)
            assert np.all(d[keep] <= S.float_sum_error(scn.T, m["costs"][keep]))
        assert np.all(d[~keep] <= tol + 2.0 ** -22 * m["costs"][~keep])
        assert r[critic]["fail"] == m["fail_flag"]
    if len(names) == 2:
        j = M.both(scn, S.critics_of(names, fp))
        assert np.all(np.abs(r["costs"] - j["costs"]) <= S.float_sum_error(scn.T, j["costs"]))
    else:
        j = M.model(scn, S.critics_of(names, fp), config)
        assert np.array_equal(r["costs"], r[config]["costs"])       # one critic: the tick's cost is its row
    assert (r["out"].fail_flag, r["out"].non_colliding) == (j["fail_flag"], j["non_colliding"])


@pytest.mark.parametrize("name", list(S.SCENES))
def test_scene_conditions(name):
    scn = S.scene(name)
    fam = scn.family
    ms = {c: M.model(scn, S.critics_of((c,), (c,)), c) for c in ("obstacles", "cost")}
    st = S.counts(scn, ms["obstacles"])
    print(f"[walk-cpu] {name}: {st}")
    assert st["margin"] >= S.MARGIN
    for m in ms.values():
        assert (0 < m["non_colliding"] < scn.B) if fam != "h" else (m["fail_flag"] == 1 and np.all(m["first"] == 0))
    pic = M.circumscribed_cost(scn)
    assert st["walked"] >= MIN_POSES or fam == "h"
    if fam == "a" and scn.label.split("-")[1] in ("rectangle", "triangle", "sixteen"):
        for k in OCTANTS + ("tie", "h", "v"):
            assert st[k] >= MIN_EDGES, k
    if scn.label.startswith("a-speck"):
        assert st["point"] >= MIN_EDGES          # every line has dx = dy = 0
    if scn.label.startswith("a-segment"):
        assert len(scn.footprint) == 2
    if scn.label.startswith("a-sixteen"):
        assert len(scn.footprint) == 16
    if fam == "b":
        if pic >= 1:
            assert min(st["below"], st["at"], st["above"]) >= MIN_POSES
            assert min(st["below_lethal"], st["at_lethal"], st["above_lethal"]) >= MIN_ENDING // 2
        else:
            # the walk is entered at every pose ObstaclesCritic scores, free space too
            assert st["walked"] == int((np.arange(scn.T)[None, :] <= ms["obstacles"]["first"][:, None]).sum())
            assert int((ms["obstacles"]["entered"] & (ms["obstacles"]["centre"] == 0)).sum()) >= MIN_POSES
    if fam == "c":
        assert st["vertex_off"] >= MIN_ENDING and st["centre_off"] >= MIN_ENDING
        if scn.track_unknown:
            assert int((ms["obstacles"]["collided"] != ms["cost"]["collided"]).sum()) >= MIN_ROLLOUTS
    if fam == "d":
        assert st["walked_255"] >= MIN_ENDING
    if fam == "e":
        assert st["straddle"] >= MIN_POSES and st["beyond"] >= MIN_POSES
    if fam in "fg":
        assert st["at_lethal"] + st["above_lethal"] >= MIN_ENDING
    if fam == "g":
        assert scn.near_goal


def _moved(name, critic, mutant):
    scn = S.scene(name)
    tol, cr = tolerance(scn, critic)
    a, b = M.model(scn, cr, critic), M.model(scn, cr, critic, mutant)
    return int(np.sum((a["collided"] != b["collided"]) | (~a["collided"] & (np.abs(a["costs"] - b["costs"]) > tol))))


def test_every_mutant_is_told_from_the_judge():
    table = {mu: {n: max(_moved(n, c, mu) for c in ("obstacles", "cost")) for n in S.SCENES} for mu in M.MUTANTS}
    for mu, row in table.items():
        print(f"[walk-cpu] mutant {mu}: rollouts moved per scene {row}")
    for mu in M.MUTANTS:
        best = max(table[mu].values())
        if mu in EQUIVALENT:
            assert best == 0
        else:
            assert best >= MIN_ROLLOUTS, mu
    for fam in S.FAMILIES:
        hit = max(table[mu][n] for mu in M.MUTANTS for n in S.SCENES if S.SCENES[n][0] == fam)
        assert hit >= MIN_ROLLOUTS, f"no mutant moves family {fam}"


def test_the_tie_mutant_walks_the_same_cells():
    """Exhaustively for deltas up to 24 cells in the four diagonal directions: the cells read, in
    order, are the same whichever branch a tie takes."""
    cells = np.zeros((64, 64), np.uint8)
    for d in range(25):
        for sx in (1, -1):
            for sy in (1, -1):
                recs = []
                for mu in (None, "tie_y"):
                    rec = []
                    a = np.array([32]), np.array([32]), np.array([32 + sx * d]), np.array([32 + sy * d])
                    M._line(cells, a[0], a[1], a[2], a[3], np.array([True]), mu, rec)
                    recs.append(M.cells_read(rec, 0))
                assert recs[0] == recs[1] and len(recs[0]) == d + 1


def test_the_line_against_a_scalar_restatement():
    """The vectorised walk against the definition written out for one line at a time."""
    def line(x0, y0, x1, y1):
        dx, dy = abs(x1 - x0), abs(y1 - y0)
        sx, sy = (1 if x1 >= x0 else -1), (1 if y1 >= y0 else -1)
        out, x, y = [], x0, y0
        den, numadd = (dx, dy) if dx >= dy else (dy, dx)
        num = den // 2
        for _ in range(den + 1):
            out.append((x, y))
            num += numadd
            minor = num >= den
            if minor:
                num -= den
            if dx >= dy:
                x, y = x + sx, y + (sy if minor else 0)
            else:
                x, y = x + (sx if minor else 0), y + sy
        return out
    rng = np.random.Generator(np.random.PCG64(5))
    cells = np.zeros((64, 64), np.uint8)
    ends = rng.integers(8, 56, size=(500, 4))
    rec = []
    M._line(cells, ends[:, 0], ends[:, 1], ends[:, 2], ends[:, 3], np.ones(500, bool), None, rec)
    for k in range(500):
        assert M.cells_read(rec, k) == line(*(int(v) for v in (ends[k, 0], ends[k, 1], ends[k, 2], ends[k, 3])))
        assert M.cells_read(rec, k)[-1] == (int(ends[k, 2]), int(ends[k, 3]))
