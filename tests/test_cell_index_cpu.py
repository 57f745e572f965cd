"""The premise of tests/test_gpu_cell_index.py, pinned on the oracle alone (no GPU).

For every scene of tests/edge_scenes.py that the GPU test scores: the stored noise is exact in
float32, the oracle's trajectories are bit-equal to the float64 model's (and to the points the
builder aimed at), its per-rollout costs are within float32 summation error of the model's, both
agree on who collides — and the scene IS adversarial: thousands of lookups within one float ulp
of a cell edge on either side, points exactly on an edge where the map's origin allows one, and
on a border walk hundreds of points on either side of each map border.  These are conditions, not
measurements: a scene that misses one gets another walk or phase (edge_scenes.PHASES), the
condition stays.
"""
import numpy as np
import pytest

from tests import edge_scenes as E

MIN_NEAR_EDGE = 2000      # lookups within one ulp below an edge, and as many above one
MIN_ON_EDGE = 500         # lookups exactly on an edge (origin (0, 0): every edge at a multiple of
#                           0.25 m is a float)
MIN_BORDER = 200          # points on each side of each map border a border walk aims at


def oracle_tolerance(scn, critics, critic, costs):
    """What separates the oracle's float32 sums from the float64 model, per rollout: T additions
    of non-negative terms (each within 2^-24 of the running sum, itself at most the result), the
    final weighted sum and its narrowing (8 more roundings, generously), and every term's own
    rounding: ObstaclesCritic narrows the distance (< 0.6 m) to float and subtracts it from a
    float constant, 3 roundings of at most 2^-24 * 0.6 m, weighted by critical_weight."""
    u = 2.0 ** -24
    w = critics.obstacles.critical_weight if critic == "obstacles" else 0.0
    return (scn.T + 8) * u * np.maximum(1.0, np.abs(costs)) + scn.T * w * 3 * u * 0.6


def run_oracle(oracle_lib, scn, critics):
    from oracle.loader import Oracle
    o = Oracle(scn.config())
    scn.configure(o, critics)
    _, out = o.optimize(scn.tick, scn.u0)
    tx, ty, _ = o.get_trajectories()
    c = o.get_costs()
    o.close()
    return out, tx, ty, c


def forms_of(key):
    return [(n, f) for n, f in E.FORMS.items() if key in f.scenes]


@pytest.mark.parametrize("key", E.all_scene_keys(), ids=[E.scene_name(k) for k in E.all_scene_keys()])
def test_edge_scene_on_the_oracle(oracle_lib, key):
    scn = E.scene(key)
    walk, border = key[2], key[2] == "border"
    assert scn.extra["noise_exact"], "a noise increment is not a float32"
    assert max(np.abs(scn.ax).max(), np.abs(scn.ay).max()) < E.MAX_DISPLACEMENT

    # the model restated by each critic the GPU test scores this scene with (ObstaclesCritic when
    # the scene is only used by the grouped or the parity case)
    critic_kinds = sorted({f.critic for _, f in forms_of(key)}) or ["obstacles"]
    for critic in critic_kinds:
        critics = E.critics_of((critic,))
        m = E.model(scn, critics, critic)
        out, tx, ty, c = run_oracle(oracle_lib, scn, critics)
        assert np.array_equal(m["x"], scn.x) and np.array_equal(m["y"], scn.y), "float32 cumsum is not exact"
        assert np.array_equal(tx, m["x"]) and np.array_equal(ty, m["y"]), "oracle trajectories differ from the model"
        d = np.abs(c.astype(np.float64) - m["costs"])
        tol = oracle_tolerance(scn, critics, critic, m["costs"])
        print(f"[edge-cpu] {scn.label} {critic}: oracle vs model max |d| {d.max():.2e} "
              f"(rel {np.max(d / np.maximum(1.0, np.abs(m['costs']))):.2e}), bound {tol.min():.2e}; "
              f"non-colliding {out.non_colliding}")
        assert np.all(d <= tol), f"oracle cost {d.max():.3e} from the model"
        assert out.non_colliding == m["non_colliding"]
        assert out.fail_flag == m["fail_flag"]
        assert E.min_single_lookup_shift(critics, scn.T, scn, critic) > 40 * d[~m["collided"]].max(initial=0.0)
        if not (border and not scn.track_unknown):
            assert m["non_colliding"] == scn.B, "a rollout collides on a scene without collisions"

    st = E.edge_stats(scn, m["x"], m["y"], m["reached"])
    print(f"[edge-cpu] {scn.label}: {st}")
    assert st["x_below"] >= MIN_NEAR_EDGE and st["x_above"] >= MIN_NEAR_EDGE, st
    if key[0] == "o0":
        assert st["x_exact"] >= MIN_ON_EDGE, st
    if border:
        for side in ("x0", "x1", "y0", "y1"):
            assert st[side + "_outside"] >= MIN_BORDER and st[side + "_inside"] >= MIN_BORDER, (side, st)
    if walk == "far":
        # past the 96-cell LDS window around the robot: the global fallback
        cells = np.abs(scn.ax) / scn.resolution
        assert int(np.sum(cells > 56)) >= MIN_NEAR_EDGE


def test_single_lookup_shift_is_the_repulsive_term_of_cost_60():
    """ISSUE figure: one wrong lookup moves a rollout's cost by at least
    repulsion_weight (R - d(60)) / T, about 9.5e-3 at T = 64."""
    scn = E.scene(E.scene_key("o0", 0))
    shift = E.min_single_lookup_shift(E.critics_of(("obstacles",)), 64, scn)
    d60 = np.log(253.0 / 60.0) / 10.0
    assert abs(shift - 1.5 * (0.55 - d60) / 64) < 1e-8
    assert 9.4e-3 < shift < 9.6e-3
