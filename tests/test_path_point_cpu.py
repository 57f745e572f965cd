"""The path-point scenes are exact, adversarial, and the oracle makes every choice the model makes.

tests/path_point_scenes.py builds rollouts whose PathAlign path point is decided at exact ties,
equalities, stalls and overruns, and judges them with a float64 model transcribed from the
reference's lines.  tests/test_gpu_path_point.py holds every kernel family to the oracle's cost on
those scenes with no flip allowance; that only means something if, on the oracle alone,

  * the stored noise and the trajectories are the intended points bit for bit,
  * the oracle's furthest point and its per-rollout PathAlign cost are the model's (within a
    fortieth of the least a single other choice moves a cost: a tenth of the GPU test's tolerance),
  * every category the scenes aim at is there in numbers (printed).

If the premise fails, the scene or the oracle is wrong, not a kernel.
"""
import numpy as np
import pytest

from oracle.loader import Oracle, ptr
from tests import path_point_scenes as S

CASES = S.judged_cases()


@pytest.mark.parametrize("case", CASES, ids=[f"{S.scene_name(k)}-pow{p}" for k, p in CASES])
def test_scene_is_exact_adversarial_and_the_oracle_follows_the_model(oracle_lib, case):
    key, power = case
    scn = S.scene(key)
    j = S.judged(key, power)
    label = f"{scn.label} power {power}"
    # exactness: the noise survives float32, the oracle's points are the intended ones
    assert scn.extra["noise_exact"], label
    assert np.array_equal(j["x"], scn.x) and np.array_equal(j["y"], scn.y), label
    o = Oracle(scn.config())
    scn.configure(o, S.critics_of(S.ONLY, scn.step, power))
    _, out = o.optimize(scn.tick, scn.u0)
    tx, ty, _ = o.get_trajectories()
    costs = o.get_costs().astype(np.float64)
    o.close()
    assert np.array_equal(tx, scn.x) and np.array_equal(ty, scn.y), label
    # the premise
    assert j["scored"], f"{label}: the occupancy gate or the furthest point keeps PathAlign from scoring"
    assert out.fail_flag == 0, label
    assert out.furthest_valid and out.furthest_reached_path_point == j["furthest"] == S.G_FURTHEST, label
    d = np.abs(costs - j["pa"])
    print(f"[path point] {label}: N {scn.N} K {scn.K}; least single-choice shift {j['shift']:.3e}; "
          f"oracle vs float64 model {d.max():.3e}")
    assert j["shift"] > 0.0
    bad = int(np.sum(~(d <= 0.025 * j["shift"])))
    assert bad == 0, f"{label}: the oracle chose another point in {bad} rollouts (worst {d.max():.3e}, rollout {int(d.argmax())})"
    # adversarial
    st = j["stats"]
    print(f"[path point] {label}: {st}")
    assert st["endpoints_past"] == 0, label
    for name in S.admitted(scn):
        assert st[name] >= S.MIN_COUNT, (label, name, st[name])
    if scn.Nt >= 4:
        base = min(scn.B, 4096)
        for L in range(1, scn.K + 1):
            assert st["stall_runs"].get(L, 0) >= S.MIN_COUNT, (label, "stall run of length", L)
        assert st["full_length_rollouts"] >= base // 4, label
        assert np.all(scn.family[0:base:4] == S.FAMILIES.index("full_stall")), label


def test_find_closest_path_pt_against_the_oracle(oracle_lib):
    """The model's findClosestPathPt on the vectors of test_find_closest_path_pt_quirks and on a
    swept grid of (dist, init) over a non-uniform D with repeats."""
    f = oracle_lib.smpc_oracle_find_closest_path_pt
    vec = np.array([0.0, 1.0, 2.0, 3.0], np.float32)
    for dist, init, want in ((0.0, 0, 0), (1.4, 0, 1), (1.6, 0, 2), (1.5, 0, 2), (2.0, 2, 0), (9.0, 1, 3)):
        pt, _ = S.find_closest_path_pt(vec, np.array([dist]), np.array([init]))
        assert int(pt[0]) == want == f(ptr(vec), 4, dist, init), (dist, init)
    D = np.array([0.0, 0.25, 0.25, 0.3125, 1.0, 1.0, 1.0, 1.125, 2.5, 2.5625], np.float32)
    sweep = np.unique(np.concatenate([np.arange(-2, 90) / 32.0, D, (D[1:] + D[:-1]) / 2,
                                      np.nextafter(D, np.float32(9)), np.nextafter(D, np.float32(-9))]).astype(np.float32))
    n = 0
    for init in range(len(D)):
        # (the reference's callers keep init at or below the lower bound's index plus one;
        # the rule itself is defined for any init)
        pts, _ = S.find_closest_path_pt(D, sweep, np.full(len(sweep), init))
        for dist, pt in zip(sweep, pts):
            assert int(pt) == f(ptr(D), len(D), float(dist), init), (float(dist), init)
            n += 1
    print(f"[path point] findClosestPathPt: {n} (dist, init) pairs agree")
