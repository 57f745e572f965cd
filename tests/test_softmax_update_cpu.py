"""The softmax control update, pinned on the CPU: the oracle against the float64 judge of
tests/softmax_model.py, on every case of its table up to 70 001 rollouts.

  * The oracle with double accumulators is within 4 units (2^-24 sum w |cv| / sum w) of the judge on
    every entry, min_cost equals min(costs), sum_w is within 4 units.  Measured 0 .. 2.1 on the
    shapes first tried; 4 leaves a factor of two for the others.  This is what pins
    update_control_sequence and apply_constraints of oracle/smpc_oracle.cpp.  The oracle with
    float accumulators (the reference's arithmetic) is within the bar by construction (its own
    error is the bar's floor); its error is printed, and is what the GPU test uses as the floor.
  * The gamma terms: costs(gamma) - costs(0) of two oracle runs against gamma_terms, within 4 ulp
    of the larger cost on the default warm start; on a warm start close to the limits, where the
    term is as large as the cost, within the worst case of the reference's float32 sums.
  * The scenes are adversarial: the judge's own update, recomputed with each planted defect of
    softmax_model.planted_defects, moves an entry of u (or sum_w, which is held to the same bar) by
    more than 10 x the bar, on every case whose shape can show the defect at all (a drop needs
    something left, a local minimum more than one group, a wrong clip a limit that binds, a vy
    defect a holonomic model); the gamma defects move the gamma term of some rollout by more than
    10 x its bar on every case with gamma > 0.
  * The regimes are reached: sum_w > 100, 1 < sum_w < 1.1, sum_w = 2 to within the bar (the tie),
    an all-collide tick, costs above 1e5, every row on its constraint, an Ackermann radius step.
"""
import numpy as np
import pytest

from tests import softmax_model as sm

CPU_CASES = [c for c in sm.CASES if not c.device_noise and c.B <= 70001]
ORACLE_UNITS = 4.0


@pytest.fixture(scope="module", autouse=True)
def _oracle_built():
    from oracle import loader
    loader.build()


run_oracle, solved = sm.run_oracle, sm.reference


@pytest.mark.parametrize("case", CPU_CASES, ids=[c.name for c in CPU_CASES])
def test_oracle_is_within_four_units_of_the_judge(case):
    bt, res = solved(case.name)
    r64, r32 = res[True], res[False]
    m32 = r32["m"]
    floor = np.abs(r32["u"].astype(np.float64) - m32.u)     # (the bar's floor: nothing to assert on it)
    with np.errstate(divide="ignore", invalid="ignore"):
        u32 = [float(np.where(m32.unit[k] > 0, floor[k] / m32.unit[k], 0.0).max()) for k in range(3)]
    j32 = dict(units=u32, sum_w_units=abs(r32["out"].sum_w - m32.sum_w) / (sm.EPS * m32.sum_w))
    assert float(r32["out"].min_cost) == m32.min
    m = r64["m"]
    print(f"[softmax-cpu] {case.name}: sum_w {m.sum_w:.6g} A {m.A:.3f} costs {r64['costs'].min():.7g} .. "
          f"{r64['costs'].max():.7g}; float-summing oracle vx {j32['units'][0]:.1f} vy {j32['units'][1]:.1f} "
          f"wz {j32['units'][2]:.1f} sum_w {j32['sum_w_units']:.1f} units (bar {sm.bar_units(case.B, m.A):.1f})")
    j64 = sm.judge(m, case.B, r64["u"], r64["out"].min_cost, r64["out"].sum_w, label=case.name + " double-summing",
                   count=ORACLE_UNITS)
    print(f"[softmax-cpu] {case.name}: double-summing oracle vx {j64['units'][0]:.2f} vy {j64['units'][1]:.2f} "
          f"wz {j64['units'][2]:.2f} sum_w {j64['sum_w_units']:.2f} units (bar {ORACLE_UNITS})")
    assert r64["out"].fail_flag == (1 if case.all_lethal else 0)


@pytest.mark.parametrize("gamma", sm.GAMMAS)
@pytest.mark.parametrize("name,warm", sm.GAMMA_CASES, ids=[f"{n}-vx{w[0]}-wz{w[2]}" for n, w in sm.GAMMA_CASES])
def test_oracle_gamma_terms(name, warm, gamma):
    bt = sm.build(sm.BY_NAME[name], warm)
    _, _, c0 = run_oracle(bt, False, gamma=0.0)
    _, _, cg = run_oracle(bt, False, gamma=gamma)
    model = sm.gamma_terms(bt.u0, bt.noise, bt.config(gamma=gamma), bt.case.model)
    ulp = np.spacing(np.maximum(np.abs(cg), np.abs(c0)).astype(np.float32)).astype(np.float64)
    err = np.abs((cg.astype(np.float64) - c0.astype(np.float64)) - model) / ulp
    print(f"[softmax-cpu] gamma {gamma} {name} warm {warm}: term {model.min():.4g} .. {model.max():.4g}, "
          f"largest error {err.max():.2f} ulp of the cost")
    if warm == sm.GAMMA_CASES[0][1]:
        assert err.max() <= 4.0
    else:
        # A warm start close to the limits: the term is as large as the cost itself (+-7 against
        # 5 .. 20 at gamma 0.1) and the float32 sums over t of terms of 0.6 have an error of their
        # own, 4.1 ulp of the cost at the worst.  Held to the worst case of the reference's own
        # arithmetic: three float32 additions to the cost (half an ulp each) and, per sum, T + 2
        # roundings (product, difference, T - 1 additions, the product with gamma / std^2) of its
        # terms' magnitudes.  The GPU test takes the error measured here as its reference.
        worst = 1.5 + (bt.case.T + 2) * sm.EPS * sm.gamma_magnitude(bt.u0, bt.noise, bt.config(gamma=gamma),
                                                                     bt.case.model) / ulp
        assert np.all(err <= worst), float(np.max(err / worst))


@pytest.mark.parametrize("case", CPU_CASES, ids=[c.name for c in CPU_CASES])
def test_every_planted_defect_is_seen(case):
    bt, res = solved(case.name)
    r = res[False]
    m = r["m"]
    count = sm.bar_units(case.B, m.A)
    bar = count * m.unit
    if m.min_r >= 0.0:
        bar[2] = np.maximum(bar[2], bar[0] / m.min_r) + 2.0 * sm.EPS * np.abs(m.u[2])
    defects = sm.planted_defects(r["costs"], r["u_in"], bt.noise, bt.cfg, bt.constraints, case.model)
    B = case.B
    # the only reasons for a defect not to apply: the shape (asserted here, so that none slips out)
    absent = {n for n, d in defects.items() if d is None}
    allowed = set()
    if B <= 64:
        allowed |= {"last partial group of 64 dropped", "weights against a per-64 minimum, not rescaled"}
    if B <= 16:
        allowed |= {"last B mod 16 rollouts dropped"}
    if B <= 1024:
        allowed |= {"weights against a per-1024 minimum, not rescaled"}
    if B == 1:
        allowed |= {"last rollout dropped", "phantom copy of rollout 0"}
    if case.constraints is None or case.model != sm.OMNI:
        allowed |= {"vy clipped with wz's limit"}
    assert absent <= allowed, (case.name, absent - allowed)
    for name, d in defects.items():
        if d is None:
            continue
        u_d, sw_d = d
        with np.errstate(divide="ignore", invalid="ignore"):
            moved = np.where(bar > 0, np.abs(u_d - m.u) / bar, 0.0)
        if m.keeps_vy:
            moved[1] = 0.0
        moved_sw = abs(sw_d - m.sum_w) / (count * sm.EPS * m.sum_w)
        print(f"[softmax-cpu] {case.name}: {name}: u moves {moved.max():.3g} x the bar, sum_w {moved_sw:.3g} x")
        assert max(moved.max(), moved_sw) > 10.0, (case.name, name)
    # (the gamma defects need a cost whose ulp is small next to the term: not an all-collide tick,
    # whose costs of 200 000 have an ulp of 0.016 under a term of +-0.4; and the warm start itself)
    if case.gamma > 0.0 and case.iterations == 1 and not case.all_lethal:
        terms = sm.gamma_terms(bt.u0, bt.noise, bt.cfg, case.model)
        ulp = np.spacing(np.abs(r["costs"]).astype(np.float32)).astype(np.float64)
        for name, t in sm.gamma_defects(bt.u0, bt.noise, bt.cfg, case.model).items():
            moved = np.abs(t - terms) / (4.0 * ulp)
            print(f"[softmax-cpu] {case.name}: gamma {name}: a term moves {moved.max():.3g} x its bar")
            assert moved.max() > 10.0, (case.name, name)


def test_the_regimes_are_reached():
    seen = {k: [] for k in ("sum_w > 100", "1 < sum_w < 1.1", "sum_w = 2 (tie)", "all collide", "costs > 1e5",
                            "every row on its constraint", "radius step")}
    for case in CPU_CASES:
        bt, res = solved(case.name)
        r = res[False]
        m = r["m"]
        tol = sm.bar_units(case.B, m.A) * sm.EPS * 2.0
        if m.sum_w > 100.0:
            seen["sum_w > 100"].append(case.name)
        if 1.0 < m.sum_w < 1.1:
            seen["1 < sum_w < 1.1"].append(case.name)
        if case.tie and 2.0 - tol <= m.sum_w < 2.5:
            seen["sum_w = 2 (tie)"].append(case.name)
        if r["out"].fail_flag == 1:
            assert r["out"].non_colliding == 0
            seen["all collide"].append(case.name)
        if r["costs"].min() > 1e5:
            seen["costs > 1e5"].append(case.name)
        on = [np.any((m.raw[k] > m.limits[k][1]) | (m.raw[k] < m.limits[k][0])) for k in range(3)]
        if all(on):
            seen["every row on its constraint"].append(case.name)
        if m.radius.any():
            seen["radius step"].append(case.name)
    for k, v in seen.items():
        print(f"[softmax-cpu] regime {k}: {v}")
    assert all(seen.values()), {k: v for k, v in seen.items() if not v}
    # on a wave and on a lane case each
    for k in ("all collide",):
        assert {sm.BY_NAME[n].path for n in seen[k]} >= {"wave", "lane"}
