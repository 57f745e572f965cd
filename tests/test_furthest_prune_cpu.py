"""The host's furthest-point prune table (smpc_prepare.cpp build_prune_table) against a brute-force
model: a float32 NumPy restatement of the lane pass's nearest-point scan and point_F, and of the
per-lane test in smpc_lane_furthest.inc.  The table is reached through the host-only debug export
smpc_debug_prune_table (no device call).

For every plan, every table entry K and a grid of fractions phi, theta = float32(K + phi) stands
for a furthest point some rollout has already attained.  No endpoint may be called prunable while
its F exceeds theta: zero violations.  So that never pruning does not pass, on the straight plan
at least 99 % of the endpoints with F <= theta - 0.01 must be called prunable."""
import numpy as np
import pytest

from tests.harness import debug_prune_table, lib  # noqa: F401

f32 = np.float32
ENTRIES = 16
FLOATS = 4 + 8 * ENTRIES
RES = 0.05


def table(lib, px, py, k0, on=1):
    out = debug_prune_table(px, py, k0, on, FLOATS)
    head = out[:4].view(np.uint32)
    return int(head[0]), int(head[1]), out[4:].reshape(ENTRIES, 8)


def model_F(px, py, x, y):
    """F of every endpoint (x[i], y[i]): the kernel's full scan (first minimum of the float32
    squared distances) and point_F, in float32 with the kernel's order of operations."""
    P = len(px)
    ex = px[None, :] - x[:, None]
    ey = py[None, :] - y[:, None]
    dd = ex * ex + ey * ey                      # float32: products and sum rounded one by one
    bi = np.argmin(dd, axis=1)                  # the first minimum
    best = dd[np.arange(len(x)), bi]
    F = bi.astype(f32)
    nxt = np.minimum(bi + 1, P - 1)
    nx, ny = px[nxt], py[nxt]
    sgx, sgy = nx - px[bi], ny - py[bi]
    d_next = (nx - x) * (nx - x) + (ny - y) * (ny - y)
    seg2 = sgx * sgx + sgy * sgy
    with np.errstate(divide="ignore", invalid="ignore"):
        tt = np.where(seg2 > 0, f32(0.5) + f32(0.5) * (best - d_next) * (f32(1.0) / seg2), f32(0.0)).astype(f32)
    Fn = np.maximum(F + np.minimum(np.maximum(tt, f32(-0.45)), f32(0.45)), f32(0.0)).astype(f32)
    return np.where(bi + 1 < P, Fn, F).astype(f32)


def model_prunable(ent, theta, x, y):
    """smpc_lane_furthest.inc's per-lane test, float32, same order of operations."""
    e = ent.astype(f32)
    ex, ey = x - e[0], y - e[1]
    ps = e[2] * ex + e[3] * ey
    pt = e[2] * ey - e[3] * ex
    theta = f32(theta)
    return ((np.maximum(np.abs(ps), np.abs(pt)) <= f32(1.0)) & (ps + e[4] * np.abs(pt) <= e[5]) &
            (np.rint(theta) + np.maximum(ps * e[6] + e[7], f32(-0.45)) <= theta))


def endpoints(px, py, rng):
    """A dense grid around the plan, and many points within 1e-6 of the bisectors between
    neighbouring plan points and of the lines lambda = phi used below."""
    lo_x, hi_x = float(px.min()) - 0.4, float(px.max()) + 0.4
    lo_y, hi_y = float(py.min()) - 0.4, float(py.max()) + 0.4
    gx, gy = np.meshgrid(np.linspace(lo_x, hi_x, 90), np.linspace(lo_y, hi_y, 50))
    xs, ys = [gx.ravel()], [gy.ravel()]
    P = len(px)
    for k in range(P - 1):
        ax, ay, bx, by = float(px[k]), float(py[k]), float(px[k + 1]), float(py[k + 1])
        dx, dy = bx - ax, by - ay
        seg = np.hypot(dx, dy)
        if seg == 0:
            continue
        nx, ny = -dy / seg, dx / seg
        for lam in (0.5,) + tuple(0.5 + p for p in PHIS) + tuple(p for p in PHIS):
            t = rng.uniform(-0.3, 0.3, 6)
            off = rng.uniform(-1e-6, 1e-6, 6)
            xs.append(ax + (lam + off / seg) * dx + t * nx)
            ys.append(ay + (lam + off / seg) * dy + t * ny)
    return np.concatenate(xs).astype(f32), np.concatenate(ys).astype(f32)


PHIS = (-0.45, -0.3, -0.1, 0.0, 0.2, 0.45)
# (beside the fractions a bound can take, the values rint() hands over at its edges)
PHI_ALL = PHIS + (-0.5, -0.4500001, 0.4499999, 0.5)


def arc(radius, P, res=RES):
    a = np.arange(P) * res / radius
    return (1.0 + radius * np.sin(a)).astype(f32), (2.0 + radius * (1.0 - np.cos(a))).astype(f32)


def straight(P, res=RES):
    return (1.0 + res * np.arange(P)).astype(f32), np.full(P, 2.0, f32)


def uturn(P=60, res=RES):
    k = np.arange(P)
    x = 1.0 + res * np.minimum(k, 33) - res * np.maximum(k - 33, 0)
    return x.astype(f32), (2.0 + np.where(k > 33, 0.05, 0.0)).astype(f32)


def repeated(P=24, res=RES):
    x, y = straight(P, res)
    x[7] = x[6]
    x[15] = x[14] = x[13]
    return x, y


PLANS = {
    "straight": straight(40),
    "arc r=0.5": arc(0.5, 40),
    "arc r=1.5": arc(1.5, 48),
    "arc r=6": arc(6.0, 60),
    "u-turn": uturn(),
    "coarse": straight(60, 3 * RES),
    "repeated points": repeated(),
    "P=1": straight(1),
    "P=2": straight(2),
    "P=3": straight(3),
}


def check_plan(lib, name, px, py):
    rng = np.random.default_rng(7)
    P = len(px)
    x, y = endpoints(px, py, rng)
    F = model_F(px, py, x, y)
    # K at both ends of the plan and in its middle
    starts = sorted({0, max(0, P // 2 - ENTRIES // 2), max(0, P - ENTRIES)})
    called = eligible = pruned_eligible = 0
    for k0 in starts:
        got_k0, n, ents = table(lib, px, py, k0)
        assert got_k0 == k0 and n == min(ENTRIES, P - k0)
        for i in range(n):
            K = k0 + i
            for phi in PHI_ALL:
                theta = f32(K + phi)
                if theta < 0:
                    continue
                Kf = np.rint(theta)             # as the kernel takes the entry and the fraction
                if int(Kf) != K:
                    continue
                ph = f32(theta - Kf)
                pr = model_prunable(ents[i], theta, x, y)
                bad = pr & (F > theta)
                assert not bad.any(), (name, K, float(ph), x[bad][:3], y[bad][:3], F[bad][:3])
                called += int(pr.sum())
                # (a bound at the plan's last point is that point's own F = P - 1 exactly: another
                # fraction there is checked for violations above but cannot occur, and is not counted)
                if -0.4501 <= ph <= 0.4501 and (K + 1 < P or ph == 0):
                    el = F <= theta - f32(0.01)
                    eligible += int(el.sum())
                    pruned_eligible += int((pr & el).sum())
    return called, eligible, pruned_eligible


@pytest.mark.parametrize("name", list(PLANS))
def test_no_endpoint_above_the_bound_is_pruned(lib, name):
    px, py = PLANS[name]
    called, eligible, pruned = check_plan(lib, name, px, py)
    print(f"[furthest prune] {name}: {called} prunable calls, {pruned} of {eligible} eligible pruned")
    if name == "straight":
        assert pruned >= 0.99 * eligible, (pruned, eligible)


def test_straight_plan_prunes_per_entry(lib):
    """The 99 % hold for every (K, phi) of the straight plan on its own, not only in the sum."""
    px, py = PLANS["straight"]
    x, y = endpoints(px, py, np.random.default_rng(7))
    F = model_F(px, py, x, y)
    for k0 in (0, 12, 24):
        _, n, ents = table(lib, px, py, k0)
        for i in range(n):
            for phi in PHIS:
                theta = f32(k0 + i + phi)
                if theta < 0 or (k0 + i + 1 == len(px) and phi != 0):
                    continue
                el = F <= theta - f32(0.01)
                pr = model_prunable(ents[i], theta, x, y)
                if el.sum():
                    assert (pr & el).sum() >= 0.99 * el.sum(), (k0 + i, phi, int((pr & el).sum()), int(el.sum()))


def test_nan_and_far_endpoints_fail_the_test(lib):
    px, py = PLANS["straight"]
    _, n, ents = table(lib, px, py, 24)
    x = np.array([np.nan, 1.0, 1e30, -1e30, 1.0, np.inf], f32)
    y = np.array([2.0, np.nan, 2.0, 2.0, 1e30, 2.0], f32)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(n):
            assert not model_prunable(ents[i], 24 + i + 0.45, x, y).any()


def test_empty_table_never_prunes(lib):
    """SMPC_FURTHEST_PRUNE=0 and long plans: every entry "never prune"."""
    px, py = PLANS["straight"]
    x, y = endpoints(px, py, np.random.default_rng(7))
    _, n, ents = table(lib, px, py, 24, on=0)
    assert n == ENTRIES
    for i in range(n):
        assert not model_prunable(ents[i], 24 + i + 0.45, x, y).any()


def test_doubling_back_marks_never_prune(lib):
    """Entries in front of the U-turn's bend see later points behind them: never prune."""
    px, py = PLANS["u-turn"]
    x, y = endpoints(px, py, np.random.default_rng(7))
    _, n, ents = table(lib, px, py, 20)
    for i in range(n):
        if 20 + i < 33:
            assert ents[i][5] == f32(-4.0), (20 + i, ents[i])
