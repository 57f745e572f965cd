"""The LDS carve-up of the three scoring passes (smpc_prepare.cpp make_lds / lane_lds / split_lds)
against what the kernels touch, and the longest plan each form admits into 160 KB.

The layouts come from the host-only debug export smpc_debug_lds_layout (no device call).  Every
requirement below is stated from the kernel text that reads or writes the region — the line is
cited next to it — not from the layout functions: a region one element short faults nothing on the
GPU (an LDS write out of range is dropped, a read returns 0), so this is where it shows.

The admission limits (largest P with total <= 160 KB) are pinned as literals.  plan_launch drops a
tick from the lane pass to the wave pass where the lane layout no longer fits: a layout change that
shrinks what rides the lane pass is a diff here, not only a slower tick."""
import numpy as np
import pytest

from tests.harness import lib  # noqa: F401
from tests.plan_scenes import KIND_LANE, KIND_SPLIT, KIND_WAVE, LDS_PER_CU, lds_layout, plan_limit

WORDS = ("off_lut", "off_px", "off_py", "off_pyaw", "off_D", "off_valid", "off_scr", "off_pts4", "off_prune",
         "scr_stride", "scr_pts", "scr_ring", "scr_c", "seg_shift", "group", "total")   # SmpcLds, smpc_dev.h:285-296

P_ALL = np.arange(1, 1025, dtype=np.int64)
HORIZONS = (1, 4, 30, 36, 40, 56, 60, 64, 100, 128, 200, 256)
WINDOWS = (0, 96 * 96, 144 * 144, 83 * 96)     # none, the default, the wide one (T > 64), a window cropped by the map's edge
PRUNE_FLOATS = 4 + 8 * 16                      # SMPC_PRUNE_FLOATS, smpc_dev.h:202-203
LUT_ENTRY = 8                                  # SmpcLut {crit, rep}: two floats
LANE_BLOCK = 512                               # smpc_lane.hip:48, :54 (both forms)
SPLIT_BLOCK = 512                              # smpc_split.hip:46
PARK_STRIDE = 68                               # LANE_PARK_STRIDE, smpc_lane_common.h:23


def sweep(lib, kind, window, T, arg):
    """The layout of every P in 1..1024 as a dict of int64 arrays."""
    out = np.zeros((len(P_ALL), 16), np.uint32)
    base, fn = out.ctypes.data, lib.smpc_debug_lds_layout
    for i, P in enumerate(P_ALL):
        assert fn(kind, window, int(P), T, arg, base + 64 * i) == 0
    return {w: out[:, k].astype(np.int64) for k, w in enumerate(WORDS)}


def holds(cond, what, kind, window, T, arg):
    bad = np.flatnonzero(~np.asarray(cond))
    assert bad.size == 0, f"{what}: kind {kind} window {window} T {T} arg {arg}, first at P = {P_ALL[bad[0]]} ({bad.size} plans)"


def check_path_regions(L, ck, window, win_need, lut_entries, after_valid, padded):
    """What the three passes share: window, table, px / py / pyaw / D / valid, in this order."""
    P = P_ALL
    # the window sits at the start of the launch's LDS (s_map = smem: smpc_lane_pass.inc:52,
    # smpc_split.hip:167, smpc_wave_pass.inc:44), the table behind it
    if window:
        ck(L["off_lut"] >= win_need, "window region too small")
        ck(L["off_px"] - L["off_lut"] >= lut_entries * LUT_ENTRY, "lookup table region too small")
        ck(L["off_lut"] % 8 == 0, "lookup table: 8-byte entries")
    ck(L["off_lut"] <= L["off_px"], "order lut, px")
    # px, py: P floats (smpc_wave_pass.inc:92-94); the lane and the split pass fill up to the next
    # multiple of four with 1e18 (smpc_lane_pass.inc:135, smpc_split.hip:225) and scan four points
    # per 16-byte read (smpc_lane_furthest.inc:78-79, smpc_split.hip:608-609)
    n_xy = 4 * ((P + 3) // 4 * 4 if padded else P)
    ck(L["off_py"] - L["off_px"] >= n_xy, "px too small")
    ck(L["off_pyaw"] - L["off_py"] >= n_xy, "py too small")
    ck(L["off_px"] % (16 if padded else 4) == 0, "px alignment")
    ck(L["off_py"] % (16 if padded else 4) == 0, "py alignment")
    # pyaw: P floats (smpc_wave_pass.inc:96)
    ck(L["off_D"] - L["off_pyaw"] >= 4 * P, "pyaw too small")
    ck(L["off_pyaw"] % 4 == 0, "pyaw alignment")
    # D: P - 1 cumulative lengths (smpc_wave_pass.inc:98) and, in the lane and the split pass, s_D one
    # float into the region with a sentinel at [-1] and at [S], S <= P - 1 (smpc_lane_pass.inc:58,
    # :199-202, smpc_split.hip:171): P + 2 floats
    ck(L["off_valid"] - L["off_D"] >= 4 * (P + 2), "D too small")
    ck(L["off_D"] % 4 == 0, "D alignment")
    # valid: one byte per point (smpc_wave_pass.inc:99, :270, :321)
    ck(after_valid - L["off_valid"] >= P, "valid too small")


@pytest.mark.parametrize("T", HORIZONS)
@pytest.mark.parametrize("window", WINDOWS)
def test_wave_pass_layout_covers_what_the_kernel_touches(lib, window, T):
    nwave = 8 if T > 128 else 16          # pass_block: 512 threads for R = 4, else 1024 (smpc_ctx.h:88)
    for nsamp in (0, 13, 15, 16, 31, 32, 63):
        L = sweep(lib, KIND_WAVE, window, T, nsamp)

        def ck(cond, what):
            holds(cond, what, "wave", window, T, nsamp)
        # the window alone: a lookup outside it goes to the global map (smpc_device_math.h:158-162);
        # 256 table entries (smpc_wave_pass.inc:89-90)
        check_path_regions(L, ck, window, window, 256, L["off_scr"], padded=False)
        # per wave (smpc_wave_pass.inc:59-65): sample points [3][64], endpoint ring [2][64], parked
        # controls [group][3][T] (:346, :875); the head is re-used for the block combine's 4 + 3T
        # floats (:916 on); slot = g * SEG + s with s = 0..nsamp (:60, :175) inside the 64 lanes
        ck(L["scr_pts"] + 3 * 64 <= L["scr_ring"], "sample points overlap the ring")
        ck(L["scr_ring"] + 2 * 64 <= L["scr_c"], "ring overlaps the parked controls")
        ck(L["group"] >= 1, "group")
        ck(L["scr_c"] + L["group"] * 3 * T <= L["scr_stride"], "parked controls beyond the wave's scratch")
        ck(4 + 3 * T <= L["scr_stride"], "block combine beyond the wave's scratch")
        ck((1 << L["seg_shift"]) >= nsamp + 1, "sample slots beyond the segment")
        ck((L["group"] << L["seg_shift"]) <= 64, "segments beyond the wave")
        ck(L["off_scr"] % 4 == 0, "scratch alignment")
        ck(L["off_valid"] < L["off_scr"], "order valid, scratch")
        ck(L["total"] == L["off_scr"] + nwave * L["scr_stride"] * 4, "total is not the end of the last wave's scratch")
        # (every wave-pass layout fits: plan_launch refuses the tick otherwise, "LDS budget exceeded")
        ck(L["total"] <= LDS_PER_CU, "wave pass beyond 160 KB")


@pytest.mark.parametrize("T", HORIZONS)
@pytest.mark.parametrize("window", WINDOWS)
def test_lane_pass_layout_covers_what_the_kernel_touches(lib, window, T):
    P = P_ALL
    for rr in (0, 1):
        L = sweep(lib, KIND_LANE, window, T, rr)

        def ck(cond, what):
            holds(cond, what, "lane", window, T, rr)
        # window + the NO_INFORMATION byte (smpc_lane_pass.inc:133) + one scratch byte per lane of the
        # block at nwin + 1 + wave * 64 + lane (smpc_lane_common.h:148, smpc_lane_pass.inc:402-403);
        # 256 table entries and the all-zero one (smpc_lane_pass.inc:128-129)
        check_path_regions(L, ck, window, window + 1 + LANE_BLOCK, 257, L["off_prune"], padded=True)
        # the prune table (smpc_lane_pass.inc:70, :136), read as 16-byte halves of an entry from its
        # fifth float on (smpc_lane_furthest.inc:60-61)
        ck(L["off_valid"] < L["off_prune"], "order valid, prune")
        ck(L["off_pts4"] - L["off_prune"] >= 4 * PRUNE_FLOATS, "prune table too small")
        ck(L["off_prune"] % 16 == 0, "prune table alignment")
        # {x, y, valid, 0} per point, one 16-byte access (smpc_lane_pass.inc:60, :141, :169), and sum
        # u^2 in the 16 bytes in front of the per-wave scratch (smpc_lane_pass.inc:63, :157-161)
        ck(L["off_pts4"] % 16 == 0, "pts4 alignment")
        ck(L["off_scr"] - 16 >= L["off_pts4"] + 16 * P, "sum u^2 overlaps the path points")
        # per wave (smpc_lane_pass.inc:85-86): parked wz [64][68] (:615, two more floats per row:
        # smpc_lane_furthest.inc:35-36) and the softmax weights [64] behind it (:850), both read in
        # 16-byte pieces (:854-859); the head is re-used for the block combine's 4 + 3T (:890-906).
        # The re-read form parks nothing (smpc_lane.hip)
        ck(L["off_scr"] % 16 == 0, "scratch alignment")
        ck(L["scr_stride"] % 4 == 0, "scratch stride alignment")
        if not rr:
            ck(L["scr_stride"] >= 64 * PARK_STRIDE + 64, "parked tile beyond the wave's scratch")
        ck(L["scr_stride"] >= 4 + 3 * T, "block combine beyond the wave's scratch")
        ck(L["total"] == L["off_scr"] + (LANE_BLOCK // 64) * L["scr_stride"] * 4,
           "total is not the end of the last wave's scratch")


@pytest.mark.parametrize("T", HORIZONS)
@pytest.mark.parametrize("window", WINDOWS)
def test_split_pass_layout_covers_what_the_kernel_touches(lib, window, T):
    P = P_ALL
    for nseg in (2, 4):
        L = sweep(lib, KIND_SPLIT, window, T, nseg)

        def ck(cond, what):
            holds(cond, what, "split", window, T, nseg)
        # window + NO_INFORMATION byte (smpc_split.hip:224) + one byte per lane (:420); 256 entries (:223)
        check_path_regions(L, ck, window, window + 1 + SPLIT_BLOCK, 256, L["off_pts4"], padded=True)
        # path points (smpc_split.hip:172, :230, :238); in front of the per-wave scratch sum u^2 [4] and
        # u [3][64] (smpc_split.hip:174-175)
        ck(L["off_valid"] < L["off_pts4"], "order valid, pts4")
        ck(L["off_pts4"] % 16 == 0, "pts4 alignment")
        ck(L["off_scr"] - 4 * (3 * 64 + 4) >= L["off_pts4"] + 16 * P, "sum u^2 / u overlap the path points")
        # per wave: parked wz [64 / nseg][64], two segments: vy behind it (smpc_split.hip:184-185,
        # :343); the head is re-used for the block combine (:692 on)
        ck(L["off_scr"] % 16 == 0, "scratch alignment")
        ck(L["scr_stride"] >= (2 if nseg == 2 else 1) * (64 // nseg) * 64, "parked tile beyond the wave's scratch")
        ck(L["scr_stride"] >= 4 + 3 * T, "block combine beyond the wave's scratch")
        ck(L["total"] == L["off_scr"] + (SPLIT_BLOCK // 64) * L["scr_stride"] * 4,
           "total is not the end of the last wave's scratch")


def test_export_refuses_what_is_not_a_layout(lib):
    out = np.zeros(16, np.uint32)
    assert lib.smpc_debug_lds_layout(3, 0, 10, 64, 0, out.ctypes.data) != 0
    assert lib.smpc_debug_lds_layout(KIND_SPLIT, 0, 10, 64, 3, out.ctypes.data) != 0
    assert lib.smpc_debug_lds_layout(KIND_LANE, 0, 10, 64, 0, None) != 0


# (form, kind, window bytes, T, arg) -> (largest P admitted, LDS bytes there).  The parking form's
# scratch does not depend on T <= 64 (the parked tile exceeds 4 + 3T), so its limit is one number.
LIMITS = [
    ("lane parking, costmap scored", KIND_LANE, 96 * 96, (30, 40, 56, 64), 0, 307, 163840),
    ("lane parking, no costmap lookup", KIND_LANE, 0, (30, 40, 56, 64), 0, 664, 163792),
    ("lane re-read, T = 64", KIND_LANE, 96 * 96, (64,), 1, 1024, 52432),
    ("lane re-read, T = 128, wide window", KIND_LANE, 144 * 144, (128,), 1, 1024, 70096),
    ("split, four segments", KIND_SPLIT, 96 * 96, (36, 60, 64), 4, 1024, 79168),
    ("split, two segments", KIND_SPLIT, 96 * 96, (64,), 2, 610, 163840),
]


@pytest.mark.parametrize("case", LIMITS, ids=[c[0] for c in LIMITS])
def test_admission_limits_are_where_they_were(case):
    form, kind, window, horizons, arg, p_star, total = case
    for T in horizons:
        got = plan_limit(kind, window, T, arg)
        got_total = lds_layout(kind, window, got, T, arg)["total"]
        print(f"[lds limit] {form}, T {T}: P* {got}, {got_total} bytes")
        assert (got, got_total) == (p_star, total), (form, T)
        if got < 1024:
            assert lds_layout(kind, window, got + 1, T, arg)["total"] > LDS_PER_CU


def test_wave_pass_admits_every_plan():
    for T in HORIZONS:
        for window in WINDOWS:
            for nsamp in (0, 15, 16, 31, 32, 63):
                assert plan_limit(KIND_WAVE, window, T, nsamp) == 1024, (T, window, nsamp)
