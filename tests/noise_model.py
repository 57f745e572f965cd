"""The device noise stream as a specification, in NumPy only: integer Philox4x32-10 (Salmon et
al., SC'11; pinned by the published known answers in test_noise_stream_cpu.py), the float32
uniforms and angle exactly as the kernels form them, and Box-Muller in float64 from there on.
The tests hold both the HIP kernels and the CPU oracle to it.

Element e = shard_offset*T + b*T + t of a tensor's global [B_global, T] array:
  * Philox block: counter {lo32(e>>2), hi32(e>>2), stream, epoch}, key {lo32(seed), hi32(seed)};
    stream 0 = vx, 1 = wz, 2 = vy; epoch 0 after seed(), +1 per reset() / redraw;
  * words (0, 1) of the block when e & 2 == 0, else (2, 3);
  * float32: u = ((float)(word >> 8) + 0.5f) * 2^-24; the pair's first word gives u1, the second u2;
  * float32: ang = 6.2831853071795864769f * u2 (this rounding belongs to the specification);
  * float64: r = sqrt(-2 ln u1), z = r cos(ang) for even e, r sin(ang) for odd e;
  * the tensor holds (float)z * sigma.
"""
import functools
import math
from statistics import NormalDist

import numpy as np

STREAM_VX, STREAM_WZ, STREAM_VY = 0, 1, 2

_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_LO = np.uint64(0xFFFFFFFF)
_32 = np.uint64(32)

# Random123's kat_vectors for philox4x32 with 10 rounds: (counter, key, expected)
KNOWN_ANSWERS = (
    ((0x00000000,) * 4, (0x00000000,) * 2, (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
)

# the cases the CPU (oracle) and GPU tensor tests share
SHAPES_LANE = ((1, 4), (63, 8), (65, 36), (257, 60), (4099, 64), (300, 128), (130, 256))   # T % 4 == 0
SHAPES_PLAIN = ((777, 33), (1000, 30))       # T % 4 != 0: the plain fill whatever the flags
SHARDS = ((133, 33, 67), (8, 64, 2**28), (8, 64, 2**28 - 3))    # (B, T, shard_offset); the last straddles q = 2^32
SEEDS = (2024, (5 << 32) | 2024, 2**64 - 1)
STDS = {"vx_std": 0.2, "vy_std": 0.3, "wz_std": 0.4}     # unequal: a swapped stream or sigma shows
STAT_SHAPE = (65536, 64)
STAT_SEEDS = SEEDS[:2]
TENSOR_RTOL = 6e-7     # |tensor - sigma z| <= sigma * TENSOR_RTOL * radius
HOOK_RTOL = 4.5e-7     # |box_muller - z| <= HOOK_RTOL * radius

MAX_RADIUS = 5.8871  # sqrt(-2 ln 2^-25) = 5.88705, the radius of the smallest u1


def philox4x32_10(ctr, key):
    """ctr: integers [n, 4] (each < 2^32), key: (k0, k1) -> uint32 [n, 4]."""
    c = np.asarray(ctr).astype(np.uint64).reshape(-1, 4)
    c0, c1, c2, c3 = (c[:, i].copy() for i in range(4))
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = _M0 * c0, _M1 * c2          # 32 x 32 -> 64: no overflow in uint64
        n0 = (p1 >> _32) ^ c1 ^ np.uint64(k0)
        n2 = (p0 >> _32) ^ c3 ^ np.uint64(k1)
        c0, c1, c2, c3 = n0, p1 & _LO, n2, p0 & _LO
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return np.stack([c0, c1, c2, c3], axis=1).astype(np.uint32)


def words(seed, stream, epoch, elements):
    """The pair of Philox words behind each flat element index: uint32 (r0, r1)."""
    e = np.asarray(elements, dtype=np.uint64).reshape(-1)
    q = e >> np.uint64(2)
    q0, q1 = int(q.min()), int(q.max())
    if q1 - q0 + 1 <= 2 * e.size:            # a dense range of blocks: each computed once
        uq = np.uint64(q0) + np.arange(q1 - q0 + 1, dtype=np.uint64)
        idx = (q - np.uint64(q0)).astype(np.int64)
    else:
        uq, idx = np.unique(q, return_inverse=True)
    ctr = np.stack([uq & _LO, uq >> _32, np.full_like(uq, stream), np.full_like(uq, epoch)], axis=1)
    seed = int(seed)
    blk = philox4x32_10(ctr, (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    w = (e & np.uint64(2)).astype(np.int64)
    return blk[idx, w], blk[idx, w + 1]


def uniforms(w):
    """float32 u = ((float)(w >> 8) + 0.5f) * 2^-24, in (0, 1]: 1.0 exactly at w >> 8 = 2^24 - 1."""
    k = (np.asarray(w, dtype=np.uint32) >> np.uint32(8)).astype(np.float32)
    return (k + np.float32(0.5)) * np.float32(1.0 / 16777216.0)


def normals64(r0, r1):
    """Box-Muller of word pairs -> float64 (radius cos, radius sin, radius); radius is -0.0 at u1 == 1."""
    u1, u2 = uniforms(r0), uniforms(r1)
    ang = (np.float32(6.2831853071795864769) * u2).astype(np.float64)
    radius = np.sqrt(-2.0 * np.log(u1.astype(np.float64)))
    return radius * np.cos(ang), radius * np.sin(ang), radius


def tensor(seed, stream, epoch, B, T, shard_offset=0):
    """(z [B, T], radius [B, T]) in float64, before the multiplication by sigma."""
    e = np.uint64(int(shard_offset) * T) + np.arange(B * T, dtype=np.uint64)
    zc, zs, radius = normals64(*words(seed, stream, epoch, e))
    z = np.where((e & np.uint64(1)).astype(bool), zs, zc)
    return z.reshape(B, T), radius.reshape(B, T)


@functools.lru_cache(maxsize=256)
def _small_tensor(seed, stream, epoch, B, T, shard_offset):
    z, radius = tensor(seed, stream, epoch, B, T, shard_offset)
    z.flags.writeable = radius.flags.writeable = False     # shared among the tests: left unchanged
    return z, radius


def shared_tensor(seed, stream, epoch, B, T, shard_offset=0):
    """tensor(), computed once per case for the small shapes the tensor tests repeat."""
    if B * T > 2**19:
        return tensor(seed, stream, epoch, B, T, shard_offset)
    return _small_tensor(int(seed), stream, epoch, B, T, int(shard_offset))


def check_noise(noise, cfg, seed, epoch, label="", holonomic=True):
    """(nvx, nvy, nwz) of a context or an oracle created from cfg against tensor(), element by
    element at sigma * TENSOR_RTOL * radius; a non-holonomic model keeps vy all zero.  Returns
    (largest |delta| / sigma, the radius there, largest |delta| / (sigma radius)): see merge()."""
    B, T, off = cfg.batch_size, cfg.time_steps, cfg.shard_offset
    worst = NO_ERROR
    for name, got, stream, sigma in (("vx", noise[0], STREAM_VX, cfg.vx_std), ("vy", noise[1], STREAM_VY, cfg.vy_std),
                                     ("wz", noise[2], STREAM_WZ, cfg.wz_std)):
        assert got.shape == (B, T) and got.dtype == np.float32
        if name == "vy" and not holonomic:
            assert not got.any(), f"{label}: vy noise of a non-holonomic model"
            continue
        assert np.all(np.isfinite(got)), f"{label} {name}: not finite"
        z, radius = shared_tensor(seed, stream, epoch, B, T, off)
        radius = np.abs(radius)                      # (-0.0 at u1 == 1)
        d = np.abs(got.astype(np.float64) / sigma - z)
        i = np.unravel_index(np.argmax(d), d.shape)
        ok = d <= TENSOR_RTOL * radius
        assert np.all(ok), (f"{label} {name}: {np.count_nonzero(~ok)} of {ok.size} elements off the model, first at "
                            f"{np.argwhere(~ok)[0]}, largest |delta|/sigma {d[i]:.3e} at {i} (radius {radius[i]:.3f})")
        rel = np.where(radius > 0, d / np.maximum(radius, 1e-300), 0.0)
        worst = merge(worst, (float(d[i]), float(radius[i]), float(rel.max())))
    return worst


NO_ERROR = (0.0, 0.0, 0.0)


def merge(a, b):
    """The larger of two check_noise() results, figure by figure."""
    return max(a[:2], b[:2]) + (max(a[2], b[2]),)


def report(label, worst):
    print(f"[noise] {label}: max |delta|/sigma {worst[0]:.2e} (radius {worst[1]:.2f}), "
          f"max |delta|/(sigma radius) {worst[2]:.2e}")


K1_NAMED = (0, 1, 2, 2**23 - 1, 2**23, 2**23 + 1, 2**24 - 2, 2**24 - 1)
K2_NAMED = (0, 1, 2**22 - 1, 2**22, 2**22 + 1, 2**23 - 1, 2**23, 2**23 + 1, 3 * 2**22 - 1, 3 * 2**22,
            3 * 2**22 + 1, 2**24 - 2, 2**24 - 1)


def edge_k1():
    """u1's 24-bit integers: the smallest (radius 5.887), the first above 0.5 where k + 0.5f rounds,
    the last two (u1 just below 1, and exactly 1), and 512 distinct log-spaced ones in between."""
    # (rounding merges some of the smallest: 640 points leave more than 512 distinct, thinned evenly)
    mid = np.unique(np.round(np.geomspace(3, 2**24 - 3, 640)).astype(np.int64))
    assert mid.size >= 512
    mid = mid[np.round(np.linspace(0, mid.size - 1, 512)).astype(np.int64)]
    return np.unique(np.concatenate([np.array(K1_NAMED, np.int64), mid]))


def edge_k2():
    """u2's 24-bit integers: the angles 0, pi/2, pi, 3pi/2 and 2pi with their neighbours, and 512
    evenly spaced ones in between."""
    mid = np.round(np.linspace(0, 2**24 - 1, 514)[1:-1]).astype(np.int64)
    return np.unique(np.concatenate([np.array(K2_NAMED, np.int64), mid]))


def edge_words():
    """The directed Box-Muller table: the cross product of edge_k1() and edge_k2() as words k << 8,
    once with the discarded low byte 0x00 and once with 0xff.  Returns flat (r0, r1, k1, k2); the
    first half of each is the 0x00 copy, the second half the 0xff copy of the same pairs."""
    a, b = np.meshgrid(edge_k1(), edge_k2(), indexing="ij")
    k1, k2 = a.reshape(-1), b.reshape(-1)
    r0 = (k1 << 8).astype(np.uint32)
    r1 = (k2 << 8).astype(np.uint32)
    low = np.uint32(0xFF)
    return (np.concatenate([r0, r0 | low]), np.concatenate([r1, r1 | low]),
            np.concatenate([k1, k1]), np.concatenate([k2, k2]))


def _tail(k):
    """Q(k) = P(Z > k) of N(0, 1)."""
    return 0.5 * math.erfc(k / math.sqrt(2.0))


_BIN_EDGES = np.array([NormalDist().inv_cdf(i / 64.0) for i in range(1, 64)])


def statistics(z2d):
    """Moments, lag-1 products, tail counts (each in units of its own standard error under
    N(0, 1) i.i.d.), a chi-square over 64 equiprobable bins (63 degrees of freedom) and max |z|
    of a [B, T] float64 sample."""
    z = np.asarray(z2d, dtype=np.float64)
    B, T = z.shape
    N = z.size
    m = z.mean()
    d = z - m
    m2 = np.mean(d * d)
    m3 = np.mean(d * d * d)
    m4 = np.mean((d * d) ** 2)
    az = np.abs(z)
    out = {
        "mean": m * math.sqrt(N),
        "variance": (m2 - 1.0) / math.sqrt(2.0 / N),
        "skewness": (m3 / m2 ** 1.5) / math.sqrt(6.0 / N),
        "kurtosis": (m4 / (m2 * m2) - 3.0) / math.sqrt(24.0 / N),
    }
    if T > 1:
        out["lag1_t"] = np.mean(z[:, :-1] * z[:, 1:]) * math.sqrt(B * (T - 1))
    if B > 1:
        out["lag1_b"] = np.mean(z[:-1] * z[1:]) * math.sqrt((B - 1) * T)
    for k in (3, 4):
        expect = 2.0 * N * _tail(k)
        out[f"tail{k}"] = (np.count_nonzero(az > k) - expect) / math.sqrt(expect)
    counts = np.bincount(np.searchsorted(_BIN_EDGES, z.reshape(-1)), minlength=64)
    out["chi2"] = float(np.sum((counts - N / 64.0) ** 2) / (N / 64.0))
    out["max_abs"] = float(az.max())
    return {k: float(v) for k, v in out.items()}


def cross(a, b):
    """Product mean of two samples in units of its standard error 1 / sqrt(N)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.mean(a * b) * math.sqrt(a.size))


SE_CAP, CHI2_CAP = 5.0, 130.0   # chi2(63) exceeds 130 with probability ~1e-6


def assert_caps(stats, label=""):
    """The caps of the distribution tests: conditions, not measurements."""
    for k, v in stats.items():
        if k == "chi2":
            assert v < CHI2_CAP, f"{label}: chi2 {v}"
        elif k == "max_abs":
            assert v <= MAX_RADIUS, f"{label}: max |z| {v}"
        else:
            assert abs(v) < SE_CAP, f"{label}: {k} = {v} standard errors"
