"""No-GPU checks of the noise stream's specification (tests/noise_model.py): the integer
Philox4x32-10 of the model and of the oracle against the published known answers, the
oracle's tensors against the model, the directed Box-Muller table, and the statistics of the
model itself for the seeds the GPU distribution test uses."""
import ctypes as C
import functools

import numpy as np
import pytest

from mpcholonavigation_amd.tick import default_config
from tests import noise_model as nm
from tests.harness import Oracle  # noqa: F401


@pytest.mark.parametrize("ctr,key,expect", nm.KNOWN_ANSWERS)
def test_philox_known_answers(oracle_lib, ctr, key, expect):
    """Random123's published vectors for philox4x32 with 10 rounds, on the model and on the
    Philox the oracle draws from."""
    got = nm.philox4x32_10(np.array([ctr]), key)
    assert got.dtype == np.uint32 and got.tolist() == [list(expect)]
    c, k, out = np.array(ctr, np.uint32), np.array(key, np.uint32), np.zeros(4, np.uint32)
    oracle_lib.smpc_oracle_philox4x32_10(c.ctypes.data_as(C.c_void_p), k.ctypes.data_as(C.c_void_p),
                                         out.ctypes.data_as(C.c_void_p))
    assert out.tolist() == list(expect)


def test_oracle_philox_equals_the_model_on_random_blocks(oracle_lib):
    rng = np.random.default_rng(11)
    ctr = rng.integers(0, 2**32, (257, 4), dtype=np.uint64).astype(np.uint32)
    key = np.array([0x9abcdef0, 0x12345678], np.uint32)
    want = nm.philox4x32_10(ctr, key)
    out = np.zeros(4, np.uint32)
    for c, w in zip(ctr, want):
        c = np.ascontiguousarray(c)
        oracle_lib.smpc_oracle_philox4x32_10(c.ctypes.data_as(C.c_void_p), key.ctypes.data_as(C.c_void_p),
                                             out.ctypes.data_as(C.c_void_p))
        assert np.array_equal(out, w)


def _cases():
    for i, (B, T) in enumerate(nm.SHAPES_LANE + nm.SHAPES_PLAIN):
        yield B, T, 0, nm.SEEDS[i % len(nm.SEEDS)]
    for i, (B, T, off) in enumerate(nm.SHARDS):
        yield B, T, off, nm.SEEDS[(i + 1) % len(nm.SEEDS)]


@pytest.mark.parametrize("B,T,off,seed", list(_cases()))
def test_oracle_noise_is_the_model(Oracle, B, T, off, seed):
    """Oracle.get_noise() (float logf / sinf / cosf) against the float64 model, epochs 0 to 2
    reached with reset(): every element within sigma * 6e-7 * radius."""
    cfg = default_config(batch_size=B, time_steps=T, shard_offset=off, global_batch_size=off + B, **nm.STDS)
    o = Oracle(cfg)
    o.seed(seed)
    worst = nm.NO_ERROR
    for epoch in range(3):
        if epoch:
            o.reset()
        w = nm.check_noise(o.get_noise(), cfg, seed, epoch, label=f"oracle {B}x{T}+{off} seed {seed:#x} epoch {epoch}")
        worst = nm.merge(worst, w)
    nm.report(f"oracle {B}x{T}+{off}", worst)
    o.close()


def test_high_seed_word_and_epoch_change_the_model():
    """The model itself uses what the device tests rely on it to use: the high key word, the
    epoch, the stream and the high counter word."""
    base = nm.tensor(2024, 0, 0, 8, 64)[0]
    assert not np.array_equal(base, nm.tensor((5 << 32) | 2024, 0, 0, 8, 64)[0])
    assert not np.array_equal(base, nm.tensor(2024, 0, 1, 8, 64)[0])
    assert not np.array_equal(base, nm.tensor(2024, 1, 0, 8, 64)[0])
    # rollouts 3.. of the shard at 2^28 - 3 lie at q >= 2^32; q mod 2^32 is the start of the stream
    hi = nm.tensor(2024, 0, 0, 8, 64, shard_offset=2**28 - 3)[0]
    assert not np.array_equal(hi[3:], base[:5])
    assert np.array_equal(hi, nm.tensor(2024, 0, 0, 11, 64, shard_offset=2**28 - 6)[0][3:])


def test_edge_table():
    """The directed table holds every named edge of u1 and u2, 512 more of each, both low bytes;
    and the float32 facts the edges stand for."""
    r0, r1, k1, k2 = nm.edge_words()
    n = r0.size // 2
    s1, s2 = set(k1.tolist()), set(k2.tolist())
    assert set(nm.K1_NAMED) <= s1 and set(nm.K2_NAMED) <= s2
    assert len(s1) >= 512 + len(nm.K1_NAMED) - 2 and len(s2) >= 512
    assert n == len(s1) * len(s2) and r0.size == 2 * n             # the full cross product, twice
    assert len(set(zip(k1[:n].tolist(), k2[:n].tolist()))) == n
    assert np.array_equal(r0[:n], (k1[:n] << 8).astype(np.uint32)) and np.array_equal(r1[:n], (k2[:n] << 8).astype(np.uint32))
    assert np.array_equal(r0[n:], r0[:n] | np.uint32(0xFF)) and np.array_equal(r1[n:], r1[:n] | np.uint32(0xFF))
    assert np.array_equal(r0 >> np.uint32(8), k1.astype(np.uint32)) and np.array_equal(r1 >> np.uint32(8), k2.astype(np.uint32))
    # log-spaced: every octave of u1 between 2^-22 and 1 holds several values
    lg = np.floor(np.log2(np.array(sorted(s1 - {0}), np.float64)))
    assert all(np.count_nonzero(lg == o) >= 8 for o in range(4, 24))
    u = nm.uniforms(np.array([0, 1 << 8, (2**23) << 8, (2**23 + 1) << 8, (2**24 - 2) << 8, (2**24 - 1) << 8, 0xFFFFFFFF],
                             np.uint32))
    assert u.dtype == np.float32
    assert u[0] == np.float32(2.0**-25) and u[1] == np.float32(1.5 * 2.0**-24)
    assert u[2] == np.float32(0.5)                      # 2^23 + 0.5 is a tie: rounds to even
    assert u[3] == np.float32((2**23 + 2) * 2.0**-24)   # 2^23 + 1.5 rounds up
    assert u[4] < 1.0 and u[5] == 1.0 and u[6] == 1.0
    zc, zs, radius = nm.normals64(r0, r1)
    assert np.all(np.isfinite(zc)) and np.all(np.isfinite(zs))
    one = k1 == 2**24 - 1
    assert one.any() and np.all(np.abs(zc[one]) == 0.0) and np.all(np.abs(zs[one]) == 0.0)
    assert abs(radius[k1 == 0][0] - 5.88705) < 1e-5 and radius.max() <= nm.MAX_RADIUS
    assert abs(radius[k1 == 2**24 - 2][0] - 4.88e-4) < 1e-6
    assert np.array_equal(zc[:n], zc[n:]) and np.array_equal(zs[:n], zs[n:])


@functools.lru_cache(maxsize=None)
def _model(seed, stream, epoch):
    return nm.tensor(seed, stream, epoch, *nm.STAT_SHAPE)[0]


def test_the_fixed_seeds_keep_the_model_inside_the_caps():
    """The statistics and caps of the GPU distribution test on the model itself, for the same
    seeds: a correct stream passes them, so a device failure is the device's."""
    for seed in nm.STAT_SEEDS:
        for stream in (0, 1, 2):
            st = nm.statistics(_model(seed, stream, 0))
            print(f"[noise] model seed {seed:#x} stream {stream}: " + " ".join(f"{k} {v:+.2f}" for k, v in st.items()))
            nm.assert_caps(st, f"model seed {seed:#x} stream {stream}")
    a, b = nm.STAT_SEEDS
    cr = {"vx.wz": nm.cross(_model(a, 0, 0), _model(a, 1, 0)), "vx.vy": nm.cross(_model(a, 0, 0), _model(a, 2, 0)),
          "vx.wz (2nd seed)": nm.cross(_model(b, 0, 0), _model(b, 1, 0)),
          "vx.vy (2nd seed)": nm.cross(_model(b, 0, 0), _model(b, 2, 0)),
          "epoch 0.1": nm.cross(_model(a, 0, 0), nm.tensor(a, 0, 1, *nm.STAT_SHAPE)[0]),
          "seed.seed": nm.cross(_model(a, 0, 0), _model(b, 0, 0))}
    print("[noise] model cross products: " + " ".join(f"{k} {v:+.2f}" for k, v in cr.items()))
    for k, v in cr.items():
        assert abs(v) < nm.SE_CAP, f"{k}: {v}"
    _model.cache_clear()
