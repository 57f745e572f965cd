"""Acceleration limits, without a GPU: the model of tests/accel_model.py against the properties the
definition promises, and the new entry points' symbols and device-free refusals."""
import ctypes as C
import os

import numpy as np
import pytest

from mpcholonavigation_amd import _abi as A
from mpcholonavigation_amd.synthetic import make_noise
from tests import accel_model as am

DT = 0.05
UPSTREAM = (3.0, -3.0, 3.0, 3.5)
SPEED = (0.25, 0.05, -0.1)


def inputs(B=512, T=56, seed=7):
    noise = make_noise(B, T, std=(0.2, 0.2, 0.4), seed=seed)
    t = np.arange(T, dtype=np.float32)
    u = np.stack([0.3 - 0.002 * t, 0.05 * np.sin(0.3 * t), 0.2 * np.cos(0.2 * t)]).astype(np.float32)
    return noise, u


def test_wide_limits_change_nothing():
    noise, u = inputs()
    out = am.limited_noise(noise, u, SPEED, DT, (1e6, -1e6, 1e6, 1e6))
    for a, b in zip(out, noise):
        assert a.dtype == np.float32 and np.array_equal(a.view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


def test_upstream_limits_bind_on_a_substantial_share():
    """The scene the GPU tests limit: at least 10 % of the elements change, per control."""
    noise, u = inputs()
    out = am.limited_noise(noise, u, SPEED, DT, UPSTREAM)
    for k, (a, b) in enumerate(zip(out, noise)):
        share = float(np.mean(a != b))
        print(f"[accel model] control {k}: {100 * share:.1f} % of the elements limited")
        assert share >= 0.10, (k, share)


@pytest.mark.parametrize("limits", [UPSTREAM, (3.0, -1.0, 3.0, 3.5), (0.5, -4.0, 1.0, 0.7)])
def test_realised_steps_lie_within_the_bounds(limits):
    """c'[t] = fl(u[t] + N'[t]) against last = c'[t - 1] (the speed at t = 0): the step lies in
    [dlo, dhi] widened by 2^-22 (|u| + |N'| + |last| + |d|) — three roundings of 2^-24 each (the
    bound, the subtraction, the re-add), the margin loose on purpose."""
    noise, u = inputs()
    out = am.limited_noise(noise, u, SPEED, DT, limits)
    dlo, dhi = am.deltas(DT, limits)
    for k in range(3):
        N = out[k]
        c = (u[k][None, :] + N).astype(np.float32)
        last = np.concatenate([np.full((N.shape[0], 1), np.float32(SPEED[k]), np.float32), c[:, :-1]], axis=1)
        step = c.astype(np.float64) - last.astype(np.float64)
        mag = np.abs(u[k][None, :].astype(np.float64)) + np.abs(N.astype(np.float64)) + np.abs(last.astype(np.float64))
        m_lo = 2.0 ** -22 * (mag + abs(float(dlo[k])))
        m_hi = 2.0 ** -22 * (mag + abs(float(dhi[k])))
        assert np.all(step >= float(dlo[k]) - m_lo), k
        assert np.all(step <= float(dhi[k]) + m_hi), k


def test_ax_min_is_honoured_asymmetrically():
    noise, u = inputs()
    out = am.limited_noise(noise, u, SPEED, DT, (3.0, -1.0, 3.0, 3.5))
    c = (u[0][None, :] + out[0]).astype(np.float32)
    last = np.concatenate([np.full((c.shape[0], 1), np.float32(SPEED[0]), np.float32), c[:, :-1]], axis=1)
    step = c.astype(np.float64) - last.astype(np.float64)
    # decelerations stop at 0.05 m/s per step, accelerations reach beyond it up to 0.15
    assert step.min() >= -0.05 - 1e-6 and step.min() <= -0.05 + 1e-6
    assert step.max() > 0.14 and step.max() <= 0.15 + 1e-6
    sym = am.limited_noise(noise, u, SPEED, DT, (3.0, -3.0, 3.0, 3.5))
    assert not np.array_equal(sym[0], out[0])
    assert np.array_equal(sym[1], out[1]) and np.array_equal(sym[2], out[2])


def test_non_holonomic_vy_is_untouched():
    noise, u = inputs(64, 12)
    out = am.limited_noise(noise, u, SPEED, DT, UPSTREAM, holonomic=False)
    assert not out[1].any()


def test_symbols_are_exported_and_bound():
    from mpcholonavigation_amd.optimizer import LIB_PATH, Smpc
    lib = A.bind(C.CDLL(LIB_PATH))
    for name in ("smpc_set_acceleration_limits", "smpc_get_acceleration_limits", "smpc_get_limited_noise"):
        assert name in A.PROTOTYPES and hasattr(lib, name), name
    for m in ("set_acceleration_limits", "get_acceleration_limits", "get_limited_noise"):
        assert callable(getattr(Smpc, m))
    # the refusals that need no device: a null context
    assert lib.smpc_set_acceleration_limits(None, 3.0, -3.0, 3.0, 3.5) == A.SMPC_ERR_INVALID
    assert lib.smpc_get_acceleration_limits(None, (C.c_float * 4)()) == A.SMPC_ERR_INVALID
    assert lib.smpc_get_limited_noise(None, None, None, None) == A.SMPC_ERR_INVALID


def test_host_face_has_the_setter():
    from mpcholonavigation_amd import host_optimizer as H
    host = C.CDLL(os.path.join(os.path.dirname(H.__file__), "libsortham_host.so"))
    assert hasattr(host, "sortham_optimizer_set_acceleration_limits")
    assert callable(H.Optimizer.set_acceleration_limits)
    assert host.sortham_optimizer_set_acceleration_limits(None, C.c_float(3), C.c_float(-3), C.c_float(3),
                                                          C.c_float(3.5)) == A.SMPC_ERR_INVALID
