"""Acceleration limits on the sampled controls: the definition of smpc_set_acceleration_limits
(include/smpc.h) restated in NumPy float32, vectorised over the batch with a Python loop over time.
Independent of the library: the GPU tests hold smpc_limit_noise to it bit for bit.

    dhi = model_dt * {ax_max, ay_max, az_max},  dlo = model_dt * {ax_min, -ay_max, -az_max}   (float)
    last = (float) speed_k
    for t: c = u_k[t] + N_k[b][t];  ct = min(max(c, last + dlo_k), last + dhi_k)
           N'_k[b][t] = N_k[b][t] if ct == c else ct - u_k[t];  last = u_k[t] + N'_k[b][t]
"""
import numpy as np

F = np.float32


def deltas(dt, limits):
    """(dlo[3], dhi[3]) in float32, the products formed once."""
    ax_max, ax_min, ay_max, az_max = (F(v) for v in limits)
    dt = F(dt)
    dhi = [F(dt * ax_max), F(dt * ay_max), F(dt * az_max)]
    dlo = [F(dt * ax_min), F(-dhi[1]), F(-dhi[2])]
    return dlo, dhi


def limit_one(N, u, v0, dlo, dhi):
    """One control: N float32 [B, T], u float32 [T], v0 the initial speed -> N' float32 [B, T]."""
    N = np.asarray(N, F)
    u = np.asarray(u, F)
    B, T = N.shape
    out = np.empty_like(N)
    last = np.full(B, F(v0), F)
    for t in range(T):
        c = u[t] + N[:, t]
        lo = last + dlo
        hi = last + dhi
        ct = np.minimum(np.maximum(c, lo), hi)
        out[:, t] = np.where(ct == c, N[:, t], ct - u[t])
        last = u[t] + out[:, t]
    assert out.dtype == F and last.dtype == F
    return out


def limited_noise(noise, u, speed, dt, limits, holonomic=True):
    """noise: (nvx, nvy, nwz) [B, T] each; u [3, T]; speed (vx, vy, wz) of the tick.
    A non-holonomic model: vy is not touched and comes back as the zeros the library stores."""
    dlo, dhi = deltas(dt, limits)
    u = np.asarray(u, F)
    out = []
    for k in range(3):
        if k == 1 and not holonomic:
            out.append(np.zeros_like(np.asarray(noise[1], F)))
            continue
        out.append(limit_one(noise[k], u[k], F(speed[k]), dlo[k], dhi[k]))
    return out
