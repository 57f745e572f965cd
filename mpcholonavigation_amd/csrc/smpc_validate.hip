// smpc_validate.hip — smpc_validate: the collision check of a control sequence's own trajectory
// (include/smpc.h: smpc_validate_trajectory, smpc_group_validate_trajectories).
//
// One kernel text serves one context and a group: blockIdx.x is the member, its arguments
// (SmpcValidateArgs) come from device memory, a thread is a trajectory point (T <= 256).  Per member:
//   poses   integrateControlSequence (host/optimizer.cpp): the sequence ITSELF integrated from the
//           pose — no measured-speed first column — in float, yaw[t] = sum(wz dt)[0..t] + yaw0,
//           dx = vx cos(yaw[t-1]) - vy sin(yaw[t-1]), x[t] = (float)(x0 + (double)sum(dx dt)[0..t]),
//           every product and sum rounded on its own (-ffp-contract=off).  The sums run in the
//           host's order: every thread adds the terms 0 .. t front to back out of LDS (a broadcast
//           read per term; T terms, a few microseconds), so a pose differs from the host's only by
//           the device's sinf / cosf.
//   costmap CostCritic's rule on point t < n_check: the centre cell by cell_index_exact (off the
//           map: 255), below 1 free; with consider_footprint a centre cost at or above the
//           possibly-inscribed cost (or that cost below 1) is replaced by the footprint cost at the
//           pose (smpc_footprint_walk.inc, its third compilation: the parameter block is
//           SmpcValidateArgs, the LDS window of zero size, every cell read from the global map);
//           254 collides, 253 unless consider_footprint, 255 unless the costmap tracks unknown.
//   discs   pose t hits disc k iff sqrtf(dx dx + dy dy) < radius[k], against the table's entry t.
//   result  the least colliding t by a ballot per wave and four words of LDS; that thread writes the
//           struct, thread 0 when nothing collides.
// The struct and the poses go straight to host memory mapped into the device: the host reads them
// after its one wait, no copy back.  A module of its own: no scoring pass's registers move.
#include <hip/hip_runtime.h>

#include "smpc_device_math.h"
#include "smpc_validate.h"

#define SMPC_FP_DEV SmpcValidateArgs
#define SMPC_FP_ATTR __forceinline__
#define SMPC_FP_NAME(name) name##_val
#include "smpc_footprint_walk.inc"
#undef SMPC_FP_ATTR
#undef SMPC_FP_NAME
#undef SMPC_FP_DEV

namespace {

// s[0] + s[1] + ... + s[t], added front to back as a host loop adds them (t >= T: the whole sum)
__device__ __forceinline__ float sum_in_order(const float* s, uint32_t t, uint32_t T)
{
  float acc = s[0];
  for (uint32_t i = 1; i < T; ++i) {
    const float v = s[i];   // the same address for every lane: one broadcast read
    if (i <= t) acc = acc + v;
  }
  return acc;
}

}  // namespace

__global__ void __launch_bounds__(SMPC_VALIDATE_BLOCK) smpc_validate(const SmpcValidateArgs* __restrict__ many)
{
  const SmpcValidateArgs& p = many[blockIdx.x];
  __shared__ float s_a[SMPC_VALIDATE_MAX_T], s_b[SMPC_VALIDATE_MAX_T];
  __shared__ uint32_t s_first[SMPC_VALIDATE_BLOCK / 64];
  __shared__ uint8_t s_map[16];   // the walk's window: of zero size, but its element 0 is always read
  const uint32_t t = threadIdx.x, T = p.T;   // (the host: 1 <= T <= SMPC_VALIDATE_MAX_T)
  const bool live = t < T;
  const float dt = p.dt, yaw0 = p.yaw0;
  float vx = 0.f, vy = 0.f, wz = 0.f;
  if (live) {
    vx = p.u[t];
    if (p.holonomic) vy = p.u[T + t];
    wz = p.u[2u * T + t];
    s_a[t] = wz * dt;
  }
  if (t < 16u) s_map[t] = 0;
  __syncthreads();
  const float yaw = sum_in_order(s_a, t, T) + yaw0;
  if (live) s_b[t] = yaw;
  __syncthreads();
  {
    const float prev = t == 0u ? yaw0 : s_b[live ? t - 1u : 0u];
    float sn, cs;
    sincosf(prev, &sn, &cs);
    float dx = vx * cs, dy = vx * sn;
    if (p.holonomic) {
      dx = dx - vy * sn;
      dy = dy + vy * cs;
    }
    __syncthreads();   // (everybody has read its s_b)
    if (live) {
      s_a[t] = dx * dt;
      s_b[t] = dy * dt;
    }
  }
  __syncthreads();
  const float x = (float)(p.x0 + (double)sum_in_order(s_a, t, T));
  const float y = (float)(p.y0 + (double)sum_in_order(s_b, t, T));
  if (live && p.xyyaw) {
    p.xyyaw[3u * t + 0u] = x;
    p.xyyaw[3u * t + 1u] = y;
    p.xyyaw[3u * t + 2u] = yaw;
  }
  // ---- the checks of point t ----
  uint32_t cause = 0u, disc = 0u;
  float cost = 0.f;
  if (t < p.n_check) {
    uint32_t mx = 0u, my = 0u;
    bool on = cell_index_exact((double)x, p.ox, p.res, p.W, mx);
    on = cell_index_exact((double)y, p.oy, p.res, p.H, my) && on;
    const uint32_t c = on ? p.map[(size_t)my * p.W + mx] : 255u;
    if (c >= 1u) {
      cost = (float)c;
      if (p.consider_footprint && (cost >= p.fp_pic || p.fp_pic < 1.0f))
        cost = footprint_cost_at_pose_val(p, s_map, x, y, yaw);
      if (cost == 254.0f || (cost == 253.0f && !p.consider_footprint) || (cost == 255.0f && !p.track_unknown)) cause = 1u;
    }
    const float2* __restrict__ tab = reinterpret_cast<const float2*>(p.tab_kt);
    for (uint32_t k = 0; k < p.K; ++k) {
      const float2 o = tab[(size_t)k * T + t];
      const float ex = x - o.x, ey = y - o.y;
      const float d = sqrtf(ex * ex + ey * ey);
      if (d < p.disc[4u * k]) {   // {radius, radius + margin, guarded squared reach, 0}
        disc = k;
        if (!cause) cause = 2u;
        break;
      }
    }
  }
  // ---- the least colliding point ----
  const unsigned long long bad = __ballot(cause != 0u);
  if ((t & 63u) == 0u) s_first[t >> 6] = bad ? (t + (uint32_t)__ffsll((long long)bad) - 1u) : 0xffffffffu;
  __syncthreads();
  uint32_t first = s_first[0];
#pragma unroll
  for (uint32_t w = 1; w < SMPC_VALIDATE_BLOCK / 64; ++w) first = min(first, s_first[w]);
  smpc_validation r;
  r.valid = first == 0xffffffffu ? 1 : 0;
  r.checked = p.n_check;
  r.first_bad = r.valid ? 0u : first;
  r.cause = cause;
  r.disc = disc;
  r.cost = cost;
  if (r.valid) {
    r.cause = 0u;
    r.disc = 0u;
    r.cost = 0.f;
    if (t == 0u) *p.out = r;
  } else if (t == first) {
    *p.out = r;
  }
}

hipError_t smpc_launch_validate(const SmpcValidateArgs* d_many, uint32_t count, hipStream_t st)
{
  if (count == 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(smpc_validate, dim3(count), dim3(SMPC_VALIDATE_BLOCK), 0, st, d_many);
  return hipGetLastError();
}
