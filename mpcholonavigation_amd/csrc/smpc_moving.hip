// smpc_moving.hip — smpc_moving_cost: the moving-obstacle term of one iteration.
//
// One launch per iteration, in front of its scoring passes, scores K discs whose centres move with
// the trajectory index against every rollout of the context and writes the result where the passes
// read their starting cost (SmpcDev::costs_prev under SD_COST_SEED).  Per rollout b, with the
// trajectory points (x[t], y[t]) the passes form (noised controls, v[:,0] = speed, float cumulative
// sums, x = (float)(x0 + (double)cumsum), smpc_sincos), all in float (-ffp-contract=off):
//   d  = sqrtf(dx dx + dy dy)                      dx = x[t] - cx[k][t], dy = y[t] - cy[k][t]
//   q  = min(max((radius[k] + margin - d) / margin, 0), 1)
//   m  = (float)(repulsion_weight (sum over t, k of q) / T + (any d < radius[k] ? collision_cost : 0))
// (the last line in double, once per rollout).  Iteration 0 stores m; a later iteration adds it to
// the costs the iteration before left there, (float)((double)cost + m).  A module of its own, like
// smpc_limit.hip: the resource usage of the scoring passes does not move.
//
// A term whose squared distance is at or beyond the guarded squared reach (smpc_moving.h) is exactly
// 0 and takes no square root; a wave none of whose lanes is inside skips the rest of the term.
//
// Two forms, for the two layouts of the noise:
//   group-major quads [B/64][T4/4][64][4] (SMPC_GM_INDEX): lane = rollout, sequential in time as the
//     lane-per-rollout pass walks it; one 16-byte load per tensor and quad, the next quad's loads
//     issued before the current quad's steps; u in LDS; the step's K table entries {x, y, guarded
//     squared reach, radius} are wave-uniform 16-byte reads of one contiguous run.
//   row-major [B,T]: wave = rollout, lane = R = ceil(T / 64) steps, positions by the DPP scans of
//     smpc_wave_common.h exactly as smpc_wave_pass.inc forms them; each lane walks the K discs of
//     its steps, the table read [k][t] (a wave's read of one disc is one run), wave_sum of q and a
//     ballot for the hit.
// The two sum q in different orders: they agree within rounding, not bit for bit.
#include <hip/hip_runtime.h>

#include "smpc_dev.h"
#include "smpc_device_math.h"
#include "smpc_moving.h"
#include "smpc_wave_common.h"

namespace {

// u of the iteration: device memory (a later iteration) or this launch's own kernel arguments
__device__ __forceinline__ const float* moving_u(const SmpcMovingArgs& p)
{
#if defined(__HIP_DEVICE_COMPILE__)
  if (!p.u_dev)
    return reinterpret_cast<const float*>(reinterpret_cast<const uint8_t*>(__builtin_amdgcn_kernarg_segment_ptr()) +
                                          __builtin_offsetof(SmpcMovingArgs, u_arg));
#endif
  return p.u_dev;
}

// one disc at one trajectory point; `reach`: radius + margin as the host formed it in float
__device__ __forceinline__ void moving_term(float d2, float radius, float reach, float margin, float& sum, bool& hit)
{
  const float d = sqrtf(d2);
  const float q = fminf(fmaxf((reach - d) / margin, 0.f), 1.f);
  sum += q;
  hit = hit || d < radius;
}

__device__ __forceinline__ void moving_store(const SmpcMovingArgs& p, uint32_t b, float sum, bool hit)
{
  const float m = (float)((double)p.repulsion_weight * (double)sum / (double)p.T + (hit ? (double)p.collision_cost : 0.0));
  p.seed[b] = p.add ? (float)((double)p.seed[b] + (double)m) : m;
  if (p.m_out) p.m_out[b] = m;
  if (p.hit_out) p.hit_out[b] = hit ? 1 : 0;
}

}  // namespace

// Group-major form.  A wave takes one group of 64 rollouts, a block four groups.
template <bool VY>
__global__ void __launch_bounds__(256) smpc_moving_cost_gm(const SmpcMovingArgs p)
{
  __shared__ float4 su4[3 * SMPC_MOVING_MAX_T / 4];   // u in quads [3][T4 / 4], zeros in the padding steps
  float* su = reinterpret_cast<float*>(su4);
  const uint32_t T = p.T, T4 = SMPC_GM_STEPS(T), Q = T4 >> 2, K = p.K;
  {
    const float* u = moving_u(p);
    for (uint32_t i = threadIdx.x; i < 3 * T4; i += 256) {
      const uint32_t k = i / T4, t = i - k * T4;
      su[i] = t < T ? u[k * T + t] : 0.f;
    }
  }
  __syncthreads();
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t g = blockIdx.x * 4u + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (g >= (p.B + 63u) / 64u) return;
  const uint32_t b = g * 64u + lane;
  const size_t at = static_cast<size_t>(g) * Q * 64u + lane;   // in quads; the next quad of the lane is 64 further
  const float4* __restrict__ s0 = reinterpret_cast<const float4*>(p.n[0]) + at;
  const float4* __restrict__ s1 = reinterpret_cast<const float4*>(p.n[VY ? 1 : 0]) + at;
  const float4* __restrict__ s2 = reinterpret_cast<const float4*>(p.n[2]) + at;
  const float4* __restrict__ tab = reinterpret_cast<const float4*>(p.tab);
  const float dt = p.dt, yaw0 = p.yaw0, margin = p.margin;
  const double x0 = p.x0, y0 = p.y0;
  float cpx = p.v0[0], cpy = VY ? p.v0[1] : 0.f, cpz = p.v0[2];   // v[:,0] = measured speed, v[:,t] = c[:,t-1]
  float acc_yaw = 0.f, ax = 0.f, ay = 0.f;
  float cs_prev = p.cos0, sn_prev = p.sin0;
  float sum = 0.f;
  bool hit = false;
  // one time step for the 64 rollouts of this wave, as the lane-per-rollout pass takes it
  auto step = [&](uint32_t t, float ux, float uy, float uz, float n0, float n1, float n2) {
    const float cvx = ux + n0, cvy = VY ? uy + n1 : 0.f, cwz = uz + n2;
    const float vx = cpx, vy = cpy, wz = cpz;
    cpx = cvx; cpy = cvy; cpz = cwz;
    acc_yaw = acc_yaw + wz * dt;
    const float yaw = acc_yaw + yaw0;
    const float dxr = VY ? vx * cs_prev - vy * sn_prev : vx * cs_prev;
    const float dyr = VY ? vx * sn_prev + vy * cs_prev : vx * sn_prev;
    ax = ax + dxr * dt;
    ay = ay + dyr * dt;
    smpc_sincos(yaw, sn_prev, cs_prev);
    const float x = (float)(x0 + (double)ax), y = (float)(y0 + (double)ay);
    const float4* __restrict__ row = tab + static_cast<size_t>(t) * K;
    for (uint32_t k = 0; k < K; ++k) {
      const float4 o = row[k];   // wave-uniform: {x, y, guarded squared reach, radius}
      const float dx = x - o.x, dy = y - o.y;
      const float d2 = dx * dx + dy * dy;
      if (__builtin_amdgcn_ballot_w64(d2 < o.z) != 0) moving_term(d2, o.w, o.w + margin, margin, sum, hit);
    }
  };
  float4 n0 = s0[0], n1 = VY ? s1[0] : make_float4(0.f, 0.f, 0.f, 0.f), n2 = s2[0];
  for (uint32_t q = 0; q < Q; ++q) {
    float4 m0 = n0, m1 = n1, m2 = n2;
    if (q + 1 < Q) {
      const size_t o = static_cast<size_t>(q + 1) * 64u;
      m0 = s0[o];
      if (VY) m1 = s1[o];
      m2 = s2[o];
    }
    const float4 ux = su4[q], uy = su4[Q + q], uz = su4[2u * Q + q];
    const uint32_t t0 = 4u * q;   // (t0 < T always: T4 - 4 < T)
    step(t0, ux.x, uy.x, uz.x, n0.x, n1.x, n2.x);
    if (t0 + 1 < T) step(t0 + 1, ux.y, uy.y, uz.y, n0.y, n1.y, n2.y);
    if (t0 + 2 < T) step(t0 + 2, ux.z, uy.z, uz.z, n0.z, n1.z, n2.z);
    if (t0 + 3 < T) step(t0 + 3, ux.w, uy.w, uz.w, n0.w, n1.w, n2.w);
    n0 = m0; n1 = m1; n2 = m2;
  }
  if (b < p.B) moving_store(p, b, sum, hit);   // (padding rollouts of the last group: zero noise, scored, never stored)
}

// Row-major form.  A wave takes one rollout, a block four; lane l owns steps l R .. l R + R - 1.
template <int R>
__global__ void __launch_bounds__(256) smpc_moving_cost_rm(const SmpcMovingArgs p)
{
  const uint32_t T = p.T, K = p.K;
  const int lane = threadIdx.x & (WAVE - 1);
  const uint32_t b = blockIdx.x * 4u + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (b >= p.B) return;   // (the whole wave: every lane of the others stays active for the scans)
  const int t0 = lane * R;
#define STEP_OK(r) ((uint32_t)(t0 + (r)) < T)
  const float* u = moving_u(p);
  const size_t row = static_cast<size_t>(b) * T;
  float cvx[R], cvy[R], cwz[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const bool a = STEP_OK(r);
    // NoiseGenerator::setNoisedControls: c = u + noise (vy of a non-holonomic model: none)
    cvx[r] = a ? u[t0 + r] + p.n[0][row + t0 + r] : 0.f;
    cvy[r] = (a && p.n[1]) ? u[T + t0 + r] + p.n[1][row + t0 + r] : 0.f;
    cwz[r] = a ? u[2 * T + t0 + r] + p.n[2][row + t0 + r] : 0.f;
  }
  const float dt = in_vgpr(p.dt), yaw0_v = in_vgpr(p.yaw0);
  const double x0_v = in_vgpr(p.x0), y0_v = in_vgpr(p.y0);
  const float first_vx = lane == 0 ? p.v0[0] : 0.f, first_vy = lane == 0 ? p.v0[1] : 0.f;
  const float first_wz = lane == 0 ? p.v0[2] : 0.f;
  const float first_cos = lane == 0 ? p.cos0 : 0.f, first_sin = lane == 0 ? p.sin0 : 0.f;
  // ---- updateStateVelocities + predict: v[:,0]=speed, v[:,1:]=c[:,:-1] (smpc_wave_pass.inc) ---
  float vx[R], vy[R], wz[R];
  vx[0] = dpp_shr1_add(cvx[R - 1], first_vx);
  vy[0] = dpp_shr1_add(cvy[R - 1], first_vy);
  wz[0] = dpp_shr1_add(cwz[R - 1], first_wz);
#pragma unroll
  for (int r = 1; r < R; ++r) {
    vx[r] = cvx[r - 1];
    vy[r] = cvy[r - 1];
    wz[r] = cwz[r - 1];
  }
#pragma unroll
  for (int r = 0; r < R; ++r) {
    if (!STEP_OK(r)) vx[r] = vy[r] = wz[r] = 0.f;
  }
  // ---- integrateStateVelocities ------------------------------------------------------------
  float yaw[R];
  {
    float acc = wz[0] * dt;
    yaw[0] = acc;
#pragma unroll
    for (int r = 1; r < R; ++r) {
      acc += wz[r] * dt;
      yaw[r] = acc;
    }
    const float incl = wave_scan_add(acc);
    if (R == 1) {
      yaw[0] = incl + yaw0_v;
    } else {
#pragma unroll
      for (int r = 0; r < R; ++r) yaw[r] = dpp_shr1_add(incl, yaw[r]) + yaw0_v;
    }
  }
  float x[R], y[R];
  {
    float sn[R], cs[R];
#pragma unroll
    for (int r = 0; r < R; ++r) smpc_sincos(yaw[r], sn[r], cs[r]);
    float c_prev = dpp_shr1_add(cs[R - 1], first_cos);
    float s_prev = dpp_shr1_add(sn[R - 1], first_sin);
    float ax = 0.f, ay = 0.f;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const float dxr = vx[r] * c_prev - vy[r] * s_prev;
      const float dyr = vx[r] * s_prev + vy[r] * c_prev;
      ax = (r == 0) ? dxr * dt : ax + dxr * dt;
      ay = (r == 0) ? dyr * dt : ay + dyr * dt;
      x[r] = ax;
      y[r] = ay;
      c_prev = cs[r];
      s_prev = sn[r];
    }
    float sx = ax, sy = ay;
    wave_scan_add2(sx, sy);
    if (R == 1) {
      x[0] = (float)(x0_v + (double)sx);
      y[0] = (float)(y0_v + (double)sy);
    } else {
#pragma unroll
      for (int r = 0; r < R; ++r) {
        x[r] = (float)(x0_v + (double)dpp_shr1_add(sx, x[r]));
        y[r] = (float)(y0_v + (double)dpp_shr1_add(sy, y[r]));
      }
    }
  }
  // ---- the discs: lane = its steps, the table read [k][t] ----------------------------------
  const float2* __restrict__ tab = reinterpret_cast<const float2*>(p.tab);
  const float4* __restrict__ disc = reinterpret_cast<const float4*>(p.disc);
  const float margin = p.margin;
  float sum = 0.f;
  bool hit = false;
  for (uint32_t k = 0; k < K; ++k) {
    const float4 dk = disc[k];   // wave-uniform: {radius, radius + margin, guarded squared reach, 0}
#pragma unroll
    for (int r = 0; r < R; ++r) {
      float d2 = 3.0e38f;   // (a step past the horizon: out of every reach)
      if (STEP_OK(r)) {
        const float2 o = tab[static_cast<size_t>(k) * T + t0 + r];
        const float dx = x[r] - o.x, dy = y[r] - o.y;
        d2 = dx * dx + dy * dy;
      }
      if (d2 < dk.z) moving_term(d2, dk.x, dk.y, margin, sum, hit);
    }
  }
#undef STEP_OK
  const float total = wave_sum(sum);
  const bool any_hit = __builtin_amdgcn_ballot_w64(hit) != 0;
  if (lane == 0) moving_store(p, b, total, any_hit);
}

hipError_t smpc_launch_moving_cost(const SmpcMovingArgs& a, bool group_major, hipStream_t st)
{
  static_assert(sizeof(SmpcMovingArgs) <= 4096, "the arguments travel in the kernel argument segment");
  if (a.B == 0 || a.T == 0 || a.T > SMPC_MOVING_MAX_T || a.K == 0 || a.K > SMPC_MOVING_MAX_K) return hipErrorInvalidValue;
  if (group_major) {
    const uint32_t groups = (a.B + 63u) / 64u;
    const dim3 grid((groups + 3u) / 4u);
    if (a.n[1]) hipLaunchKernelGGL(smpc_moving_cost_gm<true>, grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL(smpc_moving_cost_gm<false>, grid, dim3(256), 0, st, a);
    return hipGetLastError();
  }
  const dim3 grid((a.B + 3u) / 4u);
  if (a.T <= 64u) hipLaunchKernelGGL(smpc_moving_cost_rm<1>, grid, dim3(256), 0, st, a);
  else if (a.T <= 128u) hipLaunchKernelGGL(smpc_moving_cost_rm<2>, grid, dim3(256), 0, st, a);
  else hipLaunchKernelGGL(smpc_moving_cost_rm<4>, grid, dim3(256), 0, st, a);
  return hipGetLastError();
}
