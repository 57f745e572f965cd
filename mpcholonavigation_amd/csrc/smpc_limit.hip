// smpc_limit.hip — smpc_limit_noise: acceleration limits on the sampled controls.
//
// One launch per iteration, in front of its scoring passes, turns the stored noise N into the
// LIMITED noise N' the passes then read in N's place.  Per rollout b and control k, sequentially
// over t, all in float (the build has -ffp-contract=off and no fast-math: (u + N) - u stays):
//   last = v0_k
//   c  = u_k[t] + N_k[b][t]                    what the passes form
//   ct = min(max(c, last + dlo_k), last + dhi_k)
//   N'_k[b][t] = (ct == c) ? N_k[b][t] : ct - u_k[t]
//   last = u_k[t] + N'_k[b][t]                 the control the scoring pass realises
// Where no limit binds N' is N bit for bit.  A module of its own, like smpc_wave_many.hip: the
// resource usage of the scoring passes does not move.
//
// One lane per rollout, sequential in time, in the two layouts the passes read:
//   group-major quads [B/64][T4/4][64][4] (SMPC_GM_INDEX): a lane's quad is one 16-byte load and one
//     16-byte store per tensor, a wave's quad 1 KB contiguous; the next quad's loads are issued
//     before the current quad's recursion (they do not depend on it);
//   row-major [B,T]: a tile of 64 rollouts is one contiguous run of 64 T floats — staged through LDS
//     with coalesced 16-byte loads, walked by one lane per row at an odd row stride (conflict-free),
//     written back the same way.
// Both stream every tensor once in and once out: 24 B T bytes with three tensors, 16 B T with two.
#include <hip/hip_runtime.h>

#include "smpc_dev.h"
#include "smpc_limit.h"

namespace {

__device__ __forceinline__ float limit_step(float u, float n, float& last, float dlo, float dhi)
{
  const float c = u + n;
  const float lo = last + dlo, hi = last + dhi;
  const float ct = fminf(fmaxf(c, lo), hi);
  const float out = (ct == c) ? n : ct - u;
  last = u + out;
  return out;
}

// u of the iteration: device memory (a later iteration) or this launch's own kernel arguments
__device__ __forceinline__ const float* limit_u(const SmpcLimitArgs& p)
{
#if defined(__HIP_DEVICE_COMPILE__)
  if (!p.u_dev)
    return reinterpret_cast<const float*>(reinterpret_cast<const uint8_t*>(__builtin_amdgcn_kernarg_segment_ptr()) +
                                          __builtin_offsetof(SmpcLimitArgs, u_arg));
#endif
  return p.u_dev;
}

// one quad of one tensor: steps 4q .. 4q + 3 (padding steps and padding rollouts: zeros, never consumed)
__device__ __forceinline__ float4 limit_quad(const float4 u, const float4 n, uint32_t t0, uint32_t T, bool live, float& last,
                                             float dlo, float dhi)
{
  float4 o;
  o.x = limit_step(u.x, n.x, last, dlo, dhi);   // (t0 < T always: T4 - 4 < T)
  o.y = t0 + 1 < T ? limit_step(u.y, n.y, last, dlo, dhi) : 0.f;
  o.z = t0 + 2 < T ? limit_step(u.z, n.z, last, dlo, dhi) : 0.f;
  o.w = t0 + 3 < T ? limit_step(u.w, n.w, last, dlo, dhi) : 0.f;
  return live ? o : make_float4(0.f, 0.f, 0.f, 0.f);
}

}  // namespace

// Group-major form.  A wave takes one group of 64 rollouts, a block four groups.
template <bool VY>
__global__ void __launch_bounds__(256) smpc_limit_noise_gm(const SmpcLimitArgs p)
{
  __shared__ float4 su4[3 * SMPC_LIMIT_MAX_T / 4];   // u in quads [3][T4 / 4], zeros in the padding steps
  float* su = reinterpret_cast<float*>(su4);
  const uint32_t T = p.T, T4 = SMPC_GM_STEPS(T), Q = T4 >> 2;
  {
    const float* u = limit_u(p);
    for (uint32_t i = threadIdx.x; i < 3 * T4; i += 256) {
      const uint32_t k = i / T4, t = i - k * T4;
      su[i] = t < T ? u[k * T + t] : 0.f;
    }
  }
  __syncthreads();
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t g = blockIdx.x * 4u + (threadIdx.x >> 6);
  if (g >= (p.B + 63u) / 64u) return;
  const bool live = g * 64u + lane < p.B;
  const size_t at = static_cast<size_t>(g) * Q * 64u + lane;   // in quads; the next quad of the lane is 64 further
  const float4* __restrict__ s0 = reinterpret_cast<const float4*>(p.src[0]) + at;
  const float4* __restrict__ s1 = reinterpret_cast<const float4*>(p.src[VY ? 1 : 0]) + at;
  const float4* __restrict__ s2 = reinterpret_cast<const float4*>(p.src[2]) + at;
  float4* __restrict__ d0 = reinterpret_cast<float4*>(p.dst[0]) + at;
  float4* __restrict__ d1 = reinterpret_cast<float4*>(p.dst[VY ? 1 : 0]) + at;
  float4* __restrict__ d2 = reinterpret_cast<float4*>(p.dst[2]) + at;
  float l0 = p.v0[0], l1 = p.v0[1], l2 = p.v0[2];
  float4 n0 = s0[0], n1 = VY ? s1[0] : make_float4(0.f, 0.f, 0.f, 0.f), n2 = s2[0];
  for (uint32_t q = 0; q < Q; ++q) {
    float4 m0 = n0, m1 = n1, m2 = n2;
    if (q + 1 < Q) {
      const size_t o = static_cast<size_t>(q + 1) * 64u;
      m0 = s0[o];
      if (VY) m1 = s1[o];
      m2 = s2[o];
    }
    const size_t o = static_cast<size_t>(q) * 64u;
    d0[o] = limit_quad(su4[q], n0, 4u * q, T, live, l0, p.dlo[0], p.dhi[0]);
    if (VY) d1[o] = limit_quad(su4[Q + q], n1, 4u * q, T, live, l1, p.dlo[1], p.dhi[1]);
    d2[o] = limit_quad(su4[2u * Q + q], n2, 4u * q, T, live, l2, p.dlo[2], p.dhi[2]);
    n0 = m0; n1 = m1; n2 = m2;
  }
}

// Row-major form.  blockIdx.x: a tile of 64 rollouts; blockIdx.y: the tensor (vx, [vy,] wz).
// Dynamic LDS: the tile [64][stride] at an odd stride, then u of this control [T].
__global__ void __launch_bounds__(256) smpc_limit_noise_rm(const SmpcLimitArgs p)
{
  extern __shared__ __attribute__((aligned(16))) float lds_limit[];
  const uint32_t T = p.T, stride = T | 1u;
  float* tile = lds_limit;
  float* su = lds_limit + 64u * stride;
  const uint32_t k = p.src[1] ? blockIdx.y : 2u * blockIdx.y;   // (no vy tensor: the second tensor is wz)
  const uint32_t b0 = blockIdx.x * 64u;
  const uint32_t rows = min(64u, p.B - b0), n = rows * T;
  const float* __restrict__ src = p.src[k] + static_cast<size_t>(b0) * T;   // 256 T bytes into the tensor: 16-byte aligned
  float* __restrict__ dst = p.dst[k] + static_cast<size_t>(b0) * T;
  {
    const float* u = limit_u(p) + k * T;
    for (uint32_t t = threadIdx.x; t < T; t += 256) su[t] = u[t];
  }
  for (uint32_t i = threadIdx.x; i < (n >> 2); i += 256) {
    const float4 v = reinterpret_cast<const float4*>(src)[i];
    const float e4[4] = {v.x, v.y, v.z, v.w};
    uint32_t r = 4u * i / T, c = 4u * i - r * T;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      tile[r * stride + c] = e4[j];
      if (++c == T) {c = 0; ++r;}
    }
  }
  for (uint32_t e = (n & ~3u) + threadIdx.x; e < n; e += 256) {
    const uint32_t r = e / T, c = e - r * T;
    tile[r * stride + c] = src[e];
  }
  __syncthreads();
  if (threadIdx.x < rows) {
    float* row = tile + threadIdx.x * stride;
    float last = p.v0[k];
    const float dlo = p.dlo[k], dhi = p.dhi[k];
    // eight steps' reads issued together: the recursion waits for LDS once per eight steps, not per step
    for (uint32_t t0 = 0; t0 < T; t0 += 8) {
      float n[8], uu[8];
#pragma unroll
      for (uint32_t j = 0; j < 8; ++j) {
        const uint32_t t = min(t0 + j, T - 1u);
        n[j] = row[t];
        uu[j] = su[t];
      }
#pragma unroll
      for (uint32_t j = 0; j < 8; ++j)
        if (t0 + j < T) row[t0 + j] = limit_step(uu[j], n[j], last, dlo, dhi);
    }
  }
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < (n >> 2); i += 256) {
    float e4[4];
    uint32_t r = 4u * i / T, c = 4u * i - r * T;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      e4[j] = tile[r * stride + c];
      if (++c == T) {c = 0; ++r;}
    }
    reinterpret_cast<float4*>(dst)[i] = make_float4(e4[0], e4[1], e4[2], e4[3]);
  }
  for (uint32_t e = (n & ~3u) + threadIdx.x; e < n; e += 256) {
    const uint32_t r = e / T, c = e - r * T;
    dst[e] = tile[r * stride + c];
  }
}

hipError_t smpc_launch_limit_noise(const SmpcLimitArgs& a, bool group_major, hipStream_t st)
{
  static_assert(sizeof(SmpcLimitArgs) <= 4096, "the arguments travel in the kernel argument segment");
  if (a.B == 0 || a.T == 0 || a.T > SMPC_LIMIT_MAX_T) return hipErrorInvalidValue;
  const bool vy = a.src[1] != nullptr;
  if (group_major) {
    const uint32_t groups = (a.B + 63u) / 64u;
    const dim3 grid((groups + 3u) / 4u);
    if (vy) hipLaunchKernelGGL(smpc_limit_noise_gm<true>, grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL(smpc_limit_noise_gm<false>, grid, dim3(256), 0, st, a);
    return hipGetLastError();
  }
  const uint32_t lds = (64u * (a.T | 1u) + a.T) * sizeof(float);   // at most 66.8 KB (T = 256)
  if (lds > 48u * 1024u) {   // (per device, so per launch: only horizons beyond 190 steps get here)
    const hipError_t raised = hipFuncSetAttribute(reinterpret_cast<const void*>(smpc_limit_noise_rm),
                                                  hipFuncAttributeMaxDynamicSharedMemorySize, 72 * 1024);
    if (raised != hipSuccess) return raised;
  }
  const dim3 grid((a.B + 63u) / 64u, vy ? 3u : 2u);
  hipLaunchKernelGGL(smpc_limit_noise_rm, grid, dim3(256), lds, st, a);
  return hipGetLastError();
}
