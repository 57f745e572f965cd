// smpc_kernels.hip — gfx950 (MI355X / CDNA4) kernels of the sampling-MPC hot path.
//
// One wavefront (64 lanes) owns one rollout at a time; lane l holds time steps
// [l*R, l*R+R) of the horizon in registers (R = ceil(T/64)).  The reference's
// [B,T] tensor passes (noise add, predict, integrate, critics, softmax update;
// reference src/optimizer.cpp:157-164,227-233,313-343,362-394) collapse into
// one streaming pass over the three noise tensors:
//
//   noise row (coalesced 256 B/array) -> c = u + n -> v = shift(c) ->
//   yaw = scan(wz dt) -> sincos -> x,y = scan(...) -> critics (costmap window
//   and path in LDS) -> cost -> online softmax accumulation of w*c per wave ->
//   per-block partial {min, sum w, sum w*c[3T]}.
//
// Cross-lane work uses DPP row shifts / broadcasts (no LDS traffic); there is
// no dense contraction anywhere, hence no MFMA: the bound is HBM (12*T bytes of
// noise per rollout) against FP32 VALU for the two transcendentals per step.
//
// Compiled with -ffp-contract=off so that a*b+c keeps the two roundings of the
// reference's separate xtensor passes.

#include <hip/hip_runtime.h>
#include <stdio.h>
#include <algorithm>
#include <stdint.h>

#include "smpc_dev.h"
#include "smpc_device_math.h"
#include "smpc_tail.h"
#include "smpc_inst.h"

#include "smpc_wave_common.h"

// ---------------------------------------------------------------------------
// The streaming pass.
//   MODE 0: score, every cost_power == 1 (the defaults): all per-step terms of
//           the additive critics go through ONE wave reduction
//   MODE 1: rollout + endpoint argmin only (utils::findPathFurthestReachedPoint,
//           tools/utils.hpp:292-319)
//   MODE 2: score, general cost_power (pow in double per critic)
//   MODE 3: MODE 0 plus the additive forms of CostCritic, GoalCritic, ConstraintCritic,
//           TwirlingCritic and PathAngleCritic (every cost_power == 1): the deployed critic
//           list (robot_bringup/config/nav2_params.yaml:222) in ONE wave reduction instead of
//           one double-precision reduction and one pow per critic
//   MODE 4: MODE 3 plus consider_footprint for the list's one collision critic (the deployed
//           YAML as written, nav2_params.yaml:258): a step whose centre cost reaches the
//           possibly-inscribed cost walks the footprint, up to 64 steps of a rollout side by side
//   FULL:   T == 64*R, every lane owns R valid steps (no tail predicates)
//
// A wave rolls out one rollout at a time (lane = time step) and PARKS it: its noised
// controls go to an LDS ring, its PathAlign sample points to a slot table, its cost so
// far to a lane slot.  Every L.group rollouts the wave FLUSHES: PathAlign for the whole
// group with lane = (rollout, sample) so all 64 lanes work, one shared softmax rescale,
// then the weighted controls of the group are accumulated.
// ---------------------------------------------------------------------------
// The text of the pass is smpc_wave_pass.inc, compiled under two names: smpc_pass here (one planning
// instance) and smpc_pass_many in smpc_wave_many.hip (several in one launch, blockIdx.y = instance:
// R = 1 and MODE 0, 3, 4 only — a group member that needs another instance is ticked on its own).
// A translation unit of its own, so that this one's device code is what it was before the grouped
// kernel existed: with both kernels in one module the MODE 3 instances of smpc_pass came out with
// four to eight fewer SGPR spills — harmless, but not "unchanged".
#define WAVE_PASS_KERNEL smpc_pass
#define WAVE_PASS_MANY 0
#include "smpc_wave_pass.inc"
#undef WAVE_PASS_KERNEL
#undef WAVE_PASS_MANY

// smpc_wave_many.hip instantiates these six
template <int R, int MODE, bool FULL>
__global__ void smpc_pass_many(const SmpcDev* __restrict__ many, const SmpcWaveGeom* __restrict__ geom);
#define WAVE_MANY_EXTERN(...) \
  extern template __global__ void smpc_pass_many<__VA_ARGS__>(const SmpcDev* __restrict__, const SmpcWaveGeom* __restrict__)
WAVE_MANY_EXTERN(1, 0, true);
WAVE_MANY_EXTERN(1, 0, false);
WAVE_MANY_EXTERN(1, 3, true);
WAVE_MANY_EXTERN(1, 3, false);
WAVE_MANY_EXTERN(1, 4, true);
WAVE_MANY_EXTERN(1, 4, false);
#undef WAVE_MANY_EXTERN

// ---------------------------------------------------------------------------
// Reduce the per-block partials of one pass into one shard tuple
// {min, sum w, furthest, non-colliding, U[3T]}.  Block j owns 32 tuple columns;
// its 1024 threads are 32 columns x 32 row slices (coalesced 128-B row pieces).
// ---------------------------------------------------------------------------
// With fin.enabled (single-GPU tick, one tuple) every block also finishes its columns:
// divide by sum w, clip, write the new control sequence to device AND host-mapped memory
// (optimizer.cpp:382-393,237-249) — the separate combine launch and the D2H copy go away.
__device__ __forceinline__ void reduce_partials_body(const float* __restrict__ partials,
                                                     uint32_t nblk, uint32_t T, float neg_inv_temp,
                                                     float* __restrict__ tuple, const SmpcFinal& fin)
{
  __shared__ float s_red[16], s_red2[16], s_red3[16];
  __shared__ float s_sc[2048];
  __shared__ float s_acc[32][33];
  const uint32_t TL = 4 + 3 * T;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nwave = blockDim.x >> 6;
  const uint32_t col = blockIdx.x * 32 + (tid & 31);
  const uint32_t sl = tid >> 5;  // 32 slices
  const bool colon = col < TL && col != 0 && col != 2 && col != 3;
  // Every global load this thread needs is issued before the first wait: the tuple headers
  // {min, sum w, furthest, non-colliding} of (up to two) partials, and the first 16 rows of
  // its column — one memory round trip instead of five dependent ones.
  float hm[2], hw[2], hf[2], hn[2];
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const uint32_t g = tid + k * 1024;
    const bool on = g < nblk;
    const float* h = partials + (size_t)(on ? g : 0) * TL;
    hm[k] = on ? h[0] : 3.0e38f;
    hw[k] = on ? h[1] : 0.f;
    hf[k] = on ? h[2] : 0.f;
    hn[k] = on ? h[3] : 0.f;
  }
  float v[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const uint32_t g = sl + 32 * k;
    v[k] = (colon && g < nblk) ? partials[(size_t)g * TL + col] : 0.f;
  }
  float m = fminf(hm[0], hm[1]), fu = fmaxf(hf[0], hf[1]), nc = hn[0] + hn[1];
  for (int o = 32; o > 0; o >>= 1) {
    m = fminf(m, __shfl_xor(m, o, WAVE));
    fu = fmaxf(fu, __shfl_xor(fu, o, WAVE));
    nc += __shfl_xor(nc, o, WAVE);
  }
  if (lane == 0) {
    s_red[wave] = m;
    s_red2[wave] = fu;
    s_red3[wave] = nc;
  }
  __syncthreads();
  m = 3.0e38f;
  fu = 0.f;
  nc = 0.f;
  for (int w = 0; w < nwave; ++w) {
    m = fminf(m, s_red[w]);
    fu = fmaxf(fu, s_red2[w]);
    nc += s_red3[w];
  }
  // per-block rescale factors exp(-(m_g - m)/temperature), once; sum of weights from the headers
  float a = 0.f;
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const uint32_t g = tid + k * 1024;
    if (g < nblk) {
      const float sc = expf(neg_inv_temp * (hm[k] - m));
      s_sc[g] = sc;
      a += sc * hw[k];
    }
  }
  for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o, WAVE);
  __syncthreads();   // s_sc complete, s_red* free again
  if (lane == 0) s_red[wave] = a;
  float acc = 0.f;
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const uint32_t g = sl + 32 * k;
    if (g < nblk) acc += s_sc[g] * v[k];
  }
  if (colon) {   // grids beyond 512 blocks: the rest of the column
    for (uint32_t g = sl + 512; g < nblk; g += 32) acc += s_sc[g] * partials[(size_t)g * TL + col];
  }
  s_acc[sl][tid & 31] = acc;
  __syncthreads();
  float sw = 0.f;
  for (int w = 0; w < nwave; ++w) sw += s_red[w];
  if (sl == 0 && col < TL) {
    float r = 0.f;
#pragma unroll
    for (int s = 0; s < 32; ++s) r += s_acc[s][tid & 31];
    if (col == 0) r = m;
    if (col == 1) r = sw;
    if (col == 2) r = fu;
    if (col == 3) r = nc;
    tuple[col] = r;
    if (fin.enabled) {
      if (col >= 4) {
        const uint32_t i = col - 4;
        float v2 = r / sw;
        // applyControlSequenceConstraints (optimizer.cpp:237-249)
        if (i < T) v2 = fminf(fmaxf(v2, fin.vx_min), fin.vx_max);
        else if (i < 2 * T) v2 = fminf(fmaxf(v2, -fin.vy_max), fin.vy_max);
        else v2 = fminf(fmaxf(v2, -fin.wz_max), fin.wz_max);
        fin.u_dev[i] = v2;
        if (fin.u_host) fin.u_host[i] = v2;
      } else if (col == 0) {
        const float used = fin.furthest_used ? *fin.furthest_used : fu;
        const float res[5] = {m, sw, fu, nc, used};
        for (int k = 0; k < 5; ++k) {
          fin.u_dev[SMPC_RESULT_AT(T) + k] = res[k];   // slots SMPC_R_MIN_COST .. SMPC_R_F_USED
          if (fin.u_host) fin.u_host[SMPC_RESULT_AT(T) + k] = res[k];
        }
      }
    }
    // the tick block's number as the pass read it (SMPC_CANARY_SLOT): to the device copy of the
    // result (the combine kernels forward it from there) and, when finishing, to the host
    if (col == 0 && fin.u_dev) {
      const float cn = partials[SMPC_CANARY_SLOT(T)];
      fin.u_dev[SMPC_RESULT_AT(T) + SMPC_R_CANARY] = cn;
      if (fin.enabled && fin.u_host) fin.u_host[SMPC_RESULT_AT(T) + SMPC_R_CANARY] = cn;
    }
  }
  // completion for the polling host: every block publishes the tick's sequence number in its
  // own word (slot SMPC_R_BLOCK_DONE + block of u_host) behind a system-scope fence over its host stores, and the
  // host waits for all of them — no counter and no second fence between the last store and the
  // host (the tail timeline of tools/tail_timeline.py prices them at ~2 us)
  if (fin.enabled && fin.done_counter) {
    __threadfence_system();
    __syncthreads();
    if (tid == 0)
      __hip_atomic_store(reinterpret_cast<uint32_t*>(fin.u_host + SMPC_RESULT_AT(T) + SMPC_R_BLOCK_DONE + blockIdx.x), fin.seq,
                         __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}


__global__ void __launch_bounds__(1024) smpc_reduce_partials(const float* __restrict__ partials,
                                                            uint32_t nblk, uint32_t T,
                                                            float neg_inv_temp,
                                                            float* __restrict__ tuple,
                                                            const SmpcFinal fin)
{
  reduce_partials_body(partials, nblk, T, neg_inv_temp, tuple, fin);
}

// several planning instances in one launch (smpc_group_optimize): blockIdx.y picks the instance
__global__ void __launch_bounds__(1024) smpc_reduce_partials_many(const SmpcReduceArgs* __restrict__ many,
                                                                 uint32_t T)
{
  const SmpcReduceArgs& a = many[blockIdx.y];
  reduce_partials_body(a.partials, a.nblk, T, a.neg_inv_temp, a.tuple, a.fin);
}

// ---------------------------------------------------------------------------
// Combine G shard tuples into the new control sequence (optimizer.cpp:382-393):
// rescale by exp(-(min_g - min)/temperature), divide by sum w, clip.
// result: {min, sum_w, furthest, non_colliding}.  One block.
// ---------------------------------------------------------------------------
__device__ __forceinline__ void combine_tuples_body(const float* __restrict__ tuples, uint32_t stride,
                                                    uint32_t G, uint32_t T, float neg_inv_temp,
                                                    float vx_max, float vx_min, float vy_max,
                                                    float wz_max, float* __restrict__ u_out,
                                                    float* __restrict__ result,
                                                    const float* __restrict__ furthest_used,
                                                    float* __restrict__ host_out, uint32_t seq)
{
  const uint32_t TL = stride;
  float m = 3.0e38f, fu = 0.f, nc = 0.f;
  for (uint32_t g = 0; g < G; ++g) {
    m = fminf(m, tuples[(size_t)g * TL]);
    fu = fmaxf(fu, tuples[(size_t)g * TL + 2]);
    nc += tuples[(size_t)g * TL + 3];
  }
  float sw = 0.f;
  for (uint32_t g = 0; g < G; ++g)
    sw += expf(neg_inv_temp * (tuples[(size_t)g * TL] - m)) * tuples[(size_t)g * TL + 1];
  for (uint32_t i = threadIdx.x; i < 3 * T; i += blockDim.x) {
    float acc = 0.f;
    for (uint32_t g = 0; g < G; ++g)
      acc += expf(neg_inv_temp * (tuples[(size_t)g * TL] - m)) * tuples[(size_t)g * TL + 4 + i];
    float v = acc / sw;
    // applyControlSequenceConstraints (optimizer.cpp:237-249)
    if (i < T) v = fminf(fmaxf(v, vx_min), vx_max);
    else if (i < 2 * T) v = fminf(fmaxf(v, -vy_max), vy_max);
    else v = fminf(fmaxf(v, -wz_max), wz_max);
    u_out[i] = v;
    if (host_out) host_out[i] = v;
  }
  if (threadIdx.x == 0) {
    // [4]: the furthest point the critics consumed (cached across iterations)
    const float res[5] = {m, sw, fu, nc, furthest_used ? *furthest_used : fu};
    for (int k = 0; k < 5; ++k) {
      result[k] = res[k];
      if (host_out) host_out[SMPC_RESULT_AT(T) + k] = res[k];   // slots SMPC_R_MIN_COST .. SMPC_R_F_USED
    }
    if (host_out) host_out[SMPC_RESULT_AT(T) + SMPC_R_CANARY] = result[SMPC_R_CANARY];   // the pass's echo of the tick block's number (smpc_reduce_partials)
  }
  // completion word for the polling host, behind every host store of this (single) block
  if (host_out && seq) {
    __threadfence_system();
    __syncthreads();
    if (threadIdx.x == 0)
      __hip_atomic_store(reinterpret_cast<uint32_t*>(host_out + SMPC_RESULT_AT(T) + SMPC_R_DONE), seq, __ATOMIC_RELEASE,
                         __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

__global__ void __launch_bounds__(256) smpc_combine_tuples(const float* __restrict__ tuples,
                                                          uint32_t G, uint32_t T,
                                                          float neg_inv_temp, float vx_max,
                                                          float vx_min, float vy_max,
                                                          float wz_max, float* __restrict__ u_out,
                                                          float* __restrict__ result,
                                                          const float* __restrict__ furthest_used,
                                                          float* __restrict__ host_out, uint32_t seq)
{
  combine_tuples_body(tuples, 4 + 3 * T, G, T, neg_inv_temp, vx_max, vx_min, vy_max, wz_max, u_out, result,
                      furthest_used, host_out, seq);
}

// ---------------------------------------------------------------------------
// Exchange of the shard tuples WITHOUT a collective (include/smpc.h smpc_shard_p2p_*): every
// rank owns a mailbox in fine-grained device memory that its peers have mapped (IPC, xGMI):
// [2 parities][world slots][slot_floats], the last word of a slot being its sequence number.
// One block: copy this rank's tuple into slot `rank` of every mailbox, fence at system scope,
// publish the sequence number; wait until every slot of the own mailbox carries it; then
// combine as smpc_combine_tuples does (mode 0) or just take the maximum of the furthest points
// (mode 1: the exchange of the non-speculative first tick).  Two parities: a rank can run at
// most one exchange ahead of its slowest peer (it needs that peer's tuple to finish its own).
//
// The wait is bounded in WALL-CLOCK time (s_memrealtime, a constant 100 MHz counter:
// x.timeout_ticks of 10 ns each).  On expiry the block sets *x.state (sticky, device memory) and
// the host's mark (SMPC_R_MARK) to SMPC_MARK_PEER_LATE, publishes the completion word so that the host returns at once, and
// publishes nothing else.  Every later exchange of this ctx sees *x.state != 0 on entry and
// does the same WITHOUT writing to any peer: a rank that failed once stays silent, so its peers
// fail at their next exchange at the latest instead of consuming tuples of a rank whose own
// tick was lost.  Only smpc_shard_p2p_init (collective) clears the state.
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256) smpc_p2p_exchange(const float* __restrict__ my_tuple,
                                                        const SmpcP2P x, uint32_t T, int mode,
                                                        float* __restrict__ d_furthest,
                                                        float neg_inv_temp, float vx_max, float vx_min,
                                                        float vy_max, float wz_max,
                                                        float* __restrict__ u_out,
                                                        float* __restrict__ result,
                                                        const float* __restrict__ furthest_used,
                                                        float* __restrict__ host_out, uint32_t seq)
{
  __shared__ int s_late;
  const uint32_t TL = 4 + 3 * T, tid = threadIdx.x;
  const size_t slot0 = (size_t)((x.xseq & 1u) * x.world) * x.slot_floats;
  if (tid == 0) s_late = (__hip_atomic_load(x.state, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u) ? 2 : 0;
  __syncthreads();
  if (s_late == 0) {
    for (uint32_t r = 0; r < x.world; ++r) {
      float* dst = x.peer[r] + slot0 + (size_t)x.rank * x.slot_floats;
      for (uint32_t i = tid; i < TL; i += blockDim.x) dst[i] = my_tuple[i];
    }
    __threadfence_system();
    __syncthreads();
    if (tid < x.world)
      __hip_atomic_store(reinterpret_cast<uint32_t*>(x.peer[tid] + slot0 + (size_t)x.rank * x.slot_floats + TL),
                         x.xseq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
  const float* mine = x.peer[x.rank] + slot0;
  if (s_late == 0 && tid < x.world) {
    const uint32_t* flag = reinterpret_cast<const uint32_t*>(mine + (size_t)tid * x.slot_floats + TL);
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
    while (__hip_atomic_load(flag, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_SYSTEM) != x.xseq) {
      __builtin_amdgcn_s_sleep(8);
      if (__builtin_amdgcn_s_memrealtime() - t0 > x.timeout_ticks) {
        s_late = 1;
        break;
      }
    }
  }
  __syncthreads();
  if (s_late) {
    if (tid == 0) {
      __hip_atomic_store(x.state, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (host_out) {
        host_out[SMPC_RESULT_AT(T) + SMPC_R_MARK] = SMPC_MARK_PEER_LATE;
        __threadfence_system();
        if (seq)
          __hip_atomic_store(reinterpret_cast<uint32_t*>(host_out + SMPC_RESULT_AT(T) + SMPC_R_DONE), seq, __ATOMIC_RELEASE,
                             __HIP_MEMORY_SCOPE_SYSTEM);
      }
    }
    return;
  }
  if (mode == 1) {
    if (tid == 0) {
      float fu = 0.f;
      for (uint32_t r = 0; r < x.world; ++r) fu = fmaxf(fu, mine[(size_t)r * x.slot_floats + 2]);
      *d_furthest = fu;
    }
    return;
  }
  combine_tuples_body(mine, x.slot_floats, x.world, T, neg_inv_temp, vx_max, vx_min, vy_max, wz_max, u_out,
                      result, furthest_used, host_out, seq);
}

// ---------------------------------------------------------------------------
// AckermannMotionModel::applyConstraints (motion_models.hpp:110-117), the last step of
// applyControlSequenceConstraints (optimizer.cpp:248): where |vx|/|wz| < min_turning_r,
// wz = sign(wz) |vx| / min_turning_r.  It needs the finished vx AND wz of a step, which the
// column-parallel finishing kernels hold in different blocks, so it is its own T-thread
// launch behind them and publishes the tick's completion word in their place.
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256) smpc_ackermann_constrain(float* __restrict__ u_dev,
                                                               float* __restrict__ u_host,
                                                               uint32_t T, float min_r, uint32_t seq)
{
  for (uint32_t t = threadIdx.x; t < T; t += blockDim.x) {
    const float v = u_dev[t], w = u_dev[2 * T + t];
    if (fabsf(v) / fabsf(w) < min_r) {
      const float sgn = w > 0.f ? 1.f : (w < 0.f ? -1.f : 0.f);
      const float nw = sgn * fabsf(v) / min_r;
      u_dev[2 * T + t] = nw;
      if (u_host) u_host[2 * T + t] = nw;
    }
  }
  if (u_host && seq) {
    __threadfence_system();
    __syncthreads();
    if (threadIdx.x == 0)
      __hip_atomic_store(reinterpret_cast<uint32_t*>(u_host + SMPC_RESULT_AT(T) + SMPC_R_DONE), seq, __ATOMIC_RELEASE,
                         __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

// ---------------------------------------------------------------------------
// Device RNG: Philox4x32-10 + Box–Muller, one block of two samples per thread
// (stands in for xt::random::randn, noise_generator.cpp:107-122).
// ---------------------------------------------------------------------------
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3,
                                              uint32_t k0, uint32_t k1, uint32_t (&o)[4])
{
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    if (r > 0) {
      k0 += 0x9E3779B9u;
      k1 += 0xBB67AE85u;
    }
    // (one 32 x 32 -> 64 multiply each, v_mad_u64_u32: half the quarter-rate instructions of a
    // v_mul_hi_u32 / v_mul_lo_u32 pair)
    const uint64_t p0 = (uint64_t)0xD2511F53u * (uint64_t)c0, p1 = (uint64_t)0xCD9E8D57u * (uint64_t)c2;
    const uint32_t hi0 = (uint32_t)(p0 >> 32), lo0 = (uint32_t)p0;
    const uint32_t hi1 = (uint32_t)(p1 >> 32), lo1 = (uint32_t)p1;
    const uint32_t n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
    c0 = n0;
    c1 = lo1;
    c2 = n2;
    c3 = lo0;
  }
  o[0] = c0;
  o[1] = c1;
  o[2] = c2;
  o[3] = c3;
}

// Box–Muller on one pair of Philox words: {radius cos, radius sin} of N(0, 1).  The hardware's
// log2 and square root (1 ulp) and the rollout's own sin/cos (absolute error 1.3e-7): a normal
// of radius r = sqrt(-2 ln u1) lies within 4.5e-7 r of the float64 evaluation of the same u1 and
// float angle (measured: 2.3e-7 r at most, 9.6e-7 absolute at r = 5.1; r <= 5.887; the hardware
// log2 keeps its relative accuracy up to u1 = 1 - 2^-24, and u1 = 1 gives exactly 0) — tests:
// test_gpu_noise_stream.py::test_device_box_muller_against_float64 through smpc_selftest_box_muller
// — at a third of the instructions of logf / sincosf: with regenerate_noises the draw is
// 3 x B x T normals per tick.
__device__ __forceinline__ void box_muller(uint32_t r0, uint32_t r1, float& z0, float& z1)
{
  const float u1 = ((float)(r0 >> 8) + 0.5f) * (1.0f / 16777216.0f);
  const float u2 = ((float)(r1 >> 8) + 0.5f) * (1.0f / 16777216.0f);
  // -2 ln u1 = -2 ln 2 log2 u1
  const float radius = __builtin_amdgcn_sqrtf(-1.3862943611198906f * __builtin_amdgcn_logf(u1));
  float sn, cs;
  smpc_sincos_fast(6.2831853071795864769f * u2, sn, cs);
  z0 = radius * cs;
  z1 = radius * sn;
}

// Flat elements 4q .. 4q + 3 of a tensor share ONE Philox block (all four words are used: two
// Box–Muller pairs): thread q of the grid covering [base, base + n).
__global__ void __launch_bounds__(256) smpc_fill_noise(float* __restrict__ out, uint64_t n,
                                                      uint64_t base, uint64_t seed,
                                                      uint32_t stream, uint32_t epoch,
                                                      float sigma)
{
  const uint64_t q_first = base >> 2;
  const uint64_t q_last = (base + n + 3) >> 2;  // exclusive
  for (uint64_t q = q_first + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; q < q_last;
       q += (uint64_t)gridDim.x * blockDim.x) {
    uint32_t r[4];
    philox4x32_10((uint32_t)q, (uint32_t)(q >> 32), stream, epoch, (uint32_t)seed,
                  (uint32_t)(seed >> 32), r);
    float z[4];
    box_muller(r[0], r[1], z[0], z[1]);
    box_muller(r[2], r[3], z[2], z[3]);
    const uint64_t e0 = q << 2;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const uint64_t e = e0 + (uint64_t)k;
      if (e >= base && e < base + n) out[e - base] = z[k] * sigma;
    }
  }
}

// The same stream written GROUP-MAJOR (SMPC_GM_INDEX, smpc_dev.h: the layout the lane-per-rollout
// and split passes read): thread (b, group of four steps) with b fastest, so a wave writes one
// coalesced 1 KB piece.  Element e = base + b * T + t of the global [B_global, T] tensor is word
// e % 4 of Philox block e / 4 exactly as in smpc_fill_noise; T must be a multiple of four, so
// that a block never straddles two rollouts (base is a multiple of T).
__global__ void __launch_bounds__(256) smpc_fill_noise_tm(float* __restrict__ dst, uint32_t B, uint32_t T,
                                                         uint64_t base, uint64_t seed, uint32_t stream,
                                                         uint32_t epoch, float sigma)
{
  // blockIdx.y: the group of four steps; x: rollouts (no 64-bit division of a flat index)
  const uint32_t tq = blockIdx.y;
  for (uint32_t b = blockIdx.x * blockDim.x + threadIdx.x; b < B; b += gridDim.x * blockDim.x) {
    const uint64_t q = (base + (uint64_t)b * T + 4u * tq) >> 2;
    uint32_t r[4];
    philox4x32_10((uint32_t)q, (uint32_t)(q >> 32), stream, epoch, (uint32_t)seed, (uint32_t)(seed >> 32), r);
    float z[4];
    box_muller(r[0], r[1], z[0], z[1]);
    box_muller(r[2], r[3], z[2], z[3]);
    // the four steps of quad tq are 16 contiguous, 16-byte aligned bytes of the lane: one store
    typedef float fill_f32x4 __attribute__((ext_vector_type(4)));
    *reinterpret_cast<fill_f32x4*>(dst + SMPC_GM_INDEX(b, 4u * tq, T)) =
        fill_f32x4{z[0] * sigma, z[1] * sigma, z[2] * sigma, z[3] * sigma};
  }
}

// ---------------------------------------------------------------------------
// Self-test hook: the device sin/cos used by the rollout, evaluated on caller data.
// ---------------------------------------------------------------------------
__global__ void smpc_sincos_kernel(const float* __restrict__ x, uint32_t n,
                                   float* __restrict__ sn, float* __restrict__ cs)
{
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) {
    float s, c;
    smpc_sincos(x[i], s, c);
    sn[i] = s;
    cs[i] = c;
  }
}

hipError_t smpc_launch_sincos(const float* x, uint32_t n, float* sn, float* cs, hipStream_t st)
{
  hipLaunchKernelGGL(smpc_sincos_kernel, dim3((n + 255) / 256), dim3(256), 0, st, x, n, sn, cs);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Self-test hooks: the noise fills' own philox4x32_10 and box_muller on caller data.
// ---------------------------------------------------------------------------
__global__ void smpc_philox_kernel(const uint32_t* __restrict__ ctr, uint32_t k0, uint32_t k1, uint32_t n,
                                   uint32_t* __restrict__ out)
{
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) {
    uint32_t r[4];
    philox4x32_10(ctr[4 * i], ctr[4 * i + 1], ctr[4 * i + 2], ctr[4 * i + 3], k0, k1, r);
#pragma unroll
    for (int k = 0; k < 4; ++k) out[4 * i + k] = r[k];
  }
}

__global__ void smpc_box_muller_kernel(const uint32_t* __restrict__ r0, const uint32_t* __restrict__ r1,
                                       uint32_t n, float* __restrict__ z0, float* __restrict__ z1)
{
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) {
    float a, b;
    box_muller(r0[i], r1[i], a, b);
    z0[i] = a;
    z1[i] = b;
  }
}

hipError_t smpc_launch_philox(const uint32_t* ctr, uint32_t k0, uint32_t k1, uint32_t n, uint32_t* out,
                              hipStream_t st)
{
  hipLaunchKernelGGL(smpc_philox_kernel, dim3((n + 255) / 256), dim3(256), 0, st, ctr, k0, k1, n, out);
  return hipGetLastError();
}

hipError_t smpc_launch_box_muller(const uint32_t* r0, const uint32_t* r1, uint32_t n, float* z0, float* z1,
                                  hipStream_t st)
{
  hipLaunchKernelGGL(smpc_box_muller_kernel, dim3((n + 255) / 256), dim3(256), 0, st, r0, r1, n, z0, z1);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// launch wrappers (called from smpc_api.cpp through plain C++ linkage)
// ---------------------------------------------------------------------------
char smpc_last_pass_kernel[96] = "";   // (a developer aid: not per thread)

// the instances of the wave-per-rollout pass (smpc_inst.h): one row each
#define WAVE_INST(...) {__VA_ARGS__, false, reinterpret_cast<const void*>(&smpc_pass<__VA_ARGS__>)}
#define WAVE_INST_MANY(...) {__VA_ARGS__, true, reinterpret_cast<const void*>(&smpc_pass_many<__VA_ARGS__>)}
#define WAVE_INST_R(MODE) WAVE_INST(1, MODE, true), WAVE_INST(1, MODE, false), WAVE_INST(2, MODE, true), \
                          WAVE_INST(2, MODE, false), WAVE_INST(4, MODE, true), WAVE_INST(4, MODE, false)
static const WaveInst kWaveInst[] = {
  WAVE_INST_R(0), WAVE_INST_R(1), WAVE_INST_R(2), WAVE_INST_R(3), WAVE_INST_R(4),
  // grouped (smpc_group_optimize): T <= 64, the lean scoring modes
  WAVE_INST_MANY(1, 0, true), WAVE_INST_MANY(1, 0, false), WAVE_INST_MANY(1, 3, true), WAVE_INST_MANY(1, 3, false),
  WAVE_INST_MANY(1, 4, true), WAVE_INST_MANY(1, 4, false)};
#undef WAVE_INST_R
#undef WAVE_INST_MANY
#undef WAVE_INST

// FULL: T == 64 R, every step slot is live
const WaveInst* wave_select(int R, int mode, uint32_t T, bool many)
{
  const int m = (mode == 0 || mode == 1 || mode == 3 || mode == 4) ? mode : 2;
  const bool full = T == 64u * (uint32_t)R;
  for (const WaveInst& k : kWaveInst)
    if (k.r == R && k.mode == m && k.full == full && k.many == many) return &k;
  return nullptr;
}

hipError_t wave_launch(const WaveInst* k, const SmpcDev& p, const SmpcLds& L, uint32_t grid, uint32_t block, hipStream_t st)
{
  if (!k || k->many) return hipErrorInvalidValue;
  snprintf(smpc_last_pass_kernel, sizeof(smpc_last_pass_kernel), "smpc_pass<%d, %d, %s>", k->r, k->mode, k->full ? "true" : "false");
  void* args[] = {const_cast<SmpcDev*>(&p), const_cast<SmpcLds*>(&L)};
  return inst_launch(k->fn, dim3(grid), block, args, L.total, st);
}

hipError_t wave_launch_many(const WaveInst* k, const SmpcDev* d_many, const SmpcWaveGeom* d_geom, uint32_t n, uint32_t grid_max,
                            uint32_t lds_max, uint32_t block, hipStream_t st)
{
  if (!k || !k->many || !d_many || !d_geom || !n || !grid_max) return hipErrorInvalidValue;
  snprintf(smpc_last_pass_kernel, sizeof(smpc_last_pass_kernel), "smpc_pass_many<%d, %d, %s>", k->r, k->mode, k->full ? "true" : "false");
  void* args[] = {&d_many, &d_geom};
  return inst_launch(k->fn, dim3(grid_max, n), block, args, lds_max, st);
}

hipError_t wave_set_lds_limit(int bytes) {return inst_set_lds_limit(kWaveInst, bytes);}

hipError_t smpc_launch_reduce(const float* partials, uint32_t nblk, uint32_t T,
                              float neg_inv_temp, float* tuple, const SmpcFinal& fin,
                              hipStream_t st)
{
  hipLaunchKernelGGL(smpc_reduce_partials, dim3(smpc_reduce_blocks(T)), dim3(1024), 0, st, partials, nblk,
                     T, neg_inv_temp, tuple, fin);
  return hipGetLastError();
}

// After smpc_reduce_partials_many: ONE block copies every instance's result (u and the slots up to the canary echo) to its
// host-mapped mirror and publishes the sequence words behind a single system-scope fence
// (hundreds of blocks fencing PCIe writes one by one cost far more than the reduction itself).
__global__ void __launch_bounds__(1024) smpc_publish_many(const SmpcReduceArgs* __restrict__ many,
                                                         uint32_t n, uint32_t T)
{
  const uint32_t len = SMPC_RESULT_AT(T) + SMPC_R_CANARY + 1u;   // u, the five results, the tick block's number
  for (uint32_t i = threadIdx.x; i < n * len; i += blockDim.x) {
    const uint32_t q = i / len, k = i - q * len;
    many[q].host_out[k] = many[q].fin.u_dev[k];
  }
  __threadfence_system();
  __syncthreads();
  for (uint32_t q = threadIdx.x; q < n; q += blockDim.x)
    __hip_atomic_store(reinterpret_cast<uint32_t*>(many[q].host_out + SMPC_RESULT_AT(T) + SMPC_R_DONE), many[q].seq,
                       __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

hipError_t smpc_launch_reduce_many(const SmpcReduceArgs* d_many, uint32_t n, uint32_t T, hipStream_t st)
{
  hipLaunchKernelGGL(smpc_reduce_partials_many, dim3(smpc_reduce_blocks(T), n), dim3(1024), 0, st, d_many, T);
  hipLaunchKernelGGL(smpc_publish_many, dim3(1), dim3(1024), 0, st, d_many, n, T);
  return hipGetLastError();
}

hipError_t smpc_launch_combine(const float* tuples, uint32_t G, uint32_t T, float neg_inv_temp,
                               float vx_max, float vx_min, float vy_max, float wz_max,
                               float* u_out, float* result, const float* furthest_used,
                               float* host_out, uint32_t seq, hipStream_t st)
{
  hipLaunchKernelGGL(smpc_combine_tuples, dim3(1), dim3(256), 0, st, tuples, G, T, neg_inv_temp,
                     vx_max, vx_min, vy_max, wz_max, u_out, result, furthest_used, host_out, seq);
  return hipGetLastError();
}

hipError_t smpc_launch_p2p_exchange(const float* my_tuple, const SmpcP2P& x, uint32_t T, int mode,
                                    float* d_furthest, float neg_inv_temp, float vx_max, float vx_min,
                                    float vy_max, float wz_max, float* u_out, float* result,
                                    const float* furthest_used, float* host_out, uint32_t seq,
                                    hipStream_t st)
{
  hipLaunchKernelGGL(smpc_p2p_exchange, dim3(1), dim3(256), 0, st, my_tuple, x, T, mode, d_furthest,
                     neg_inv_temp, vx_max, vx_min, vy_max, wz_max, u_out, result, furthest_used, host_out,
                     seq);
  return hipGetLastError();
}

hipError_t smpc_launch_ackermann(float* u_dev, float* u_host, uint32_t T, float min_r, uint32_t seq,
                                 hipStream_t st)
{
  hipLaunchKernelGGL(smpc_ackermann_constrain, dim3(1), dim3(256), 0, st, u_dev, u_host, T, min_r,
                     seq);
  return hipGetLastError();
}

hipError_t smpc_launch_fill_noise_tm(float* dst, uint32_t B, uint32_t T, uint64_t base, uint64_t seed,
                                     uint32_t stream, uint32_t epoch, float sigma, hipStream_t st)
{
  if (T & 3u) return hipErrorInvalidValue;   // a Philox block of four must not straddle two rollouts
  uint32_t grid = std::min<uint32_t>((B + 255u) / 256u, 2048u);
  if (grid == 0) grid = 1;
  hipLaunchKernelGGL(smpc_fill_noise_tm, dim3(grid, T >> 2), dim3(256), 0, st, dst, B, T, base, seed, stream, epoch, sigma);
  return hipGetLastError();
}

hipError_t smpc_launch_fill_noise(float* out, uint64_t n, uint64_t base, uint64_t seed,
                                  uint32_t stream, uint32_t epoch, float sigma, hipStream_t st)
{
  const uint64_t blocks4 = (n + 6) / 4;   // (covers a base that is not a multiple of four)
  uint32_t grid = (uint32_t)((blocks4 + 255) / 256);
  if (grid > 4096) grid = 4096;
  if (grid == 0) grid = 1;
  hipLaunchKernelGGL(smpc_fill_noise, dim3(grid), dim3(256), 0, st, out, n, base, seed, stream,
                     epoch, sigma);
  return hipGetLastError();
}
