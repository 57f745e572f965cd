// smpc_lane.hip — the streaming pass with one LANE per rollout (T <= 64, lean critics).
//
// smpc_kernels.hip gives every rollout a whole wavefront (lane = time step): the lowest
// latency and the right shape for the reference's deployed batch (2 000 rollouts), but it
// pays ~35 cross-lane DPP steps and a lot of per-rollout scalar work executed 64 lanes wide.
// On CDNA4 a wave64 VALU instruction costs 4 cycles and at 10^5..10^6 rollouts that issue
// rate — not HBM — bounds the pass.  Here a wave owns 64 rollouts and
// walks the horizon step by step:
//   * every per-step operation is one instruction for 64 rollouts, no cross-lane traffic;
//     the float cumulative sums run in the reference's own sequential order
//     (optimizer.cpp:313-343);
//   * everything uniform over the batch (u[t], map geometry, weights) sits in SGPRs;
//   * noise is read from a group-major copy [B / 64][T / 4][64][4] (smpc_dev.h): one coalesced 1 KB
//     piece per array and quad of steps (a 16-byte load per lane), a group's quads back to back,
//     prefetched a quad ahead;
//   * the noised controls of the 64 rollouts stay PARKED IN REGISTERS (3 x 64 per lane)
//     until the rollouts' costs, hence softmax weights, are known; then
//     U[t] += sum_b w_b c[b][t] is a 64 x 64 transpose-reduce done in registers:
//     v_permlane32_swap / v_permlane16_swap (gfx950) and bank-masked DPP adds — two
//     instructions per butterfly node, no LDS, no second read of the noise;
//   * the block partial {min, sum w, furthest, non-colliding, U[3T]} has the layout of the
//     wave-per-rollout pass, so reduction, combine and the multi-GPU tuple are shared.
//
// Scope: the five critics (instances of their own for the near-goal GoalAngle term and for the
// deployed list's cruise tick), no path orientations, no trajectory write-out; T <= 64 parked,
// T = 64 or 128 in the re-read form.  smpc_pass_lane scores with every cost_power == 1;
// smpc_pass_lane_pow is the same body with general powers on the five critics, applied to each
// critic's per-rollout total in the epilogue (single context, parking form; the host sends it
// ticks of at least kLaneMinBatch rollouts); smpc_pass_lane_nh is the same body without a vy stream,
// for the plain cruise tick of the non-holonomic motion models (single context, parking form, whole
// quads; same batch rule).  smpc_prepare.cpp routes every other tick to smpc_pass.  Compiled with -ffp-contract=off like smpc_kernels.hip.

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include <type_traits>

#include "smpc_dev.h"
#include "smpc_device_math.h"
#include "smpc_tail.h"
#include "smpc_lane_common.h"
#include "smpc_inst.h"

#ifndef WAVE
#define WAVE 64
#endif
#define LANE_BLOCK 512   // 8 waves: 2 per SIMD, 256 registers each
// the re-read instances: 8 waves, one block per CU like the parking form.  (First built with 4
// waves and three blocks per CU: 136 registers allow three waves per SIMD.  The pass is
// VALU-bound either way, three blocks stage three copies of the window, and 4096 groups on 3072
// waves leave a ragged second round: 262 144 x 128 the same within noise, 131 072 x 128: 86 -> 78 us,
// 70 000 x 128: 73 -> 67 us.)
#define LANE_BLOCK_RR 512

// ---------------------------------------------------------------------------
// [B][T] row-major <-> group-major (SMPC_GM_INDEX, smpc_dev.h): one-off, after the noise is supplied
// (or drawn row-major), and back when something asks for the [B, T] tensors of a group-major draw
// ---------------------------------------------------------------------------
template <bool TO_GM>
__global__ void __launch_bounds__(256) smpc_relayout(const float* __restrict__ src, float* __restrict__ dst,
                                                    uint32_t B, uint32_t T)
{
  __shared__ float tile[32][33];
  const uint32_t b0 = blockIdx.x * 32, t0 = blockIdx.y * 32;
  const uint32_t lx = threadIdx.x & 31, ly = threadIdx.x >> 5;   // 32 x 8
  if (TO_GM) {
    for (uint32_t k = ly; k < 32; k += 8) {      // rows of the [B][T] tensor: coalesced along t
      const uint32_t b = b0 + k, t = t0 + lx;
      tile[k][lx] = (b < B && t < T) ? src[(size_t)b * T + t] : 0.f;
    }
    __syncthreads();
    for (uint32_t k = ly; k < 32; k += 8) {      // a quad of steps of 8 rollouts of one group: 128 bytes in a row
      const uint32_t e = k * 32 + lx, tl = 4 * (e >> 7) + (e & 3), bb = (e >> 2) & 31;
      const uint32_t t = t0 + tl, b = b0 + bb;
      if (b < B && t < T) dst[SMPC_GM_INDEX(b, t, T)] = tile[bb][tl];
    }
  } else {
    for (uint32_t k = ly; k < 32; k += 8) {
      const uint32_t e = k * 32 + lx, tl = 4 * (e >> 7) + (e & 3), bb = (e >> 2) & 31;
      const uint32_t t = t0 + tl, b = b0 + bb;
      tile[bb][tl] = (b < B && t < T) ? src[SMPC_GM_INDEX(b, t, T)] : 0.f;
    }
    __syncthreads();
    for (uint32_t k = ly; k < 32; k += 8) {
      const uint32_t b = b0 + k, t = t0 + lx;
      if (b < B && t < T) dst[(size_t)b * T + t] = tile[k][lx];
    }
  }
}

// to_gm: src [B][T] -> dst group-major; else src group-major -> dst [B][T]
hipError_t smpc_launch_relayout(const float* src, float* dst, uint32_t B, uint32_t T, bool to_gm, hipStream_t st)
{
  const dim3 grid((B + 31) / 32, (T + 31) / 32);
  if (to_gm) hipLaunchKernelGGL(smpc_relayout<true>, grid, dim3(256), 0, st, src, dst, B, T);
  else hipLaunchKernelGGL(smpc_relayout<false>, grid, dim3(256), 0, st, src, dst, B, T);
  return hipGetLastError();
}

// self-test of the transpose-reduce (tests/test_gpu_parity.py): v [64 lanes][64], w [64]
__global__ void __launch_bounds__(64) smpc_lane_reduce_kernel(const float* __restrict__ v,
                                                              const float* __restrict__ w,
                                                              float* __restrict__ out)
{
  const int lane = threadIdx.x;
  float V[64];
#pragma unroll
  for (int t = 0; t < 64; ++t) V[t] = v[lane * 64 + t];
  const LaneW lw = lane_weights(w[lane], lane);
  out[lane] = lane_reduce64(V, lw, lane);
}

hipError_t smpc_launch_lane_reduce(const float* v, const float* w, float* out, hipStream_t st)
{
  hipLaunchKernelGGL(smpc_lane_reduce_kernel, dim3(1), dim3(64), 0, st, v, w, out);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// The pass
// ---------------------------------------------------------------------------
// FULL: T == 64 NCH, every step slot of the unrolled loops is live; OBST: ObstaclesCritic scored
// MANY: several planning instances in one launch (smpc_group_optimize): blockIdx.y picks
// the instance, whose parameter block comes from device memory instead of the kernel arguments
// NCH: horizon in chunks of 64 steps (T <= 64 NCH)
// RR ("re-read"): the noised controls are NOT parked.  Once a group's weights are known the wave
// reads the group's noise a second time — 64 steps of one control at a time, straight into the
// registers the transpose-reduce consumes — and forms c = u + n again (the same single rounding).
// The second read comes seconds of microseconds after the first: from the Infinity Cache, not
// from HBM.  Without the 128 parked registers and the per-wave LDS slot a lane needs ~1/2 of
// the register file's per-wave share, but the blocks are the parking form's all the same:
// LANE_BLOCK_RR = 512 threads, one block per CU (see there for what three smaller blocks cost).
// The only form for T > 64 (3 T parked values per lane do not fit any register budget).
#define LANE_PASS_KERNEL smpc_pass_lane
#define LANE_PASS_POW false
#define LANE_PASS_NH false
#include "smpc_lane_pass.inc"
#undef LANE_PASS_KERNEL
#undef LANE_PASS_POW
#undef LANE_PASS_NH
// the same pass with general cost powers on the five critics (single context, parking form)
#define LANE_PASS_KERNEL smpc_pass_lane_pow
#define LANE_PASS_POW true
#define LANE_PASS_NH false
#include "smpc_lane_pass.inc"
#undef LANE_PASS_KERNEL
#undef LANE_PASS_POW
#undef LANE_PASS_NH
// the same pass without the vy stream, for the non-holonomic motion models (single context, parking
// form, the plain ObstaclesCritic rows of whole quads)
#define LANE_PASS_KERNEL smpc_pass_lane_nh
#define LANE_PASS_POW false
#define LANE_PASS_NH true
#include "smpc_lane_pass.inc"
#undef LANE_PASS_KERNEL
#undef LANE_PASS_POW
#undef LANE_PASS_NH

// ---------------------------------------------------------------------------
// The instances (smpc_inst.h): one row each.  Name, LDS limit, occupancy, selection and launch
// all read this table; adding an instance is adding a row and, if need be, a rule in lane_select.
// ---------------------------------------------------------------------------
#define LANE_INST(...) {__VA_ARGS__, reinterpret_cast<const void*>(&smpc_pass_lane<__VA_ARGS__>), false, false}
#define LANE_INST_POW(...) {__VA_ARGS__, reinterpret_cast<const void*>(&smpc_pass_lane_pow<__VA_ARGS__>), true, false}
#define LANE_INST_NH(...) {__VA_ARGS__, reinterpret_cast<const void*>(&smpc_pass_lane_nh<__VA_ARGS__>), false, true}
//                          FULL   OBST   MANY  NCH RR     GA     QUADS  TC  DEP
static const LaneInst kLaneInst[] = {
  LANE_INST(false, false, false, 1, false, false, false, 0, false),   // the five critics: ragged horizon
  LANE_INST(true, false, false, 1, false, false, true, 0, false),     // ... T = 64
  LANE_INST(false, true, false, 1, false, false, false, 0, false),
  LANE_INST(true, true, false, 1, false, false, true, 0, false),
  LANE_INST(false, true, false, 1, false, false, true, 0, false),     // whole quads
  LANE_INST(false, true, false, 1, false, false, true, 56, false),    // T = 56: the reference's default horizon, at compile time
  LANE_INST(false, false, true, 1, false, false, false, 0, false),    // grouped (smpc_group_optimize)
  LANE_INST(true, false, true, 1, false, false, true, 0, false),
  LANE_INST(false, true, true, 1, false, false, false, 0, false),
  LANE_INST(true, true, true, 1, false, false, true, 0, false),
  LANE_INST(true, true, false, 1, true, false, true, 0, false),       // re-read: one chunk, two chunks
  LANE_INST(true, true, false, 2, true, false, true, 0, false),
  LANE_INST(false, true, false, 1, false, true, false, 0, false),     // near-goal: the GoalAngle term
  LANE_INST(true, true, false, 1, false, true, true, 0, false),
  LANE_INST(true, true, false, 1, false, false, true, 0, true),       // deployed list: Constraint / Cost / Twirling
  LANE_INST(false, true, false, 1, false, false, true, 56, true),
  LANE_INST(true, true, true, 1, false, false, true, 0, true),        // ... grouped
  LANE_INST(false, true, true, 1, false, false, true, 56, true),
  // smpc_pass_lane_pow: general cost powers on the five critics (single context, parking form)
  LANE_INST_POW(true, true, false, 1, false, false, true, 0, false),      // T = 64
  LANE_INST_POW(false, true, false, 1, false, false, true, 0, false),     // whole quads
  LANE_INST_POW(false, true, false, 1, false, false, true, 56, false),    // T = 56
  LANE_INST_POW(false, true, false, 1, false, false, false, 0, false),    // ragged
  LANE_INST_POW(true, true, false, 1, false, true, true, 0, false),       // near-goal: the GoalAngle term
  LANE_INST_POW(false, true, false, 1, false, true, false, 0, false),
  LANE_INST_POW(true, false, false, 1, false, false, true, 0, false),     // no costmap lookup (a tick stripped of
  LANE_INST_POW(false, false, false, 1, false, false, false, 0, false),   // ObstaclesCritic after it was planned)
  // smpc_pass_lane_nh: no vy stream, the twins of the plain ObstaclesCritic rows of whole quads
  LANE_INST_NH(true, true, false, 1, false, false, true, 0, false),       // T = 64
  LANE_INST_NH(false, true, false, 1, false, false, true, 56, false),     // T = 56
  LANE_INST_NH(false, true, false, 1, false, false, true, 0, false),      // whole quads, T < 64
};
#undef LANE_INST
#undef LANE_INST_POW
#undef LANE_INST_NH

static const LaneInst* lane_find(bool full, bool obst, bool many, int nch, bool rr, bool ga, bool quads, int tc, bool dep,
                                 bool pow = false, bool nh = false)
{
  for (const LaneInst& k : kLaneInst)
    if (k.full == full && k.obst == obst && k.many == many && k.nch == nch && k.rr == rr && k.ga == ga &&
        k.quads == quads && k.tc == tc && k.dep == dep && k.pow == pow && k.nh == nh)
      return &k;
  return nullptr;
}

const LaneInst* lane_select(uint32_t flags, uint32_t T, bool rr, bool many, float acker_r, bool pow, bool nh)
{
  if (nh) {
    // the row these flags always got; where that is a plain ObstaclesCritic row of whole quads, its
    // twin without the vy stream
    const LaneInst* k = lane_select(flags, T, rr, many, acker_r, pow, false);
    if (!k || !k->obst || k->many || k->rr || k->ga || k->dep || k->pow || !k->quads) return k;
    return lane_find(k->full, true, false, 1, false, false, true, k->tc, false, false, true);
  }
  const uint32_t dep_set = SD_CONSTRAINT | SD_COST | SD_TWIRLING, lean_extra = dep_set | SD_GOAL | SD_PATH_ANGLE;
  // what no instance scores: trajectory write-out, path orientations, the general pass's critics
  if (flags & (SD_STORE_TRAJ | SD_USE_PATH_YAW | (SD_EXTRA_CRITICS & ~lean_extra))) return nullptr;
  const bool obst = (flags & (SD_OBSTACLES | SD_COST)) != 0;   // (Cost: the deployed-list instances, same lookup)
  const bool full = T == 64u;
  if (pow) {
    // cost powers: the five critics, one context, parking form — the shapes of the plain rows, the
    // two near-goal rows and the two rows without a costmap lookup
    if (rr || many || T > 64u || (flags & lean_extra)) return nullptr;
    if (flags & SD_GOAL_ANGLE) return obst ? lane_find(full, true, false, 1, false, true, full, 0, false, true) : nullptr;
    if (obst && T == 56u) return lane_find(false, true, false, 1, false, false, true, 56, false, true);
    return lane_find(full, obst, false, 1, false, false, full || (obst && (T & 3u) == 0u), 0, false, true);
  }
  if (rr) {
    // the five critics with ObstaclesCritic scored, whole chunks only (T = 64 or 128): the ragged
    // instances spill registers, and a spill in the time loop costs the noise prefetch its depth
    // (every scratch access waits vmcnt(0))
    if (!(flags & SD_OBSTACLES) || (flags & (lean_extra | SD_GOAL_ANGLE)) || (T != 64u && T != 128u)) return nullptr;
    return lane_find(true, true, many, T > 64u ? 2 : 1, true, false, true, 0, false);
  }
  if (T > 64u) return nullptr;   // the parking form: 3 x 64 noised controls per lane
  if (flags & dep_set) {   // cruise tick of the deployed critic list (PathAngle: the host knows it inert)
    if (!obst || (flags & (SD_GOAL_ANGLE | SD_GOAL)) || ((flags & SD_COST) && (flags & SD_OBSTACLES)) ||
        acker_r >= 0.f || (!full && T != 56u))
      return nullptr;
    return lane_find(full, true, many, 1, false, false, true, full ? 0 : 56, true);
  }
  if (flags & (SD_GOAL | SD_PATH_ANGLE)) return nullptr;
  if (flags & SD_GOAL_ANGLE)   // near-goal tick: the instances with the GoalAngle term
    return obst ? lane_find(full, true, many, 1, false, true, full, 0, false) : nullptr;
  if (many) return lane_find(full, obst, true, 1, false, false, full, 0, false);
  if (obst && T == 56u) return lane_find(false, true, false, 1, false, false, true, 56, false);
  return lane_find(full, obst, false, 1, false, false, full || (obst && (T & 3u) == 0u), 0, false);
}

const LaneInst* lane_occupancy_row(uint32_t T, bool rr)   // (a representative: smpc_inst.h)
{
  if (rr) return lane_find(true, true, false, T > 64u ? 2 : 1, true, false, true, 0, false);
  return lane_find(T == 64u, true, false, 1, false, false, T == 64u, 0, false);
}

// block: threads per block — LANE_BLOCK_RR for the re-read form; LANE_BLOCK for the parking form, or
// LANE_BLOCK / 2 for batches of at most one group per SIMD (a wave alone on its SIMD runs a group
// in 2/3 of the time)
hipError_t lane_launch(const LaneInst* k, const SmpcDev& p, const SmpcDev* d_many, uint32_t n, const SmpcLds& L,
                       uint32_t grid, uint32_t block, hipStream_t st)
{
  if (!k || k->many != (d_many != nullptr)) return hipErrorInvalidValue;
  if (k->rr ? block != LANE_BLOCK_RR : (block != LANE_BLOCK && block != LANE_BLOCK / 2)) return hipErrorInvalidValue;
  // the instance's name with every template argument written out, as rocprofv3 prints it
  auto b = [](bool v) {return v ? "true" : "false";};
  snprintf(smpc_last_pass_kernel, sizeof(smpc_last_pass_kernel), "smpc_pass_lane%s<%s, %s, %s, %d, %s, %s, %s, %d, %s>",
           k->pow ? "_pow" : (k->nh ? "_nh" : ""), b(k->full), b(k->obst), b(k->many), k->nch, b(k->rr), b(k->ga), b(k->quads), k->tc, b(k->dep));
  static const SmpcDev none{};   // (the grouped instances read their parameter blocks from device memory)
  void* args[] = {const_cast<SmpcDev*>(d_many ? &none : &p), const_cast<SmpcLds*>(&L), &d_many};
  return inst_launch(k->fn, d_many ? dim3(grid, n) : dim3(grid), block, args, L.total, st);
}

uint32_t smpc_lane_block() {return LANE_BLOCK;}
uint32_t smpc_lane_block_rr() {return LANE_BLOCK_RR;}

hipError_t lane_set_lds_limit(int bytes) {return inst_set_lds_limit(kLaneInst, bytes);}
