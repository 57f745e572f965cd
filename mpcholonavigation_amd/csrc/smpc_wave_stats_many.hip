// smpc_wave_stats_many.hip — the kernels of smpc_group_critic_breakdown (include/smpc.h): the critic
// breakdown of every member of a group in launches whose number does not depend on the members.
//
//   smpc_furthest_many<R, 1, FULL>   the furthest-point pre-pass (smpc_wave_pass.inc, MODE 1) with the
//                                    member as the second grid dimension: each member's parameter block
//                                    names its own furthest-point word (SmpcDev::furthest_out).
//   smpc_pass_stats_many<R, FULL>    smpc_pass_stats (smpc_wave_stats.hip) likewise: the text compiled
//                                    with WAVE_PASS_MANY and WAVE_PASS_STATS together.  blockIdx.y picks the
//                                    member; its parameter block, its geometry (SmpcWaveGeom: the carve-up
//                                    and the grid of its own smpc_pass_stats launch) and its rows
//                                    (SmpcStatsDst) come from device memory.  A block beyond its member's
//                                    grid leaves before the first barrier; nW is the member's grid times
//                                    the waves per block — so a member's rows, costs and partials are
//                                    those of its own smpc_pass_stats launch bit for bit.
//   smpc_reduce_stats_many           grid (slices of the largest member, 14, members): the body of
//   smpc_reduce_stats_final_many     smpc_reduce_stats / _final (smpc_stats_reduce.inc) with the
//                                    arguments of member blockIdx.z (the final: blockIdx.x) from device
//                                    memory.  Members differ in batch size, hence in slices: a block
//                                    beyond its member's slices returns before the first barrier.
//
// Instances: R = 1 (T <= 64), whole and ragged horizon.  A translation unit of its own, like the
// other compilations of the wave pass.  Compiled with -ffp-contract=off like them.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/smpc.h"
#include "smpc_dev.h"
#include "smpc_device_math.h"
#include "smpc_tail.h"
#include "smpc_inst.h"

#include "smpc_wave_common.h"

// one lane of the wave keeps the term add_cost_pow has just folded into the cost: (float)v^power
// (as in smpc_wave_stats.hip)
__device__ __forceinline__ void stats_put(float* __restrict__ stats, uint32_t ld, uint32_t row, uint32_t b, bool on, double v,
                                          uint32_t power)
{
  if (on) stats[(size_t)row * ld + b] = (float)powu(v, power);
}

#define WAVE_PASS_KERNEL smpc_pass_stats_many
#define WAVE_PASS_MANY 1
#define WAVE_PASS_STATS 1
#include "smpc_wave_pass.inc"
#undef WAVE_PASS_KERNEL
#undef WAVE_PASS_STATS

#define WAVE_PASS_KERNEL smpc_furthest_many
#define WAVE_PASS_STATS 0
#define WAVE_PASS_MANY_FURTHEST 1
#include "smpc_wave_pass.inc"
#undef WAVE_PASS_KERNEL
#undef WAVE_PASS_STATS
#undef WAVE_PASS_MANY_FURTHEST
#undef WAVE_PASS_MANY

#include "smpc_stats_reduce.inc"

__global__ void __launch_bounds__(kReduceBlock) smpc_reduce_stats_many(const SmpcStatsReduceArgs* __restrict__ many)
{
  const SmpcStatsReduceArgs& a = many[blockIdx.z];
  if (blockIdx.x >= a.S) return;   // (uniform over the block, before the first barrier)
  reduce_stats_body(a.stats, a.ld, a.costs, a.B, a.slice, a.k2, a.part, a.S, blockIdx.x, blockIdx.y);
}

__global__ void __launch_bounds__(kReduceBlock) smpc_reduce_stats_final_many(const SmpcStatsReduceArgs* __restrict__ many)
{
  const SmpcStatsReduceArgs& a = many[blockIdx.x];
  reduce_stats_final_body(a.part, a.S, a.k2, a.stats, a.ld, a.pass_partials, a.nblk, a.TL, a.out);
}

// ---------------------------------------------------------------------------
// the instances (smpc_inst.h): one row each
// ---------------------------------------------------------------------------
#define STATS_MANY_INST(FULL)                                                            \
  {1, FULL, reinterpret_cast<const void*>(&smpc_pass_stats_many<1, FULL>),               \
   reinterpret_cast<const void*>(&smpc_furthest_many<1, 1, FULL>)}
static const StatsManyInst kStatsManyInst[] = {STATS_MANY_INST(true), STATS_MANY_INST(false)};
#undef STATS_MANY_INST

const StatsManyInst* stats_many_select(int R, uint32_t T)
{
  const bool full = T == 64u * (uint32_t)R;
  for (const StatsManyInst& k : kStatsManyInst)
    if (k.r == R && k.full == full) return &k;
  return nullptr;
}

hipError_t stats_many_set_lds_limit(int bytes)
{
  hipError_t e = inst_set_lds_limit(kStatsManyInst, bytes);
  for (const StatsManyInst& k : kStatsManyInst)
    if (e == hipSuccess) e = hipFuncSetAttribute(k.fn_furthest, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  return e;
}

hipError_t stats_launch_furthest_many(const StatsManyInst* k, const SmpcDev* d_many, const SmpcWaveGeom* d_geom, uint32_t n,
                                      uint32_t grid_max, uint32_t lds_max, uint32_t block, hipStream_t st)
{
  if (!k || !d_many || !d_geom || !n || !grid_max) return hipErrorInvalidValue;
  void* args[] = {&d_many, &d_geom};
  return inst_launch(k->fn_furthest, dim3(grid_max, n), block, args, lds_max, st);
}

hipError_t stats_launch_many(const StatsManyInst* k, const SmpcDev* d_many, const SmpcWaveGeom* d_geom, const SmpcStatsDst* d_dst,
                             uint32_t n, uint32_t grid_max, uint32_t lds_max, uint32_t block, hipStream_t st)
{
  if (!k || !d_many || !d_geom || !d_dst || !n || !grid_max) return hipErrorInvalidValue;
  void* args[] = {&d_many, &d_geom, &d_dst};
  return inst_launch(k->fn, dim3(grid_max, n), block, args, lds_max, st);
}

hipError_t stats_launch_reduce_many(const SmpcStatsReduceArgs* d_many, uint32_t n, uint32_t slices_max, hipStream_t st)
{
  if (!d_many || !n || !slices_max) return hipErrorInvalidValue;
  hipLaunchKernelGGL(smpc_reduce_stats_many, dim3(slices_max, SMPC_STATS_ROWS + 1, n), dim3(kReduceBlock), 0, st, d_many);
  hipLaunchKernelGGL(smpc_reduce_stats_final_many, dim3(n), dim3(kReduceBlock), 0, st, d_many);
  return hipGetLastError();
}
