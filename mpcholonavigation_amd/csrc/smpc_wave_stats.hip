// smpc_wave_stats.hip — the kernels of smpc_critic_breakdown (include/smpc.h): per-critic costs
// and effective samples of a tick.
//
//   smpc_pass_stats<R, FULL>   the general wave-per-rollout pass (smpc_wave_pass.inc, MODE 2: the one
//                              pass that forms every critic's contribution as a value of its own)
//                              compiled a third time, under WAVE_PASS_STATS: at every add_cost_pow site
//                              and at the gamma add one lane stores the term to stats[row * ld + b].
//                              The same arithmetic in the same order as smpc_pass<R, 2, FULL>, so the
//                              costs it writes are that pass's costs bit for bit.
//   smpc_reduce_stats          grid (slices, 14): block (s, k < 13) reduces row k over slice s of the
//                              batch — sum, min, max and the softmax-weighted sum; block (s, 13) the
//                              weights themselves: sum w, sum w^2, the least cost and where it is.
//                              Weights are 2^(k2 (c - m_s)) with m_s the SLICE's least cost, as the pass
//                              forms them against its running minimum.
//   smpc_reduce_stats_final    one block: rescales the slices to the batch's least cost
//                              (2^(k2 (m_s - m)), the pass's own online-softmax step), sums them in
//                              double in slice order and writes the statistics.
//                              (The bodies of both: smpc_stats_reduce.inc, which
//                              smpc_wave_stats_many.hip compiles too.)
//
// A translation unit of its own, like smpc_wave_many.hip: a second kernel in smpc_kernels.hip moves
// the SGPR spill counts of smpc_pass.  Compiled with -ffp-contract=off like it.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/smpc.h"
#include "smpc_dev.h"
#include "smpc_device_math.h"
#include "smpc_tail.h"
#include "smpc_inst.h"

#include "smpc_wave_common.h"

// one lane of the wave keeps the term add_cost_pow has just folded into the cost: (float)v^power
__device__ __forceinline__ void stats_put(float* __restrict__ stats, uint32_t ld, uint32_t row, uint32_t b, bool on, double v,
                                          uint32_t power)
{
  if (on) stats[(size_t)row * ld + b] = (float)powu(v, power);
}

#define WAVE_PASS_KERNEL smpc_pass_stats
#define WAVE_PASS_MANY 0
#define WAVE_PASS_STATS 1
#include "smpc_wave_pass.inc"
#undef WAVE_PASS_KERNEL
#undef WAVE_PASS_MANY
#undef WAVE_PASS_STATS

// ---------------------------------------------------------------------------
// the reduction (its text: smpc_stats_reduce.inc, shared with smpc_wave_stats_many.hip)
// ---------------------------------------------------------------------------
#include "smpc_stats_reduce.inc"

__global__ void __launch_bounds__(kReduceBlock) smpc_reduce_stats(const float* __restrict__ stats, uint32_t ld,
                                                                  const float* __restrict__ costs, uint32_t B, uint32_t slice,
                                                                  float k2, double* __restrict__ part)
{
  reduce_stats_body(stats, ld, costs, B, slice, k2, part, gridDim.x, blockIdx.x, blockIdx.y);
}

__global__ void __launch_bounds__(kReduceBlock) smpc_reduce_stats_final(const double* __restrict__ part, uint32_t S, float k2,
                                                                        const float* __restrict__ stats, uint32_t ld,
                                                                        const float* __restrict__ pass_partials, uint32_t nblk,
                                                                        uint32_t TL, SmpcStatsOut* __restrict__ out)
{
  reduce_stats_final_body(part, S, k2, stats, ld, pass_partials, nblk, TL, out);
}

// ---------------------------------------------------------------------------
// the instances (smpc_inst.h): one row each
// ---------------------------------------------------------------------------
#define STATS_INST(...) {__VA_ARGS__, reinterpret_cast<const void*>(&smpc_pass_stats<__VA_ARGS__>)}
static const StatsInst kStatsInst[] = {STATS_INST(1, true), STATS_INST(1, false), STATS_INST(2, true),
                                       STATS_INST(2, false), STATS_INST(4, true), STATS_INST(4, false)};
#undef STATS_INST

const StatsInst* stats_select(int R, uint32_t T)
{
  const bool full = T == 64u * (uint32_t)R;
  for (const StatsInst& k : kStatsInst)
    if (k.r == R && k.full == full) return &k;
  return nullptr;
}

hipError_t stats_launch(const StatsInst* k, const SmpcDev& p, const SmpcLds& L, float* stats, uint32_t ld, uint32_t grid,
                        uint32_t block, hipStream_t st)
{
  if (!k || !stats || ld < p.B) return hipErrorInvalidValue;
  void* args[] = {const_cast<SmpcDev*>(&p), const_cast<SmpcLds*>(&L), &stats, &ld};
  return inst_launch(k->fn, dim3(grid), block, args, L.total, st);
}

hipError_t stats_set_lds_limit(int bytes) {return inst_set_lds_limit(kStatsInst, bytes);}

uint32_t stats_reduce_slices(uint32_t B, uint32_t* slice_out)
{
  // a block of 1024 threads takes four quads per thread; batches beyond 1024 such slices take longer ones
  uint32_t slice = 16384u;
  while ((B + slice - 1u) / slice > 1024u) slice *= 2u;
  if (slice_out) *slice_out = slice;
  return B ? (B + slice - 1u) / slice : 1u;
}

hipError_t stats_launch_reduce(const float* stats, uint32_t ld, const float* costs, uint32_t B, float k2, double* part,
                               const float* pass_partials, uint32_t nblk, uint32_t T, SmpcStatsOut* out, hipStream_t st)
{
  if ((ld & 3u) || ld < B || !B) return hipErrorInvalidValue;
  uint32_t slice = 0;
  const uint32_t S = stats_reduce_slices(B, &slice);
  hipLaunchKernelGGL(smpc_reduce_stats, dim3(S, SMPC_STATS_ROWS + 1), dim3(kReduceBlock), 0, st, stats, ld, costs, B, slice, k2,
                     part);
  hipLaunchKernelGGL(smpc_reduce_stats_final, dim3(1), dim3(kReduceBlock), 0, st, part, S, k2, stats, ld, pass_partials, nblk,
                     4u + 3u * T, out);
  return hipGetLastError();
}
