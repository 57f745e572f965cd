// smpc_inst.h — the scoring-pass instances as data.  Each kernel family keeps ONE table next to its
// kernel (smpc_kernels.hip, smpc_lane.hip, smpc_split.hip, smpc_wave_stats.hip): a row holds the template arguments and
// the instance's address, written by one macro.  The kernel's name, the LDS limit, occupancy, the
// selector ("which instance scores these flags?") and the launch all read that table.  Internal:
// not part of the C-ABI.
#ifndef SMPC_INST_H_
#define SMPC_INST_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "smpc_dev.h"

#pragma GCC visibility push(hidden)

// many: the instance is smpc_pass_many<...>, the same template arguments with several planning instances per launch
struct WaveInst { int r, mode; bool full, many; const void* fn; };                                 // smpc_pass<R, MODE, FULL>
// pow: the instance is smpc_pass_lane_pow<...>, the same template arguments with general cost powers
// nh: the instance is smpc_pass_lane_nh<...>, the same template arguments without the vy stream
struct LaneInst { bool full, obst, many; int nch; bool rr, ga, quads; int tc; bool dep; const void* fn; bool pow, nh; };   // smpc_pass_lane<...>
struct SplitInst { int nseg; bool full; const void* fn; };                                         // smpc_pass_split<NSEG, FULL>

// Selectors: the instance that scores these flags at this horizon, or null when there is none.
// mode: 0 score (all cost_power == 1), 1 furthest only, 3 score (all cost_power == 1, with the
// additive forms of Cost, Goal, Constraint, Twirling, PathAngle), anything else: the general pass
// many: the grouped rows (smpc_group_optimize) — R = 1 and mode 0, 3 or 4 only, null otherwise
const WaveInst* wave_select(int R, int mode, uint32_t T, bool many = false);
// rr: the re-read form (no parked controls; required for T > 64); many: the grouped instances
// (smpc_group_optimize); acker_r: the Ackermann min_turning_r, < 0 for the other models
// pow: the tick scores with a cost_power other than 1 among the five critics — only then is a row of
// smpc_pass_lane_pow returned (single context, parking form); false behaves as it always did
// nh: the tick runs a non-holonomic model on the rows of smpc_pass_lane_nh — flags that select a
// plain ObstaclesCritic row of whole quads get that row's twin without the vy stream, every other
// flags the row they always got (a pass stripped of ObstaclesCritic, say)
const LaneInst* lane_select(uint32_t flags, uint32_t T, bool rr, bool many, float acker_r, bool pow, bool nh = false);
// step: PathAlign's trajectory_point_step; nseg: lanes per rollout, 4 or 2
const SplitInst* split_select(uint32_t flags, uint32_t T, uint32_t step, uint32_t nseg);

// Occupancy is asked about one REPRESENTATIVE of the instances a tick shape may run (they share the
// launch bounds; the grids were measured with these): the plain ObstaclesCritic instance of the
// parking form (whole horizon or ragged), the re-read instance with one or two chunks, and the
// whole-horizon instance of the split form.
const LaneInst* lane_occupancy_row(uint32_t T, bool rr);
const SplitInst* split_occupancy_row(uint32_t nseg);

// Launch a row; each records the instance's name for smpc_debug_last_pass_kernel().
hipError_t wave_launch(const WaveInst* k, const SmpcDev& p, const SmpcLds& L, uint32_t grid, uint32_t block, hipStream_t st);
// a grouped row: n instances in one launch of grid_max x n blocks, their parameter blocks and geometry
// (each its own LDS carve-up and grid, both in device memory); lds_max: the largest carve-up's total
hipError_t wave_launch_many(const WaveInst* k, const SmpcDev* d_many, const SmpcWaveGeom* d_geom, uint32_t n, uint32_t grid_max,
                            uint32_t lds_max, uint32_t block, hipStream_t st);
// d_many == nullptr: one planning instance, p its parameter block; else n instances in one launch,
// their parameter blocks in device memory (p is not read)
hipError_t lane_launch(const LaneInst* k, const SmpcDev& p, const SmpcDev* d_many, uint32_t n, const SmpcLds& L,
                       uint32_t grid, uint32_t block, hipStream_t st);
hipError_t split_launch(const SplitInst* k, const SmpcDev& p, const SmpcLds& L, uint32_t grid, hipStream_t st);

// ---- smpc_critic_breakdown (smpc_wave_stats.hip): the general wave pass that keeps every critic's term ----
struct StatsInst { int r; bool full; const void* fn; };                                            // smpc_pass_stats<R, FULL>
const StatsInst* stats_select(int R, uint32_t T);
// stats: [SMPC_STATS_ROWS][ld] floats, ld >= p.B; p.costs: the totals; nothing is recorded for
// smpc_debug_last_pass_kernel (a breakdown leaves no trace in what a tick reports)
hipError_t stats_launch(const StatsInst* k, const SmpcDev& p, const SmpcLds& L, float* stats, uint32_t ld, uint32_t grid,
                        uint32_t block, hipStream_t st);
hipError_t stats_set_lds_limit(int bytes);
// what the reduction leaves on the device
struct SmpcStatsOut {
  uint32_t best_rollout;
  float best_cost, effective_samples;
  float non_colliding;   // of the pass whose partials were handed in
  float sum[13], min[13], max[13], weighted[13], at_best[13];
};
// slices of the batch the reduction's first launch works in (and their length, a multiple of four)
uint32_t stats_reduce_slices(uint32_t B, uint32_t* slice_out);
// smpc_reduce_stats + smpc_reduce_stats_final over the rows and `costs` (both 16-byte aligned, ld a
// multiple of four, allocations padded to it); part: (SMPC_STATS_ROWS + 1) x slices x 4 doubles of scratch;
// pass_partials / nblk: the scoring pass's per-block partials, for its non-colliding count
hipError_t stats_launch_reduce(const float* stats, uint32_t ld, const float* costs, uint32_t B, float k2, double* part,
                               const float* pass_partials, uint32_t nblk, uint32_t T, SmpcStatsOut* out, hipStream_t st);

// ---- smpc_group_critic_breakdown (smpc_wave_stats_many.hip): the breakdown of a group's members per launch ----
// fn: smpc_pass_stats_many<R, FULL>; fn_furthest: smpc_furthest_many<R, 1, FULL>, the pre-pass.  R = 1 only.
struct StatsManyInst { int r; bool full; const void* fn; const void* fn_furthest; };
const StatsManyInst* stats_many_select(int R, uint32_t T);
hipError_t stats_many_set_lds_limit(int bytes);
// one member's arguments of the two reduction kernels (device memory): those of stats_launch_reduce
struct SmpcStatsReduceArgs {
  const float* stats;
  const float* costs;
  double* part;
  const float* pass_partials;
  SmpcStatsOut* out;
  uint32_t ld, B, slice, S;   // S: this member's slices, of `slice` rollouts
  uint32_t nblk, TL;          // the scoring pass's blocks and the floats of one of its partials
  float k2;
};
// n members in one launch of grid_max x n blocks: parameter blocks, geometry and (the stats pass) rows
// per member in device memory; lds_max: the largest carve-up's total.  Nothing is recorded for
// smpc_debug_last_pass_kernel.
hipError_t stats_launch_furthest_many(const StatsManyInst* k, const SmpcDev* d_many, const SmpcWaveGeom* d_geom, uint32_t n,
                                      uint32_t grid_max, uint32_t lds_max, uint32_t block, hipStream_t st);
hipError_t stats_launch_many(const StatsManyInst* k, const SmpcDev* d_many, const SmpcWaveGeom* d_geom, const SmpcStatsDst* d_dst,
                             uint32_t n, uint32_t grid_max, uint32_t lds_max, uint32_t block, hipStream_t st);
// smpc_reduce_stats_many + smpc_reduce_stats_final_many; slices_max: the most slices any member has
hipError_t stats_launch_reduce_many(const SmpcStatsReduceArgs* d_many, uint32_t n, uint32_t slices_max, hipStream_t st);

hipError_t wave_set_lds_limit(int bytes);
hipError_t lane_set_lds_limit(int bytes);
hipError_t split_set_lds_limit(int bytes);

// developer aid: the scoring-pass instance launched last, as rocprofv3 names it
extern char smpc_last_pass_kernel[96];

// ---- what the three tables share -------------------------------------------------------------
template <typename Inst, size_t N>
inline hipError_t inst_set_lds_limit(const Inst (&table)[N], int bytes)
{
  hipError_t e = hipSuccess;
  for (size_t k = 0; k < N && e == hipSuccess; ++k)
    e = hipFuncSetAttribute(table[k].fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  return e;
}

inline hipError_t inst_occupancy(const void* fn, uint32_t block, uint32_t lds_bytes, int* blocks_per_cu)
{
  if (!fn) return hipErrorInvalidValue;
  return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks_per_cu, fn, static_cast<int>(block), lds_bytes);
}

inline hipError_t inst_launch(const void* fn, dim3 grid, uint32_t block, void** args, uint32_t lds_bytes, hipStream_t st)
{
  (void)hipLaunchKernel(fn, grid, dim3(block), args, lds_bytes, st);   // (what hipLaunchKernelGGL wraps)
  return hipGetLastError();
}

#pragma GCC visibility pop

#endif  // SMPC_INST_H_
