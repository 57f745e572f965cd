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
// Their text is smpc_moving_cost.inc, which smpc_moving_many.hip compiles a second time for the members
// of a group in one launch.
#include <hip/hip_runtime.h>

#include "smpc_dev.h"
#include "smpc_device_math.h"
#include "smpc_moving.h"
#include "smpc_wave_common.h"

// the two forms: one text with smpc_moving_many.hip (the member of a group as a grid dimension)
#define MOVING_COST_GM smpc_moving_cost_gm
#define MOVING_COST_RM smpc_moving_cost_rm
#include "smpc_moving_cost.inc"
#undef MOVING_COST_GM
#undef MOVING_COST_RM

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
