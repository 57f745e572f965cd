// smpc_moving_many.hip — smpc_moving_cost_gm_many<VY>, smpc_moving_cost_rm_many<R>: the
// moving-obstacle term of smpc_moving.hip with the member of a group as the second grid dimension
// (smpc_group_optimize_some: a fleet with mutual avoidance seeds every riding member's costs in ONE
// launch per form instead of one per member).
//
// The text is smpc_moving_cost.inc, the one the single kernels are compiled from: the same
// arithmetic in the same order, so a member's m, hits and seed are bit for bit those of its own
// smpc_moving_cost launch.  What differs (MOVING_COST_MANY in the .inc): the arguments of member
// blockIdx.y (SmpcMovingMember) come from device memory, the control sequence is always read from
// the device, and a block at or beyond its member's own grid leaves before the first barrier having
// written nothing.  Compiled with -ffp-contract=off like smpc_moving.hip; a module of its own: the
// resource usage of no other kernel moves.
#include <hip/hip_runtime.h>

#include "smpc_dev.h"
#include "smpc_device_math.h"
#include "smpc_moving.h"
#include "smpc_wave_common.h"

#define MOVING_COST_GM smpc_moving_cost_gm_many
#define MOVING_COST_RM smpc_moving_cost_rm_many
#define MOVING_COST_MANY 1
#include "smpc_moving_cost.inc"
#undef MOVING_COST_GM
#undef MOVING_COST_RM
#undef MOVING_COST_MANY

// `count` members of one form from d_many on; grid: the largest of the members' own grids
hipError_t smpc_launch_moving_cost_many(const SmpcMovingMember* d_many, uint32_t count, uint32_t grid, SmpcMovingForm form,
                                        uint32_t T, hipStream_t st)
{
  if (!d_many || count == 0 || grid == 0 || T == 0 || T > SMPC_MOVING_MAX_T) return hipErrorInvalidValue;
  const dim3 g(grid, count);
  switch (form) {
    case SMPC_MOVING_GM_VY: hipLaunchKernelGGL(smpc_moving_cost_gm_many<true>, g, dim3(256), 0, st, d_many); break;
    case SMPC_MOVING_GM: hipLaunchKernelGGL(smpc_moving_cost_gm_many<false>, g, dim3(256), 0, st, d_many); break;
    case SMPC_MOVING_RM:
      if (T <= 64u) hipLaunchKernelGGL(smpc_moving_cost_rm_many<1>, g, dim3(256), 0, st, d_many);
      else if (T <= 128u) hipLaunchKernelGGL(smpc_moving_cost_rm_many<2>, g, dim3(256), 0, st, d_many);
      else hipLaunchKernelGGL(smpc_moving_cost_rm_many<4>, g, dim3(256), 0, st, d_many);
      break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}
