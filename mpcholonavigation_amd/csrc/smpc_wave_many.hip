// smpc_wave_many.hip — smpc_pass_many<R, MODE, FULL>: the wave-per-rollout pass of smpc_kernels.hip
// with the planning instance as the second grid dimension (smpc_group_optimize: a fleet whose
// members run the wave pass — the deployed critic list with consider_footprint, near-goal ticks,
// contexts created without the lane flag — scored in ONE launch).
//
// The text is smpc_wave_pass.inc, the one smpc_pass is compiled from: the same arithmetic in the
// same order, so a member's partials are bit for bit those of its own smpc_pass launch with the same
// grid and carve-up.  What differs (WAVE_PASS_MANY in the .inc): the parameter block and the
// geometry of instance blockIdx.y come from device memory, a block beyond its member's own grid
// leaves before the first barrier, the tick block is never in the kernel arguments, and there is no
// in-launch reduction — nothing in this kernel waits for another block.
//
// Instances: R = 1 (T <= 64), MODE 0, 3 and 4, whole and ragged horizon.  The rows of the table
// live with the other rows of the wave pass in smpc_kernels.hip.  Compiled with -ffp-contract=off
// like smpc_kernels.hip.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "smpc_dev.h"
#include "smpc_device_math.h"
#include "smpc_tail.h"

#include "smpc_wave_common.h"

#define WAVE_PASS_KERNEL smpc_pass_many
#define WAVE_PASS_MANY 1
#include "smpc_wave_pass.inc"
#undef WAVE_PASS_KERNEL
#undef WAVE_PASS_MANY

#define WAVE_MANY_INST(...) \
  template __global__ void smpc_pass_many<__VA_ARGS__>(const SmpcDev* __restrict__, const SmpcWaveGeom* __restrict__)
WAVE_MANY_INST(1, 0, true);
WAVE_MANY_INST(1, 0, false);
WAVE_MANY_INST(1, 3, true);
WAVE_MANY_INST(1, 3, false);
WAVE_MANY_INST(1, 4, true);
WAVE_MANY_INST(1, 4, false);
#undef WAVE_MANY_INST
