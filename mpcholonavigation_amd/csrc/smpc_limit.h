// smpc_limit.h — arguments of smpc_limit_noise (smpc_limit.hip): the acceleration limits applied to
// the stored noise of one iteration.  Shared by the kernel and the host side (smpc_ctx.h); kept out
// of smpc_dev.h, whose structs every scoring pass is compiled against.
#ifndef SMPC_LIMIT_H_
#define SMPC_LIMIT_H_

#include <stdint.h>

#define SMPC_LIMIT_MAX_T 256u

// Controls in the order vx, vy, wz.  src[1] == null: a non-holonomic model — no vy tensor is read or
// written.  u: the iteration's control sequence [3][T]; u_dev == null: it is in u_arg (the uploaded
// sequence of iteration 0, whichever way the scoring pass gets its tick block).
struct SmpcLimitArgs {
  const float* src[3];
  float* dst[3];
  const float* u_dev;
  uint32_t B, T;
  float v0[3];     // (float) speed: state v[:,0]
  float dlo[3];    // model_dt * {ax_min, -ay_max, -az_max}, formed on the host in float
  float dhi[3];    // model_dt * {ax_max, ay_max, az_max}
  uint32_t pad;
  float u_arg[3 * SMPC_LIMIT_MAX_T] __attribute__((aligned(16)));
};

#endif  // SMPC_LIMIT_H_
