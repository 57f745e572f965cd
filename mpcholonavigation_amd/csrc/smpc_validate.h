// smpc_validate.h — arguments of smpc_validate (smpc_validate.hip): the collision check of one control
// sequence's trajectory (include/smpc.h: smpc_validate_trajectory).  Shared by the
// kernel and the host side (smpc_validate_host.cpp); kept out of smpc_dev.h, whose structs every
// scoring pass is compiled against.
#ifndef SMPC_VALIDATE_H_
#define SMPC_VALIDATE_H_

#include <stdint.h>

#include "../../include/smpc.h"   // smpc_validation: the kernel writes the caller's struct

#define SMPC_VALIDATE_MAX_T 256u   // a thread is a trajectory point, a block a member
#define SMPC_VALIDATE_BLOCK 256u

// One member of a launch (blockIdx.x): an array of these, each followed somewhere by its control
// sequence, is the call's ONE upload.
struct SmpcValidateArgs {
  // what smpc_footprint_walk.inc reads of its parameter block, under the names SmpcDev gives them.
  // The window is of zero size: every cell comes from the global map.
  const uint8_t* map;
  uint32_t W, H;
  double ox, oy, res;
  int32_t win_x0, win_y0, win_w, win_h;
  uint32_t fp_n;
  float fp_pic;                // the possibly-inscribed cost (findCircumscribedCost); < 0: no inflation layer
  double fp_x[SMPC_MAX_FOOTPRINT], fp_y[SMPC_MAX_FOOTPRINT];
  // the control sequence [3][T] (device) and the pose it is integrated from
  const float* u;
  double x0, y0;
  float yaw0, dt;
  uint32_t T;
  uint32_t n_check;            // poses checked: min(T, floorf(collision_lookahead_time / model_dt))
  uint32_t holonomic;          // 0: the vy row is not read
  uint32_t consider_footprint, track_unknown;
  // moving obstacles: the row-major table of smpc_moving.h ([K][T]{x, y}, [K]{radius, ...}); K == 0: none
  uint32_t K;
  const float* tab_kt;
  const float* disc;
  // where the host reads after its one wait (host memory mapped into the device)
  smpc_validation* out;
  float* xyyaw;                // [T][3]
};

#endif  // SMPC_VALIDATE_H_
