// smpc_moving.h — arguments of smpc_moving_cost (smpc_moving.hip): the moving-obstacle term of one
// iteration, written where the iteration's scoring passes read their starting cost.
// Shared by the kernel and the host side (smpc_ctx.h); kept out of smpc_dev.h, whose structs every
// scoring pass is compiled against.
#ifndef SMPC_MOVING_H_
#define SMPC_MOVING_H_

#include <stdint.h>

#define SMPC_MOVING_MAX_T 256u
#define SMPC_MOVING_MAX_K 64u   // SMPC_MAX_MOVING_OBSTACLES (include/smpc.h)

// By how much the squared reach (radius + margin)^2 is widened before a squared distance is compared
// with it: a term at or beyond it has sqrtf(d2) >= radius + margin whatever the roundings of the two
// squares, so q is exactly 0 and the square root is not taken.
#define SMPC_MOVING_REACH_GUARD 1.000001f

// Noise in the order vx, vy, wz, in the layout of the launch; n[1] == null: a non-holonomic model — no
// vy tensor is read.  u: the iteration's control sequence [3][T]; u_dev == null: it is in u_arg (the
// uploaded sequence of iteration 0, whichever way the scoring pass gets its tick block).
// The obstacle table comes in the form the launch reads:
//   group-major launch: tab = [T][K] of {x, y, guarded squared reach, radius}  (a step's K discs: one run)
//   row-major launch:   tab = [K][T] of {x, y} (a wave's read of one disc: one run), disc = [K] of
//                       {radius, radius + margin, guarded squared reach, 0}
struct SmpcMovingArgs {
  const float* n[3];
  const float* u_dev;
  const float* tab;
  const float* disc;
  float* seed;        // [B] what the passes read as costs_prev: m, or (add) its own content + m
  float* m_out;       // [B] m itself, or null
  uint8_t* hit_out;   // [B] hit, or null
  uint32_t B, T, K;
  uint32_t add;       // iteration > 0: seed = (float)((double)seed + m)
  double x0, y0;      // robot state, as SmpcDev has it
  float yaw0, cos0, sin0, dt;
  float v0[3];        // (float) speed: state v[:,0]
  float collision_cost, repulsion_weight, margin;
  uint32_t pad[2];
  float u_arg[3 * SMPC_MOVING_MAX_T] __attribute__((aligned(16)));
};

// One member of a grouped launch (smpc_moving_many.hip: the member is blockIdx.y): SmpcMovingArgs
// without u_arg — an array of these travels in a group's hand-over, 152 bytes a member instead of
// 3 KB — and with the member's own grid: a block whose blockIdx.x is at or beyond it belongs to a
// larger member's grid and does nothing.  u_dev is never null: the iteration's control sequence in
// the member's tick block on the device (or what the limiter was given).  T: the group's.
struct SmpcMovingMember {
  const float* n[3];
  const float* u_dev;
  const float* tab;
  const float* disc;
  float* seed;
  float* m_out;
  uint8_t* hit_out;
  uint32_t B, T, K;
  uint32_t add;
  double x0, y0;
  float yaw0, cos0, sin0, dt;
  float v0[3];
  float collision_cost, repulsion_weight, margin;
  uint32_t grid;      // ceil(B / 4) of the row-major form, ceil(ceil(B / 64) / 4) of the group-major form
  uint32_t pad;
};

// the instances of a grouped launch: the row-major form (R from the group's T) and the two group-major forms
enum SmpcMovingForm { SMPC_MOVING_RM = 0, SMPC_MOVING_GM_VY = 1, SMPC_MOVING_GM = 2, SMPC_MOVING_FORMS = 3 };

#endif  // SMPC_MOVING_H_
