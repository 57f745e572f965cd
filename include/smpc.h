/*
 * smpc.h — C-ABI of the MI355X-native sampling-MPC hot path.
 *
 * This is the drop-in boundary for ONE path of the reference
 * (soham2560/MPCHoloNavigation, package nav2_sortham_controller): the body of
 * sortham::Optimizer::optimize() — noise add, holonomic rollout, critic
 * scoring, softmax-weighted control update — i.e. everything between
 * Optimizer::prepare() and utils::savitskyGolayFilter() in
 * Optimizer::evalControl() (reference src/optimizer.cpp:134-164).
 *
 * Plain C, plain pointers and sizes; no C++/torch/ROS types cross it.
 * Every entry point cites the reference interface it replaces as
 * [ref file:line], paths relative to nav2_sortham_controller/.
 *
 * Conventions
 *   - every function returning int returns SMPC_OK (0) or a negative
 *     SMPC_ERR_* code; smpc_last_error(ctx) gives the text.  No exception
 *     crosses the ABI.  "All trajectories collide" is NOT an error: it is
 *     smpc_tick_out.fail_flag = 1 and the host runs Optimizer::fallback()
 *     [ref src/optimizer.cpp:166-183].
 *   - the caller owns every pointer it passes; the library copies what it
 *     needs before returning (device pointers in the *_device entry points
 *     are the exception and are documented there).
 *   - a ctx is used by one thread at a time [ref src/controller.cpp:94-103
 *     holds the parameter and costmap mutexes around the whole tick];
 *     distinct ctx are independent (the reference's function-static retry
 *     counter, src/optimizer.cpp:168, is per-host-object here).
 *   - tensors are row-major [batch, time] float32 exactly like the
 *     reference's xt::xtensor<float,2> members [ref models/state.hpp:30-57].
 */
#ifndef SMPC_H_
#define SMPC_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SMPC_ABI_VERSION 3

/* ---- status codes ------------------------------------------------------ */
#define SMPC_OK 0
#define SMPC_ERR_INVALID -1     /* bad argument / inconsistent sizes          */
#define SMPC_ERR_UNSUPPORTED -2 /* feature outside the hot-path scope         */
#define SMPC_ERR_DEVICE -3      /* HIP runtime error (text in last_error)     */
#define SMPC_ERR_STATE -4       /* call order (no costmap / no noise yet)     */
#define SMPC_ERR_NOMEM -5

/* ---- costmap cost constants [nav2_costmap_2d cost_values.hpp; used at
 *      ref src/critics/obstacles_critic.cpp:185-201, tools/utils.hpp:374-386] */
#define SMPC_COST_NO_INFORMATION 255
#define SMPC_COST_LETHAL 254
#define SMPC_COST_INSCRIBED 253
#define SMPC_COST_FREE 0

/* ---- motion models [ref include/.../motion_models.hpp:85-171,
 *      src/optimizer.cpp:414-426 setMotionModel].  Omni is the holonomic
 *      model the north star names.  The two non-holonomic models draw no vy
 *      noise, keep state.vy and control_sequence.vy at zero and return a Twist
 *      without linear.y [ref src/optimizer.cpp:220-224,241-243,264-266,
 *      334-337,374-389,404-410; src/noise_generator.cpp:117-121]; Ackermann
 *      also bounds the turning radius of the updated control sequence
 *      [ref motion_models.hpp:110-117] and adds a ConstraintCritic term
 *      [ref src/critics/constraint_critic.cpp:54-69].  They run the Omni
 *      kernels with vy held at zero, except the plain cruise tick of the
 *      lane-per-rollout pass from 61 440 rollouts up — the five critics with
 *      ObstaclesCritic scored, every cost_power 1, no GoalAngle term, no
 *      deployed-list critic, trajectory_point_step 4, time_steps <= 64 and a
 *      multiple of four, the context not in a group — which runs
 *      smpc_pass_lane_nh: the same pass without a vy stream, the same results
 *      bit for bit.  SMPC_NONHOLO_PASS=omni in the environment at smpc_create
 *      keeps the Omni kernels for those ticks too.                          */
#define SMPC_MODEL_OMNI 0
#define SMPC_MODEL_DIFF_DRIVE 1
#define SMPC_MODEL_ACKERMANN 2

/* ---- smpc_config.flags ------------------------------------------------- */
#define SMPC_FLAG_STORE_TRAJECTORIES 0x1u /* materialise x,y,yaw [B,T] each
                                             pass so smpc_get_trajectories()
                                             works [ref optimizer.cpp:455-458] */
#define SMPC_FLAG_NO_SPECULATION 0x2u     /* always run the furthest-point
                                             pre-pass (exact two-pass mode)  */
#define SMPC_FLAG_WAVE_PER_ROLLOUT 0x8u   /* always the wave-per-rollout pass             */
#define SMPC_FLAG_LANE_PER_ROLLOUT 0x10u  /* the lane-per-rollout pass (csrc/smpc_lane.hip)
                                             on every tick it has an instance for, whatever
                                             the batch size: the five critics (near the goal
                                             with the GoalAngle term) or the deployed list's
                                             cruise tick, time_steps <= 64 (128 for the
                                             re-read form), every cost_power 1.  A tick whose
                                             only departure from that is a cost_power other
                                             than 1 among the five critics takes the lane pass
                                             too (smpc_pass_lane_pow), but only from 61 440
                                             rollouts up, with or without this flag: below
                                             that it stays on the wave-per-rollout pass.
                                             Likewise the rows without a vy stream of a
                                             non-holonomic model (smpc_pass_lane_nh): from
                                             61 440 rollouts up, with or without this flag;
                                             below that such a tick runs the Omni-form rows */
#define SMPC_FLAG_PROFILE 0x4u            /* bracket each scoring pass with HIP
                                             events (smpc_tick_out.score_pass_ms) */

/*
 * Optimizer settings.  Mirrors sortham::models::OptimizerSettings,
 * ControlConstraints and SamplingStd
 * [ref models/optimizer_settings.hpp:28-41, models/constraints.hpp:25-42];
 * defaults are the ones Optimizer::getParams() declares
 * [ref src/optimizer.cpp:69-82]; see smpc_config_default().
 */
typedef struct smpc_config {
  uint32_t batch_size;      /* B, this ctx's rollouts (a shard when sharded) */
  uint32_t time_steps;      /* T                                             */
  uint32_t iteration_count; /* optimize() iterations per tick                */
  uint32_t motion_model;    /* SMPC_MODEL_*                                  */
  float model_dt;
  float temperature;
  float gamma;
  float vx_max, vx_min, vy_max, wz_max; /* base constraints                   */
  float vx_std, vy_std, wz_std;         /* sampling std                       */
  int32_t device;                       /* HIP device ordinal, -1 = current   */
  uint32_t flags;                       /* SMPC_FLAG_*                        */
  /* batch sharding: this ctx holds rows
   * [shard_offset, shard_offset+batch_size) of a global batch of
   * global_batch_size rollouts.  0/0 means "not sharded". */
  uint64_t shard_offset;
  uint64_t global_batch_size;
  /* AckermannConstraints.min_turning_r [ref motion_models.hpp:91-95],
   * default 0.2; read only when motion_model == SMPC_MODEL_ACKERMANN. */
  float ackermann_min_turning_r;
  uint32_t reserved0;
} smpc_config;

/*
 * Critic parameters: the five critics the north star names, each with the
 * parameter names and defaults of its initialize()
 * [ref src/critics/obstacles_critic.cpp:21-51, path_align_critic.cpp:26-44,
 *  path_follow_critic.cpp:23-33, goal_angle_critic.cpp:20-34,
 *  prefer_forward_critic.cpp:20-31].  `enabled` mirrors CriticFunction's
 * enabled_ [ref critic_function.hpp:65-106] AND membership in the YAML
 * `critics` list [ref src/critic_manager.cpp:36-60].
 */
typedef struct smpc_obstacles_params {
  int32_t enabled;
  int32_t consider_footprint; /* 1: SE2 footprint check near obstacles (needs
                                 smpc_set_footprint; the wave-per-rollout pass
                                 at any batch: its lean instance with every
                                 cost_power 1, else the general one).  With
                                 BOTH ObstaclesCritic and CostCritic in the list
                                 and either one's consider_footprint set, the
                                 two disagree on which rollouts collide and a
                                 shard tuple carries one non-colliding count:
                                 smpc_optimize scores such a tick with an extra
                                 counting pass, the sharded tick
                                 (smpc_shard_*) refuses it (SMPC_ERR_UNSUPPORTED) */
  uint32_t cost_power;
  float repulsion_weight;
  float critical_weight;
  float collision_cost;
  float collision_margin_distance;
  float near_goal_distance;
} smpc_obstacles_params;

typedef struct smpc_path_align_params {
  int32_t enabled;
  int32_t use_path_orientations;
  uint32_t cost_power;
  float cost_weight;
  float max_path_occupancy_ratio;
  uint32_t offset_from_furthest;
  uint32_t trajectory_point_step;
  float threshold_to_consider;
} smpc_path_align_params;

typedef struct smpc_path_follow_params {
  int32_t enabled;
  uint32_t cost_power;
  float cost_weight;
  float threshold_to_consider;
  uint32_t offset_from_furthest;
} smpc_path_follow_params;

typedef struct smpc_goal_angle_params {
  int32_t enabled;
  uint32_t cost_power;
  float cost_weight;
  float threshold_to_consider;
} smpc_goal_angle_params;

typedef struct smpc_prefer_forward_params {
  int32_t enabled;
  uint32_t cost_power;
  float cost_weight;
  float threshold_to_consider;
} smpc_prefer_forward_params;

/*
 * The other registered critics of the holonomic stack, scored by
 * the general streaming pass.  `enabled` defaults to 0 (not in the `critics` list).
 * Parameter names and defaults: cost_critic.cpp:25-34, goal_critic.cpp:26-28,
 * constraint_critic.cpp:27-38, twirling_critic.cpp:24-25, path_angle_critic.cpp:24-50,
 * velocity_deadband_critic.cpp:24-33.
 */
typedef struct smpc_cost_params {
  int32_t enabled;
  int32_t consider_footprint; /* 1: SE2 footprint check near obstacles (needs
                                 smpc_set_footprint; the wave-per-rollout pass
                                 at any batch: its lean instance with every
                                 cost_power 1, else the general one)               */
  uint32_t cost_power;
  float cost_weight;          /* as in the YAML (3.81); divided by 254 inside    */
  float critical_cost;
  float collision_cost;
  float near_goal_distance;
} smpc_cost_params;

typedef struct smpc_goal_params {
  int32_t enabled;
  uint32_t cost_power;
  float cost_weight;
  float threshold_to_consider;
} smpc_goal_params;

typedef struct smpc_constraint_params {
  int32_t enabled;
  uint32_t cost_power;
  float cost_weight;
  float vx_max, vy_max, vx_min; /* the controller's vx_max / vy_max / vx_min at
                                   initialize() (constraint_critic.cpp:31-38)     */
} smpc_constraint_params;

typedef struct smpc_twirling_params {
  int32_t enabled;
  uint32_t cost_power;
  float cost_weight;
} smpc_twirling_params;

typedef struct smpc_path_angle_params {
  int32_t enabled;
  uint32_t cost_power;
  float cost_weight;
  uint32_t offset_from_furthest;
  float threshold_to_consider;
  float max_angle_to_furthest;
  int32_t forward_preference;
  float vx_min;                 /* the controller's vx_min: reversing allowed iff
                                   it is negative (path_angle_critic.cpp:24-31)   */
} smpc_path_angle_params;

typedef struct smpc_velocity_deadband_params {
  int32_t enabled;
  uint32_t cost_power;
  float cost_weight;
  float deadband_velocities[3]; /* vx, vy, wz                                     */
} smpc_velocity_deadband_params;

/* Scoring order (CriticManager scores in list order and stops at the first critic that
 * sets fail_flag, critic_manager.cpp:67-76): Constraint, Cost, Obstacles, PathAlign, PathAlignLegacy,
 * PathFollow, GoalAngle, PreferForward, Goal, PathAngle, Twirling, VelocityDeadband.  A
 * different YAML order changes float summation order (last bits) and which costs the
 * discarded all-collide tick carries, nothing else. */
typedef struct smpc_critic_params {
  smpc_obstacles_params obstacles;
  smpc_path_align_params path_align;
  smpc_path_follow_params path_follow;
  smpc_goal_angle_params goal_angle;
  smpc_prefer_forward_params prefer_forward;
  smpc_cost_params cost;
  smpc_goal_params goal;
  smpc_constraint_params constraint;
  smpc_twirling_params twirling;
  smpc_path_angle_params path_angle;
  smpc_velocity_deadband_params velocity_deadband;
  /* PathAlignLegacyCritic (path_align_legacy_critic.cpp:26-44: the parameters of PathAlignCritic,
   * the pre-October-2023 formulation: every trajectory sample against its nearest path point by
   * brute force, :84-124), scored right behind PathAlign by the general pass.  ABI version 2. */
  smpc_path_align_params path_align_legacy;
} smpc_critic_params;

/*
 * Per-tick inputs: what Optimizer::prepare() copies into the optimizer
 * [ref src/optimizer.cpp:185-204] plus the sticky fail flag the critic
 * manager consults [ref src/critic_manager.cpp:67-76].
 */
typedef struct smpc_tick_in {
  double pose_x, pose_y; /* state.pose.pose.position (double in the msg)       */
  float pose_yaw;        /* (float)tf2::getYaw(orientation) [optimizer.cpp:317] */
  double speed_vx, speed_vy, speed_wz; /* state.speed (Twist, double)          */
  const float* path_x;   /* utils::toTensor(plan) [ref tools/utils.hpp:180-192] */
  const float* path_y;
  const float* path_yaw;
  uint32_t path_len;     /* P                                                  */
  double goal_x, goal_y; /* goal.position                                      */
  /* Optional P-1 entries of CriticData::path_pts_valid
   * [ref tools/utils.hpp:361-395]; NULL = derive from the ctx's costmap.     */
  const uint8_t* path_pts_valid;
  /* 1 = CriticData::fail_flag is already set (retry after fallback():
   * CriticManager scores nothing) [ref critic_manager.cpp:70-73].            */
  int32_t fail_flag_in;
  /* GoalChecker::getTolerances(): pose_tolerance.position.x; < 0 = no goal checker
   * (TwirlingCritic's gate, twirling_critic.cpp:33-37, tools/utils.hpp:201-224).       */
  float goal_checker_xy_tolerance;
} smpc_tick_in;

typedef struct smpc_tick_out {
  int32_t fail_flag;        /* all trajectories collide [obstacles_critic.cpp:177] */
  int32_t furthest_valid;   /* furthest_reached_path_point was evaluated           */
  uint32_t furthest_reached_path_point; /* [ref tools/utils.hpp:292-319]           */
  uint32_t non_colliding;   /* rollouts that did not collide (last iteration)      */
  float min_cost;           /* xt::amin(costs_) of the last iteration              */
  float sum_w;              /* sum of exp weights of the last iteration            */
  uint32_t passes;          /* scoring passes over the noise (speculation misses
                               show up as passes > iteration_count)               */
  float device_ms;          /* SMPC_FLAG_PROFILE: GPU time of this call, first upload to
                               last kernel (HIP events on the ctx's stream); else 0 */
  float score_pass_ms;      /* SMPC_FLAG_PROFILE: mean GPU time of one scoring-pass
                               kernel of this call, HIP events around it            */
  uint32_t pass_kind;       /* which streaming pass scored the last iteration:
                               0 smpc_pass (wave per rollout), 1 smpc_pass_lane or
                               smpc_pass_lane_pow (lane per rollout), 2 smpc_pass_split
                               (split horizon)                                      */
} smpc_tick_out;

typedef struct smpc_ctx smpc_ctx;

/* ---- lifetime ---------------------------------------------------------- */

/* Fill *cfg with Optimizer::getParams() defaults [ref src/optimizer.cpp:69-82]
 * (motion model Omni, device -1, flags 0). */
void smpc_config_default(smpc_config* cfg);

/* Fill *p with every critic's initialize() defaults, all five enabled. */
void smpc_critic_params_default(smpc_critic_params* p);

/* Replaces Optimizer::initialize()'s allocation half + reset()
 * [ref src/optimizer.cpp:35-55,116-132].  Control-sequence state is NOT kept
 * in the ctx: u travels through smpc_optimize(u_inout), as control_sequence_
 * stays a host member in the reference. */
int smpc_create(const smpc_config* cfg, smpc_ctx** out);
void smpc_destroy(smpc_ctx* ctx);

/* Text of the last error on this ctx (never NULL).  ctx may be NULL for the
 * last smpc_create() failure of the calling thread. */
const char* smpc_last_error(const smpc_ctx* ctx);

/* ABI version and build string. */
int smpc_abi_version(void);
const char* smpc_build_info(void);

/* ---- configuration ------------------------------------------------------ */

/* NoiseGenerator::reset() half of Optimizer::reset()
 * [ref src/noise_generator.cpp:76-95]: in device-RNG mode re-draws the noise
 * (next draw epoch); in supplied-noise mode keeps the arrays given to
 * smpc_set_noise().  Also drops cached per-tick state. */
int smpc_reset(smpc_ctx* ctx);

/* Current (speed-limited) constraints used by
 * applyControlSequenceConstraints() [ref src/optimizer.cpp:237-249,428-453]. */
int smpc_set_constraints(smpc_ctx* ctx, float vx_max, float vx_min, float vy_max,
                         float wz_max);

/* Acceleration limits on the sampled controls (nav2_mppi_controller's ax_max, ax_min, ay_max,
 * az_max; m/s^2 on vx, on vy — symmetric — and rad/s^2 on wz — symmetric).  With
 *   dhi = model_dt * {ax_max, ay_max, az_max},  dlo = model_dt * {ax_min, -ay_max, -az_max}
 * (products formed once, in float), every iteration turns the stored noise N into the LIMITED
 * noise N' it scores with: per rollout b and control k, sequentially over t, all in float,
 *   last = (float) speed_k
 *   c  = u_k[t] + N_k[b][t];   ct = min(max(c, last + dlo_k), last + dhi_k)
 *   N'_k[b][t] = (ct == c) ? N_k[b][t] : ct - u_k[t];   last = u_k[t] + N'_k[b][t]
 * Every pass of the iteration (furthest-point pre-pass, scoring passes, the critic breakdown)
 * reads N' where it read N: rollout velocities, the gamma term and the weighted update use the
 * limited controls.  Where no limit binds N' == N bit for bit.  vy of a DiffDrive or Ackermann
 * model is not touched.  The stored noise itself is never modified (smpc_get_noise).
 * All four zero: off (the default; nothing is allocated or launched).  Otherwise ax_max > 0,
 * ax_min < 0, ay_max > 0, az_max > 0, all finite; anything else is SMPC_ERR_INVALID.  The limits
 * survive smpc_reset.  (Additions under ABI 3.) */
int smpc_set_acceleration_limits(smpc_ctx* ctx, float ax_max, float ax_min, float ay_max,
                                 float az_max);
int smpc_get_acceleration_limits(const smpc_ctx* ctx, float out[4]);
/* The N' the last tick's last iteration scored with, [B,T] each; any pointer may be NULL (vy of a
 * non-holonomic model: zeros).  SMPC_ERR_STATE when the limits are off or no tick has run. */
int smpc_get_limited_noise(smpc_ctx* ctx, float* noise_vx, float* noise_vy, float* noise_wz);

/* Moving obstacles: discs whose centres are indexed by the trajectory point, scored against every
 * rollout in front of the critics of every iteration.  n discs, 0 <= n <= SMPC_MAX_MOVING_OBSTACLES;
 * disc k has its centre at xy[(k*T + t)*2 + {0,1}] (costmap world frame, T = time_steps) when the
 * robot is at trajectory point t — the indexing of smpc_get_trajectories — and radius[k] > 0 is the
 * centre-to-centre distance below which the robot collides with it (the caller adds the two radii).
 * For rollout b with the trajectory points (x[b][t], y[b][t]) the scoring passes form, in float,
 *   d = sqrtf(dx*dx + dy*dy);   q = clamp((radius[k] + margin - d) / margin, 0, 1)
 *   m(b) = repulsion_weight * (sum over t,k of q) / T + (any d < radius[k] ? collision_cost : 0)
 * and m(b) is what the rollout's cost starts from: iteration 0 scores every critic of the tick on
 * top of m(b), iteration k > 0 on top of (float)((double)cost_prev + m_k(b)) with m_k from that
 * iteration's own control sequence.  Every pass of an iteration starts from the same value.  The
 * term has no cost_power, never sets fail_flag and does not enter non_colliding; a tick with
 * fail_flag_in scores nothing, this term included.
 * smpc_set_moving_obstacles copies before it returns; the table holds from the next tick until it
 * is replaced and survives smpc_reset.  n == 0 (xy, radius and p may be NULL): off — the default;
 * nothing is allocated, uploaded or launched.  collision_cost >= 0, repulsion_weight >= 0,
 * margin > 0, radius > 0, everything finite: anything else is SMPC_ERR_INVALID; n above the maximum
 * is SMPC_ERR_UNSUPPORTED.  (Additions under ABI 3.) */
#define SMPC_MAX_MOVING_OBSTACLES 64
typedef struct smpc_moving_obstacles_params {
  float collision_cost;     /* added once to a rollout that comes closer than radius[k] to a disc */
  float repulsion_weight;
  float margin;             /* metres beyond radius[k] over which q falls from 1 to 0 */
  uint32_t reserved;
} smpc_moving_obstacles_params;
void smpc_moving_obstacles_params_default(smpc_moving_obstacles_params* p);
int smpc_set_moving_obstacles(smpc_ctx* ctx, const smpc_moving_obstacles_params* p, const float* xy,
                              const float* radius, uint32_t n);
/* m [B] and hit [B] (0 / 1; may be NULL) of the last tick's last iteration.  SMPC_ERR_STATE when
 * the term is off, no tick has scored this table yet, or the last tick had fail_flag_in (it scored
 * nothing: an earlier tick's values are not handed out as its own). */
int smpc_get_moving_obstacle_costs(smpc_ctx* ctx, float* m, uint8_t* hit);

int smpc_set_critics(smpc_ctx* ctx, const smpc_critic_params* p);

/* Replaces the Costmap2D* the critics hold
 * [ref src/critics/obstacles_critic.cpp:32,203-224, tools/utils.hpp:361-395].
 * cells: uint8[height*width], index my*width+mx (Costmap2D::getCost).
 * inscribed_radius: LayeredCostmap::getInscribedRadius().
 * cost_scaling_factor / inflation_radius: ObstaclesCritic's parameters of the
 * same name, read only when the costmap has an InflationLayer
 * [ref obstacles_critic.cpp:70-80]; pass 0,0 when it has none. */
int smpc_set_costmap(smpc_ctx* ctx, const uint8_t* cells, uint32_t width,
                     uint32_t height, double origin_x, double origin_y,
                     double resolution, int track_unknown, float inscribed_radius,
                     float cost_scaling_factor, float inflation_radius);

/* Costmap hand-off at the controller's rate.  The reference holds a
 * Costmap2D* and reads it under the costmap mutex during the tick
 * [ref src/controller.cpp:99-103]; a device needs its own copy.  smpc_set_costmap() may be
 * called every tick: it keeps a pinned host mirror, uploads only the band of rows that
 * changed since the previous call (nothing for an unchanged map of the same size; the
 * lookup tables are rebuilt only when resolution / inflation parameters change) and
 * returns without waiting for the DMA — the next tick is ordered behind it.
 * A caller that knows the updated window (Costmap2D's updated bounds) can hand over just
 * that: `cells` points at the window's first cell inside the caller's map, whose rows are
 * `row_stride` bytes apart; geometry and parameters stay those of the last
 * smpc_set_costmap(). */
int smpc_update_costmap_region(smpc_ctx* ctx, const uint8_t* cells, uint32_t row_stride,
                               uint32_t x0, uint32_t y0, uint32_t width, uint32_t height);
/* Bytes uploaded by the last smpc_set_costmap / smpc_update_costmap_region call, and in
 * total (either pointer may be NULL). */
int smpc_costmap_upload_bytes(const smpc_ctx* ctx, uint64_t* last_call, uint64_t* total);

/* Supplied-noise (parity) mode: the three [B,T] row-major noise tensors
 * NoiseGenerator holds [ref tools/noise_generator.hpp:97-99], already scaled
 * by the sampling std.  Host pointers; copied. */
/* The robot footprint for consider_footprint = true (ObstaclesCritic, CostCritic): n_points
 * (x, y) pairs in the robot frame (costmap_ros->getRobotFootprint()), the layered costmap's
 * circumscribed radius, and the inflation layer's own cost_scaling_factor (< 0: the costmap
 * has no inflation layer) — what {Obstacles,Cost}Critic::findCircumscribedCost and
 * FootprintCollisionChecker::footprintCostAtPose consume [ref obstacles_critic.cpp:52-97,
 * 203-224, cost_critic.cpp:62-106,175-201].  At most SMPC_MAX_FOOTPRINT points. */
#define SMPC_MAX_FOOTPRINT 16
int smpc_set_footprint(smpc_ctx* ctx, const double* xy, uint32_t n_points,
                       double circumscribed_radius, double layer_cost_scaling_factor);

int smpc_set_noise(smpc_ctx* ctx, const float* noise_vx, const float* noise_vy,
                   const float* noise_wz);

/* Device-RNG mode: Philox4x32-10 + Box–Muller, draw order vx, wz, vy
 * [ref src/noise_generator.cpp:107-122].  Draw epoch 0 is drawn here; each
 * smpc_reset() draws the next epoch (the reference's first tick also runs on
 * its second draw, optimizer.cpp:52-54). */
int smpc_seed(smpc_ctx* ctx, uint64_t seed);

/* NoiseGenerator::generateNextNoises() with regenerate_noises = true
 * [ref src/noise_generator.cpp:54-63,97-105]: draw the next epoch's noise now
 * (device-RNG mode only; constraints and costs are left alone). */
int smpc_redraw_noise(smpc_ctx* ctx);
/* The same draw OFF the tick's critical path, as the reference runs it (a thread draws the next
 * tensors while the optimizer goes on, noise_generator.cpp:54-63,97-105): the next epoch is drawn
 * into a second set of tensors on a stream of its own and the call returns at once; the next
 * tick (smpc_optimize, smpc_shard_begin / _tick, smpc_group_optimize) waits for the draw on the
 * device and scores with it.  A second call before a tick has taken the first draw is a no-op;
 * smpc_seed / smpc_reset / smpc_set_noise / smpc_redraw_noise drop a draw not yet taken.  Doubles
 * the noise tensors' memory (allocated at the first call). */
int smpc_redraw_noise_async(smpc_ctx* ctx);

/* Copy the ctx's noise tensors back (tests / RNG parity). Any pointer may be NULL. */
int smpc_get_noise(smpc_ctx* ctx, float* noise_vx, float* noise_vy, float* noise_wz);

/* ---- the hot path -------------------------------------------------------- */

/* Replaces the body of Optimizer::optimize() [ref src/optimizer.cpp:157-164]:
 * iteration_count x { generateNoisedTrajectories (:227-233),
 * CriticManager::evalTrajectoriesScores (critic_manager.cpp:67-76),
 * updateControlSequence (:362-394) }, costs_ zeroed once per call as
 * prepare() does (:197).
 * u_inout: control_sequence_ as 3*T floats {vx[T], vy[T], wz[T]}, host memory. */
int smpc_optimize(smpc_ctx* ctx, const smpc_tick_in* in, float* u_inout,
                  smpc_tick_out* out);

/* Optimizer::getGeneratedTrajectories() [ref src/optimizer.cpp:455-458]:
 * x, y, yaws [B,T] of the last scoring pass.  Needs
 * SMPC_FLAG_STORE_TRAJECTORIES.  Any pointer may be NULL. */
int smpc_get_trajectories(smpc_ctx* ctx, float* x, float* y, float* yaws);

/* costs_ [B] after the last iteration (incl. the gamma terms of
 * updateControlSequence) [ref include/.../optimizer.hpp:255]. */
int smpc_get_costs(smpc_ctx* ctx, float* costs);

/* ---- critic statistics: which critic steers a tick, and how many rollouts carry weight ------
 * (What upstream Nav2 publishes as `publish_critics_stats`; the reference fork predates it.)
 * Ids of the registered critics in the scoring order above, and one pseudo-row for the gamma
 * term of updateControlSequence [ref src/optimizer.cpp:365-380]. */
#define SMPC_N_CRITICS 12
#define SMPC_CRITIC_CONSTRAINT 0
#define SMPC_CRITIC_COST 1
#define SMPC_CRITIC_OBSTACLES 2
#define SMPC_CRITIC_PATH_ALIGN 3
#define SMPC_CRITIC_PATH_ALIGN_LEGACY 4
#define SMPC_CRITIC_PATH_FOLLOW 5
#define SMPC_CRITIC_GOAL_ANGLE 6
#define SMPC_CRITIC_PREFER_FORWARD 7
#define SMPC_CRITIC_GOAL 8
#define SMPC_CRITIC_PATH_ANGLE 9
#define SMPC_CRITIC_TWIRLING 10
#define SMPC_CRITIC_VELOCITY_DEADBAND 11
#define SMPC_STATS_CONTROL 12
#define SMPC_STATS_ROWS 13

/* The critic's class name as nav2_plugin/critics.xml registers it ("ConstraintCritic", ...);
 * "ControlCost" for SMPC_STATS_CONTROL; NULL for any other id.  Needs no device. */
const char* smpc_critic_name(uint32_t id);

/* Row k of a rollout is the value CriticManager's k-th critic added to its cost,
 * (float)pow(v_k, cost_power_k) [ref e.g. src/critics/goal_critic.cpp:44-54]; row 12 the float
 * sum of the three gamma terms.  The rows of a rollout add up to its entry of smpc_get_costs
 * to within float rounding. */
typedef struct smpc_critic_stats {
  uint32_t scored_mask;              /* bit k: row k was scored on this tick */
  uint32_t fail_flag;                /* as smpc_tick_out.fail_flag would be */
  uint32_t batch;                    /* rollouts reduced */
  uint32_t best_rollout;             /* least total cost, lowest index among ties */
  float    best_cost, effective_samples; /* (sum w)^2 / sum w^2, w the tick's softmax weights */
  float    sum[13], min[13], max[13]; /* over the rollouts; rows not in scored_mask hold zeros */
  float    weighted[13];             /* sum_b w_b t_kb / sum_b w_b */
  float    at_best[13];              /* the row's value for best_rollout */
} smpc_critic_stats;

/* Break down the tick smpc_optimize(ctx, in, u_in) would run: what its FIRST iteration scores —
 * the same noise, the same host gates, the true furthest point (a furthest-point pre-pass, no
 * speculation), the same all-collide rule: when every rollout collides fail_flag is 1 and mask
 * and rows are those of the re-score [ref critic_manager.cpp:70-73]; with in->fail_flag_in
 * nothing is scored and the mask holds only the control row.  Scored by the general pass
 * whatever pass the tick itself takes.  per_rollout: NULL, or [SMPC_STATS_ROWS][batch_size]
 * floats, row-major.  Changes nothing a later tick depends on: u_in is read only, costs,
 * furthest-point prediction and counters of the ctx stay as they are.  Its device buffers
 * (SMPC_STATS_ROWS + 1 floats per rollout) are allocated at the first call.  A member of an
 * smpc_group returns SMPC_ERR_STATE; a tick that needs the counting pass of two collision
 * critics with a footprint returns SMPC_ERR_UNSUPPORTED; on a shard ctx the numbers are the
 * shard's own.  (An addition under ABI 3, like smpc_group_optimize_some.) */
int smpc_critic_breakdown(smpc_ctx* ctx, const smpc_tick_in* in, const float* u_in,
                          smpc_critic_stats* stats, float* per_rollout);

/* ---- trajectory validation: a collision check of the tick's RESULT -------------------------------
 * (What upstream Nav2's MPPI controller runs behind optimize() as its optimal-trajectory validator;
 * the reference fork predates it.)  A tick returns the softmax-weighted mean of the sampled control
 * sequences and nothing checks that mean: fail_flag fires only when every rollout collides, and a
 * rollout that hits a moving obstacle is made expensive, never refused.  This call integrates a
 * control sequence from a pose and checks the poses it passes through.
 *   poses    the T poses of Optimizer::getOptimizedTrajectory: u = {vx[T], vy[T], wz[T]} ITSELF
 *            integrated from the pose (no measured-speed first column), float sums,
 *            x = (float)(pose_x + (double)sum); vy is ignored for DiffDrive and Ackermann;
 *   checked  the first n = min(T, (uint32_t)floorf(collision_lookahead_time / model_dt)) of them, the
 *            quotient formed in float (2.0f / 0.05f is 40); n == 0 checks nothing and is valid;
 *   costmap  CostCritic's own rule on pose t < n [ref cost_critic.cpp:136-146,175-210]: the cost c
 *            under the centre (Costmap2D::worldToMap; off the map: 255); c < 1 is free; with
 *            consider_footprint, where c >= the possibly-inscribed cost (findCircumscribedCost) or
 *            that cost is < 1, c becomes the footprint cost at the pose (footprintCostAtPose, a
 *            vertex off the map: 254); 254 collides, 253 collides unless consider_footprint, 255
 *            collides unless the costmap tracks unknown space;
 *   discs    with moving_obstacles set and a table on the ctx (smpc_set_moving_obstacles), pose t
 *            hits disc k iff sqrtf(dx*dx + dy*dy) < radius[k] against xy[k][t], in float;
 *   result   valid; checked = n; first_bad, the least colliding t; cause at first_bad (1 costmap,
 *            2 disc; the costmap wins); cost, the c above at first_bad; disc, the least k that is
 *            hit at first_bad (0 when none is).  A valid result has first_bad = cause = disc = 0
 *            and cost = 0.
 * xyyaw: NULL, or T*3 floats {x, y, yaw} per pose — all T, whatever n.
 * One upload, one launch (csrc/smpc_validate.hip) and one wait on the ctx's stream, behind a costmap
 * upload still pending there.  Changes nothing a tick depends on.  SMPC_ERR_INVALID: a null argument,
 * a lookahead that is not > 0 and finite; SMPC_ERR_STATE: no costmap yet, consider_footprint without
 * smpc_set_footprint, a member of a group (as smpc_critic_breakdown).  Buffers (a few KB) are
 * allocated at the first call.  (Additions under ABI 3.) */
typedef struct smpc_validation_params {
  float collision_lookahead_time;   /* seconds; default 2.0 */
  int32_t consider_footprint;       /* default 0   */
  int32_t moving_obstacles;         /* default 1   */
  uint32_t reserved;
} smpc_validation_params;

#define SMPC_VALIDATION_CAUSE_COSTMAP 1u
#define SMPC_VALIDATION_CAUSE_DISC 2u
typedef struct smpc_validation {
  int32_t valid;
  uint32_t checked, first_bad, cause, disc;
  float cost;
} smpc_validation;

void smpc_validation_params_default(smpc_validation_params* p);

int smpc_validate_trajectory(smpc_ctx* ctx, const smpc_validation_params* p, double pose_x, double pose_y,
                             float pose_yaw, const float* u, smpc_validation* out,
                             float* xyyaw /* NULL or T*3 */);

/* Diagnostics: the device sin/cos the rollout uses (integrateStateVelocities,
 * ref src/optimizer.cpp:326-329), evaluated on n host values; tests pin its error. */
int smpc_selftest_sincos(smpc_ctx* ctx, const float* x, uint32_t n, float* sin_out,
                         float* cos_out);
/* Diagnostics: the device Philox4x32-10 of the noise generator on n caller-given counters
 * ctr[4n] under one key; out[4n] are the four words of each block.  Tests compare them with
 * the published known answers and an integer model, bit for bit. */
int smpc_selftest_philox(smpc_ctx* ctx, const uint32_t* ctr, const uint32_t key[2], uint32_t n,
                         uint32_t* out);
/* Diagnostics: the device Box-Muller of the noise generator on n pairs of Philox words:
 * z0 = radius cos, z1 = radius sin of N(0, 1), before the multiplication by a std. */
int smpc_selftest_box_muller(smpc_ctx* ctx, const uint32_t* r0, const uint32_t* r1, uint32_t n,
                             float* z0, float* z1);
/* Diagnostics: the in-register 64 x 64 transpose-reduce of the lane-per-rollout pass
 * (updateControlSequence's weighted sum, ref src/optimizer.cpp:382-393):
 * out[t] = sum_b w[b] * v[b*64 + t], b, t = 0..63. */
int smpc_selftest_lane_reduce(smpc_ctx* ctx, const float* v, const float* w, float* out);

/* ---- batch-sharded path; one ctx per GPU ------------------
 * A tick on G shards is
 *   begin -> [furthest -> MAX over ranks] -> score -> all-gather -> combine
 * where the bracketed exchange is skipped when the caller speculates on the
 * furthest point (score() reports the true local value in its tuple and the
 * caller re-scores on a miss).  The two exchanges are done by the caller
 * (RCCL through torch.distributed in bench.py); the library never blocks on a
 * peer.  All device pointers must be on this ctx's device and all work is
 * enqueued on the stream given to smpc_set_stream(). */

/* hipStream_t to enqueue on.  NULL is HIP's default (null) stream — what
 * torch.cuda.current_stream() is unless the caller changed it;
 * SMPC_STREAM_OWN goes back to the ctx's own non-blocking stream. */
#define SMPC_STREAM_OWN ((void*)(intptr_t)-1)
int smpc_set_stream(smpc_ctx* ctx, void* hip_stream);

/* Turn SMPC_FLAG_PROFILE on/off after creation (event records cost ~15 us of host and
 * queue time per tick, so throughput is measured with it off). */
int smpc_set_profile(smpc_ctx* ctx, int enable);

#define SMPC_TUPLE_HEADER 4 /* floats before U: min, sum_w, furthest, non_colliding */
/* Length in floats of one shard tuple: SMPC_TUPLE_HEADER + 3*T. */
uint32_t smpc_tuple_len(const smpc_ctx* ctx);

/* (The sharded tick — these phases and smpc_shard_tick — runs ONE iteration per tick: a ctx with
 * iteration_count != 1 is refused with SMPC_ERR_UNSUPPORTED, as is consider_footprint with both
 * collision critics in the list.)
 * Upload the tick's inputs and control sequence (host pointers).  Everything the later phases
 * of the tick need (smpc_shard_combine feeds the path and the pose to the furthest-point
 * predictor) is copied before this returns: *in, its arrays and u_in are the caller's again. */
int smpc_shard_begin(smpc_ctx* ctx, const smpc_tick_in* in, const float* u_in);
/* The furthest reached path point this tick is expected to have: the previous tick's value
 * (as smpc_shard_combine saw it) carried forward by the robot's motion, the plan's pruning and
 * the last tick's drift — what smpc_optimize and smpc_shard_tick speculate with.  Returns 1 and
 * writes *hint when there is a prediction (smpc_shard_begin of this tick has run and an
 * earlier tick's smpc_shard_combine reported a furthest point), else 0.  Every rank computes
 * the same value from the same inputs.  Scoring with it is exact either way: the combined
 * tuple reports the true value and a caller that finds a mismatch scores again. */
int smpc_shard_predicted_furthest(smpc_ctx* ctx, uint32_t* hint);
/* Local max over this shard of the nearest-path-point index of each rollout's
 * endpoint [ref tools/utils.hpp:292-319], written as one float to d_furthest. */
int smpc_shard_furthest(smpc_ctx* ctx, float* d_furthest);
/* Score this shard with the batch-wide furthest point read from d_furthest
 * (device, one float) or, if d_furthest is NULL, furthest_hint; writes the
 * shard tuple {min cost, sum w, true local furthest, non-colliding count,
 * sum w*cvx[T], sum w*cvy[T], sum w*cwz[T]} to d_tuple (device). */
int smpc_shard_score(smpc_ctx* ctx, const float* d_furthest, uint32_t furthest_hint,
                     float* d_tuple);
/* After smpc_shard_combine() reported fail_flag = 1 on a tick that did not
 * start with fail_flag_in: the reference scored no critic past Obstacles
 * [ref critic_manager.cpp:70-73].  Re-score this shard that way into d_tuple;
 * the caller gathers and combines again. */
int smpc_shard_rescore_failed(smpc_ctx* ctx, float* d_tuple);
/* Combine n_tuples shard tuples (device, contiguous) into the new control
 * sequence: rescale by exp(-(min_g - min)/temperature), divide, clip
 * [ref src/optimizer.cpp:382-393]; copies u (3*T) to host and fills *out.
 * Synchronises the stream. */
int smpc_shard_combine(smpc_ctx* ctx, const float* d_tuples, uint32_t n_tuples,
                       float* u_out, smpc_tick_out* out);

/* ---- several planning instances per launch (multi-robot fleets; BASELINE "multi-query") ----
 * Independent contexts (own noise, costmap, critics, control sequence) on one GPU whose
 * ticks are issued together: one upload, one scoring launch per scoring instance with the member
 * as the second grid dimension, one reduction launch — and, for the riding members with moving
 * obstacles, one launch of the moving-obstacle term per form of it (at most three: the noise
 * layout and the motion model decide the form) in front of the scoring launches, the member as
 * the second grid dimension there too.  Results are exactly those of
 * smpc_optimize on each context, bit for bit.
 * Which members ride a batched launch:
 *   - members whose tick takes the lane-per-rollout pass (SMPC_FLAG_LANE_PER_ROLLOUT, or a batch
 *     large enough for it; the five critics or the deployed list's cruise tick): one launch of a
 *     grouped lane instance for all of them;
 *   - members whose tick takes the wave-per-rollout pass with time_steps <= 64 and every
 *     cost_power == 1 — the deployed critic list with or without consider_footprint, near-goal
 *     ticks, any context created without the lane flag: one launch of smpc_pass_many per distinct
 *     instance that at least two members chose.  The lane flag is not required.
 * Which members are ticked on their own inside the call (smpc_optimize): time_steps > 64, a
 * cost_power other than 1, SMPC_FLAG_STORE_TRAJECTORIES, path orientations, the critics of the
 * general pass, the Ackermann model, iteration_count > 1, fail_flag_in, SMPC_FLAG_NO_SPECULATION or
 * SMPC_FLAG_PROFILE, the only member on its instance; and, for the tick at hand, a member without
 * a furthest-point guess (its first tick), one whose guess missed, one whose rollouts all collide.
 * Members must share device and time_steps; while grouped, a context must not be used through
 * smpc_optimize directly; destroy the group before its members.  Replaces N calls of
 * Optimizer::optimize() [ref src/optimizer.cpp:157-164] by N controller instances.
 * A round that returns an error may have been abandoned between its launches and the last
 * member's result: the group remembers that, and the next round waits for the group's stream
 * before it writes the shared tick blocks and argument arrays again.  The next round is safe. */
typedef struct smpc_group smpc_group;
int smpc_group_create(smpc_ctx* const* ctxs, uint32_t n, smpc_group** out);
void smpc_group_destroy(smpc_group* group);
/* ins[n], u_inout[n] (pointers to 3*T floats each), outs[n] (may be NULL) */
int smpc_group_optimize(smpc_group* group, const smpc_tick_in* ins, float* const* u_inout,
                        smpc_tick_out* outs);
/* The same round over a subset: take[n], one byte per member; take == NULL, or every byte non-zero,
 * is smpc_group_optimize exactly (which is a call of this).  A member with take[i] == 0 is not
 * prepared, uploaded, launched or fetched: ins[i], u_inout[i] and outs[i] are neither read nor
 * written (the pointers may be NULL), its device and host state — furthest-point prediction,
 * costs, a pending smpc_redraw_noise_async, the tick number — stays as it is, and its next tick is
 * bit for bit what it would have been without this round: the controller is simply not called
 * for a robot without a plan [ref src/controller.cpp:80-116].  The rules above on who rides a
 * batched launch apply to the members taken (an instance needs two riding members).  A round
 * with nobody taken returns SMPC_OK and does nothing.  An addition under ABI 3: the number is
 * pinned by the suite and no existing entry point or struct changed; a caller that must run
 * against an older library looks the symbol up. */
int smpc_group_optimize_some(smpc_group* group, const smpc_tick_in* ins, float* const* u_inout,
                             smpc_tick_out* outs, const uint8_t* take);
/* How the group's ticks went so far: *batched_launches counts scoring launches that carried two or
 * more members, *single_ticks members ticked through smpc_optimize (a re-score after a missed guess
 * included).  Either pointer may be NULL; a NULL group returns SMPC_ERR_INVALID.  (ABI 3) */
int smpc_group_stats(const smpc_group* group, uint64_t* batched_launches, uint64_t* single_ticks);
/* smpc_set_moving_obstacles for the members of a group in one call: params[n], xy[n] (member i:
 * [n_discs[i]][T][2] floats), radius[n] (member i: [n_discs[i]] floats), n_discs[n], take[n] as in
 * smpc_group_optimize_some (NULL: every member).  For every member taken the meaning is exactly
 * smpc_set_moving_obstacles(member, &params[i], xy[i], radius[i], n_discs[i]): the same checks, the
 * same table, n_discs[i] == 0 switches the member's term off (its pointers may be NULL); a member
 * that is not taken keeps its table, whoever set it.  Every member taken is checked before
 * anything is written: a call that returns an error has changed no member, the message is in that
 * member's smpc_last_error and smpc_last_error(NULL) names the member.
 * What differs is the transport: the tables of all members are packed back to back into ONE pinned
 * buffer of the group's and go up as ONE copy on the group's stream into ONE device allocation of
 * the group's, behind one event, nothing waited for — their number does not depend on n.
 * The last call wins: a later smpc_set_moving_obstacles on a member replaces that member's table
 * with one in the member's own buffer, as ever.  A table set here belongs to the group:
 * smpc_group_destroy switches the term off for every member whose table still lives in the
 * group's buffer (as n == 0 does); a member whose table was set through its own handle keeps it.
 * (An addition under ABI 3, like smpc_group_optimize_some.) */
int smpc_group_set_moving_obstacles(smpc_group* group, const smpc_moving_obstacles_params* params,
                                    const float* const* xy, const float* const* radius,
                                    const uint32_t* n_discs, const uint8_t* take);

/* smpc_critic_breakdown for the members of a group, the group staying a group: ins[n], u_ins[n]
 * (3*T floats each, read only), take[n] as in smpc_group_optimize_some (NULL: every member),
 * stats[n], per_rollout (NULL, or n pointers of which any may be NULL; else
 * [SMPC_STATS_ROWS][batch_size] floats of that member), status[n].
 * For every member taken, stats[i] and per_rollout[i] are bit for bit what smpc_critic_breakdown
 * returns on an identical context that is in no group — the first iteration's flags, the same
 * noise (limited, where the member has acceleration limits) and host gates, the true furthest
 * point, the all-collide re-score, fail_flag_in — and status[i] is SMPC_OK or the code that call
 * would have returned (SMPC_ERR_UNSUPPORTED for both collision critics with a footprint, a refused
 * plan, ...), the message in that member's smpc_last_error.  A member that fails this way does not
 * fail the others.  stats[i], per_rollout[i] and status[i] of a member that is not taken are
 * neither read nor written, and nothing of it is prepared.
 * With time_steps <= 64 the members taken ride ONE furthest-point pre-pass (those whose critics
 * need it), ONE launch of smpc_pass_stats_many and ONE pair of reduction launches, behind one
 * memset and one upload, in front of one copy back and one wait: their number does not depend on
 * n.  A member whose rollouts all collide is re-scored behind that, on its own.  Members of a
 * group with time_steps > 64 are scored one by one inside the call, with the same results (as
 * smpc_pass_many has no instance for them either).
 * Changes nothing a later round depends on, for any member: control sequences, costs, result
 * blocks, furthest-point prediction, launch plan and counters stay, and so do the two counters of
 * smpc_group_stats.  The float regions live in one allocation of the group's, sized at the first
 * call and again when the members taken or their batch sizes need more.
 * Returns an error only for NULL arguments (before any member is touched), when no member is
 * taken, or for a device error; a call that follows an abandoned round waits for the group's
 * stream first, as a round does.  (An addition under ABI 3, like smpc_group_optimize_some.) */
int smpc_group_critic_breakdown(smpc_group* group, const smpc_tick_in* ins,
                                const float* const* u_ins, const uint8_t* take,
                                smpc_critic_stats* stats, float* const* per_rollout,
                                int32_t* status);
/* Which way the member-breakdowns of smpc_group_critic_breakdown went so far: *batched_members
 * counts those that rode a grouped stats launch, *single_members those scored one by one
 * (time_steps > 64).  Either pointer may be NULL; a NULL group returns SMPC_ERR_INVALID.  (ABI 3) */
int smpc_group_breakdown_counts(const smpc_group* group, uint64_t* batched_members,
                                uint64_t* single_members);

/* smpc_validate_trajectory for the members of a group, the group staying a group: params[n],
 * poses[n][3] ({x, y, yaw} as doubles; yaw is rounded to float), u[n] (3*T floats each, read only),
 * take[n] as in smpc_group_optimize_some (NULL: every member), out[n], xyyaw (NULL, or n pointers of
 * which any may be NULL), status[n].  For every member taken out[i] and xyyaw[i] are bit for bit what
 * smpc_validate_trajectory returns on an identical context that is in no group, and status[i] is
 * SMPC_OK or the code that call would have returned, the message in that member's smpc_last_error; a
 * member that fails this way does not fail the others.  Entries of a member that is not taken are
 * neither read nor written.  ONE upload, ONE launch and ONE wait on the group's stream, whatever n;
 * a moving-obstacle table the group owns (smpc_group_set_moving_obstacles) is read where it lives.
 * Changes nothing a later round depends on, the counters of smpc_group_stats included.  Returns an
 * error only for NULL arguments, when no member is taken, or for a device error; a call that follows
 * an abandoned round waits for the group's stream first, as a round does.  (ABI 3) */
int smpc_group_validate_trajectories(smpc_group* group, const smpc_validation_params* params /*[n]*/,
                                     const double* poses /*[n][3]*/, const float* const* u,
                                     const uint8_t* take, smpc_validation* out,
                                     float* const* xyyaw, int32_t* status);
/* *launches counts the launches of smpc_group_validate_trajectories so far (one per call that had a
 * member to check), *members the members they carried.  Either pointer may be NULL; a NULL group
 * returns SMPC_ERR_INVALID.  (ABI 3) */
int smpc_group_validation_counts(const smpc_group* group, uint64_t* launches, uint64_t* members);

/* ---- the same tick with the exchanges inside the library (RCCL over xGMI) ----
 * One ncclComm per ctx, one call per tick: upload -> score -> ncclAllGather(tuples) ->
 * combine -> wait, all on the ctx's stream (speculate != 0: the furthest point of the
 * previous tick is used and the tick is re-scored on a miss; else an
 * ncclAllReduce(MAX) of the furthest point precedes the scoring pass).  RCCL is
 * resolved at run time (dlopen of librccl.so, sharing the copy the process already
 * holds, e.g. torch.distributed's): a single-GPU user never loads it.
 *   rank 0: smpc_shard_comm_id(id, SMPC_COMM_ID_BYTES); ship the bytes to every rank;
 *   every rank: smpc_shard_comm_init(ctx, id, rank, world)  (collective);
 *   per tick:   smpc_shard_tick(ctx, &in, u, &out, 1)       (collective).
 * Replaces, for a sharded deployment, the Optimizer::optimize() call of
 * ref src/optimizer.cpp:133-148. */
#define SMPC_COMM_ID_BYTES 128
int smpc_shard_comm_id(void* id_out, uint32_t id_bytes);
int smpc_shard_comm_init(smpc_ctx* ctx, const void* id, int rank, int world);
int smpc_shard_tick(smpc_ctx* ctx, const smpc_tick_in* in, float* u_inout, smpc_tick_out* out,
                    int speculate);

/* The same tick with NO collective (the exchange is a few hundred bytes per rank: a library
 * collective costs more in latency than it moves).  Every rank owns a mailbox in peer-visible
 * device memory; smpc_shard_p2p_handle() creates it and returns its IPC handle
 * (SMPC_P2P_HANDLE_BYTES), the caller hands every rank the handles of all ranks (rank order,
 * world * SMPC_P2P_HANDLE_BYTES bytes) and smpc_shard_p2p_init() maps them; the ranks must
 * synchronise (any barrier) between that call and their first tick.  From then on
 * smpc_shard_tick() exchanges through the mailboxes: the finishing kernel of a rank writes its
 * tuple into its peers' memory over xGMI and waits for theirs.  The wait is bounded in
 * wall-clock time (default 10 000 ms, smpc_shard_p2p_set_timeout): it has to cover the skew
 * between the ranks' calls, not just the exchange.  A peer that does not answer in time makes
 * the tick fail with SMPC_ERR_DEVICE, it does not hang; the failed rank then stops publishing
 * and every later smpc_shard_tick on it returns SMPC_ERR_STATE, so its peers fail at their
 * next exchange at the latest (they may have completed the tick the failed rank lost: treat
 * any failure as "exchange down on all ranks": smpc_shard_p2p_init again on every rank, then
 * smpc_reset).  At most SMPC_P2P_MAX_WORLD ranks, all on one node; the Omni and DiffDrive
 * models (smpc_shard_p2p_init refuses an Ackermann ctx).  This exchange is an opt-in
 * optimisation; the RCCL exchange above is the default a sharded deployment should start with. */
#define SMPC_P2P_HANDLE_BYTES 64
#define SMPC_P2P_MAX_WORLD 16
int smpc_shard_p2p_handle(smpc_ctx* ctx, void* handle_out, uint32_t handle_bytes);
int smpc_shard_p2p_init(smpc_ctx* ctx, const void* handles, int rank, int world);
int smpc_shard_p2p_set_timeout(smpc_ctx* ctx, uint32_t milliseconds);

#ifdef __cplusplus
}
#endif
#endif /* SMPC_H_ */
