/*
 * smpc_host.h — C face of the C++ host optimizer (mpcholonavigation_amd/host/
 * optimizer.hpp, class sortham::Optimizer).  It exists so that tests (and
 * non-C++ callers) can drive the host logic that stays on the CPU in the
 * reference — Optimizer::evalControl and friends [ref src/optimizer.cpp:116-225,
 * 396-453] — through plain C.  A Nav2 build links the C++ class directly
 * (INTEGRATION.md).  Exceptions the reference throws become
 * SORTHAM_ERR_THROWN with the message in sortham_optimizer_last_error().
 */
#ifndef SMPC_HOST_H_
#define SMPC_HOST_H_

#include "smpc.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SORTHAM_ERR_THROWN -10 /* std::runtime_error where the reference throws */

typedef struct sortham_optimizer sortham_optimizer;

typedef struct sortham_optimizer_config {
  smpc_config base;             /* batch/horizon/iterations, dt, temperature, gamma,
                                   base constraints, sampling std, device; of flags,
                                   SMPC_FLAG_LANE_PER_ROLLOUT alone is passed on    */
  double controller_frequency;  /* setOffset [ref src/optimizer.cpp:95-114]         */
  uint32_t retry_attempt_limit; /* [ref :82]                                        */
  int32_t regenerate_noises;    /* [ref src/noise_generator.cpp:35]                 */
  int32_t visualize;            /* keep generated trajectories readable             */
  uint64_t noise_seed;
  /* YAML `critics` list: up to 16 names without the namespace, e.g.
   * "ObstaclesCritic" [ref src/critic_manager.cpp:36-65]                          */
  const char* critics[16];
  uint32_t n_critics;
  float cost_scaling_factor, inflation_radius; /* ObstaclesCritic params           */
  const char* motion_model;     /* "Omni" [ref :84]                                 */
} sortham_optimizer_config;

int sortham_optimizer_create(const sortham_optimizer_config* cfg, const smpc_critic_params* critics,
                             sortham_optimizer** out);
/* Optimizer::initialize() again on a live object: what the plugin's reset() does after every
 * idle period and on a parameter change [ref src/optimizer.cpp:46-60,116-132,
 * src/controller.cpp:89-92].  An unchanged configuration (shapes, model, sampling, seed) keeps
 * the device context and only resets state and re-draws the noise; anything else rebuilds it. */
int sortham_optimizer_initialize(sortham_optimizer* o, const sortham_optimizer_config* cfg,
                                 const smpc_critic_params* critics);
void sortham_optimizer_destroy(sortham_optimizer* o);
const char* sortham_optimizer_last_error(const sortham_optimizer* o);

int sortham_optimizer_set_costmap(sortham_optimizer* o, const uint8_t* cells, uint32_t width,
                                  uint32_t height, double origin_x, double origin_y,
                                  double resolution, int track_unknown, float inscribed_radius,
                                  int has_inflation_layer);
/* The robot footprint for consider_footprint = true, with the arguments, the limit
 * (SMPC_MAX_FOOTPRINT points) and the meaning of smpc_set_footprint: n_points (x, y) pairs in the
 * robot frame, the layered costmap's circumscribed radius, the inflation layer's own
 * cost_scaling_factor (< 0: no inflation layer).  What the C++ class takes in
 * CostmapView::footprint_xy and its neighbours.  Applies from the next tick on, whatever the order
 * of this call and sortham_optimizer_set_costmap, and survives sortham_optimizer_initialize.
 * SMPC_ERR_INVALID for a null argument or no point, SMPC_ERR_UNSUPPORTED for too many. */
int sortham_optimizer_set_footprint(sortham_optimizer* o, const double* xy, uint32_t n_points,
                                    double circumscribed_radius, double layer_cost_scaling_factor);
int sortham_optimizer_set_noise(sortham_optimizer* o, const float* nvx, const float* nvy,
                                const float* nwz);
/* Optimizer::evalControl: in carries pose / speed / plan / goal (fail_flag_in ignored);
 * twist_out = {linear.x, linear.y, angular.z}. */
int sortham_optimizer_eval_control(sortham_optimizer* o, const smpc_tick_in* in, double* twist_out,
                                   smpc_tick_out* out);
/* Optimizer::getCriticStats: per-critic costs and effective samples (smpc.h: smpc_critic_breakdown)
 * of the tick sortham_optimizer_eval_control(o, in, ...) would run next, from the control sequence
 * as it stands; in as for eval_control.  Changes nothing: eval_control afterwards returns what it
 * would have returned without the call.  per_rollout: NULL or [SMPC_STATS_ROWS][batch_size] floats. */
int sortham_optimizer_critic_stats(sortham_optimizer* o, const smpc_tick_in* in, smpc_critic_stats* stats,
                                   float* per_rollout);
/* The smpc_tick_out of the last tick the object ran — the last retry's when eval_control threw. */
int sortham_optimizer_last_tick(const sortham_optimizer* o, smpc_tick_out* out);
int sortham_optimizer_set_speed_limit(sortham_optimizer* o, double speed_limit, int percentage);
/* Optimizer::setAccelerationLimits: the limits of smpc_set_acceleration_limits (all zero: off).
 * Before or after initialize; kept across reset and across a re-initialize. */
int sortham_optimizer_set_acceleration_limits(sortham_optimizer* o, float ax_max, float ax_min,
                                              float ay_max, float az_max);
/* Optimizer::setMovingObstacles / clearMovingObstacles (n == 0): the table of
 * smpc_set_moving_obstacles, xy [n][time_steps][2], radius [n].  Before or after initialize; kept
 * across reset and across a re-initialize. */
int sortham_optimizer_set_moving_obstacles(sortham_optimizer* o, const smpc_moving_obstacles_params* params,
                                           const float* xy, const float* radius, uint32_t n,
                                           uint32_t time_steps);
/* smpc_get_moving_obstacle_costs of the object's context: m [batch_size], hit [batch_size] or NULL */
int sortham_optimizer_moving_obstacle_costs(sortham_optimizer* o, float* m, uint8_t* hit, uint32_t batch_size);
/* Optimizer::setTrajectoryValidation / clearTrajectoryValidation (params == NULL): with it on,
 * eval_control validates the trajectory of the control sequence each optimize() left
 * (smpc.h: smpc_validate_trajectory) and treats a colliding one as a tick whose rollouts all collide:
 * reset, retry, and past retry_attempt_limit SORTHAM_ERR_THROWN with the reference's message.  Off by
 * default.  Before or after initialize; kept across reset and across a re-initialize.  A lookahead
 * that is not > 0 and finite: SORTHAM_ERR_THROWN, the setting stays what it was. */
int sortham_optimizer_set_trajectory_validation(sortham_optimizer* o, const smpc_validation_params* params);
/* The verdict of the object's last validation (valid with nothing checked before the first one), how
 * many it has run and how many of them came back invalid.  Any of the three may be NULL. */
int sortham_optimizer_last_validation(const sortham_optimizer* o, smpc_validation* out, uint64_t* run,
                                      uint64_t* invalid);
int sortham_optimizer_reset(sortham_optimizer* o);
/* control_sequence_ as {vx[T], vy[T], wz[T]} */
int sortham_optimizer_get_control_sequence(sortham_optimizer* o, float* u);
int sortham_optimizer_set_control_sequence(sortham_optimizer* o, const float* u);
/* settings_.constraints = {vx_max, vx_min, vy, wz}; shift flag */
int sortham_optimizer_get_constraints(sortham_optimizer* o, float* c4, int32_t* shift_control_sequence);
/* getOptimizedTrajectory: xyyaw = T x 3 */
int sortham_optimizer_get_optimized_trajectory(sortham_optimizer* o, float* xyyaw);

/* utils::savitskyGolayFilter [ref tools/utils.hpp:442-605] on u = {vx[T], vy[T], wz[T]};
 * history = 4 x {vx, vy, wz}, oldest first.  No GPU involved. */
void sortham_utils_savitsky_golay(float* u, uint32_t T, float* history, int shift_control_sequence);

/* n consecutive closed-loop ticks from a compiled caller: smpc_optimize (or smpc_shard_tick with
 * SORTHAM_TICKS_SHARD*) on the same inputs, the control sequence u [3][time_steps] updated in
 * place and, with SORTHAM_TICKS_SHIFT, shifted one step between ticks as Optimizer::evalControl
 * does [ref src/optimizer.cpp:134-164, 206-225; the caller is src/controller.cpp:80-116].
 * outs: n entries; *done (may be null) = ticks completed; returns the first SMPC_ERR_* met. */
#define SORTHAM_TICKS_SHIFT 0x1u           /* shiftControlSequence after every tick            */
#define SORTHAM_TICKS_REDRAW_ASYNC 0x2u    /* smpc_redraw_noise_async after every tick         */
#define SORTHAM_TICKS_SHARD 0x4u           /* smpc_shard_tick(..., speculate = 0)              */
#define SORTHAM_TICKS_SHARD_SPECULATE 0x8u /* smpc_shard_tick(..., speculate = 1)              */
int sortham_run_ticks(smpc_ctx* ctx, const smpc_tick_in* in, float* u, uint32_t time_steps, uint32_t n,
                      uint32_t flags, smpc_tick_out* outs, uint32_t* done);

/* ---- Optimizer::evalControl for N robots through one grouped tick (host/fleet.hpp) ----
 * A fleet over n existing optimizers: the caller keeps them, goes on using them through their own
 * handles between rounds (set_costmap, set_speed_limit, reset, set_noise, set_control_sequence,
 * initialize again) and may destroy them and the fleet in any order.  One round ticks the members
 * taken with ONE smpc_group_optimize_some call and then runs, per member, what
 * sortham_optimizer_eval_control runs around its own tick: fallback / reset / retry (alone, the
 * fail flag sticky) / throw, Savitzky-Golay filter, Twist, shift [ref src/optimizer.cpp:134-225].
 * Every member computes what it computes alone, bit for bit.  Single-threaded.
 * create: SMPC_ERR_INVALID for a null argument, n = 0, a null member or one listed twice;
 * SMPC_ERR_STATE for a member without a context or in a fleet already; smpc_group_create's code
 * for members on different devices or with different time_steps.  The text of a failed create is
 * sortham_fleet_last_error(NULL). */
#define SORTHAM_FLEET_NOT_TAKEN 1 /* status of a member the round left out: nothing of its changed */
typedef struct sortham_fleet sortham_fleet;
int sortham_fleet_create(sortham_optimizer* const* members, uint32_t n, sortham_fleet** out);
void sortham_fleet_destroy(sortham_fleet* fleet);
const char* sortham_fleet_last_error(const sortham_fleet* fleet);
/* One round.  ins[n] as for sortham_optimizer_eval_control; take[n], one byte per member, NULL =
 * everybody (a member with take[i] == 0: ins[i] is not read, twists / outs entries not written,
 * status SORTHAM_FLEET_NOT_TAKEN); twists: n x 3 doubles; outs[n] (may be NULL); status[n]:
 * SMPC_OK, SORTHAM_FLEET_NOT_TAKEN, or SORTHAM_ERR_THROWN where that member's evalControl would
 * have thrown — the text is then in that member's sortham_optimizer_last_error, the member is as
 * evalControl leaves it when it throws, and the other members are not affected.
 * Returns SMPC_OK, or the SMPC_ERR_* of a round that failed as a whole (sortham_fleet_last_error):
 * then no member's control sequence, filter history or retry counter moved and the next round is
 * safe to run.  Taking a member that was shut down or destroyed is SMPC_ERR_STATE. */
int sortham_fleet_eval_control(sortham_fleet* fleet, const smpc_tick_in* ins, const uint8_t* take,
                               double* twists, smpc_tick_out* outs, int32_t* status);
/* smpc_group_stats summed over the groups the fleet has had (it regroups when a member rebuilds its
 * context), and the retries the fleet ran alone.  Any pointer may be NULL. */
int sortham_fleet_stats(const sortham_fleet* fleet, uint64_t* batched_launches, uint64_t* single_ticks,
                        uint64_t* retries);
/* FleetOptimizer::setMutualAvoidance: before a round's ticks every member taken gets one moving
 * obstacle per other member — a member taken this round as the trajectory of its control sequence
 * from this round's pose, one not taken as a disc standing at its last pose, one never taken left
 * out — with radius robot_radius[i] + robot_radius[j].  robot_radius[n], n the fleet's size;
 * n == 0: off (the default), every member's table cleared.  The tables of a round go to the
 * library in ONE smpc_group_set_moving_obstacles call (one upload for the fleet) and the members
 * taken ride the group's moving-obstacle launch; SMPC_FLEET_AVOID=per_member in the environment
 * when the fleet is created keeps one smpc_set_moving_obstacles per member — the same results. */
int sortham_fleet_set_mutual_avoidance(sortham_fleet* fleet, const smpc_moving_obstacles_params* params,
                                       const float* robot_radius, uint32_t n);
/* smpc_debug_group_moving_launches summed over the groups the fleet has had: launches of the grouped
 * moving-obstacle kernels and uploads of a group's table buffer.  Either pointer may be NULL. */
int sortham_fleet_moving_launches(const sortham_fleet* fleet, uint64_t* grouped_launches, uint64_t* table_uploads);
/* Trajectory validation in a fleet: a member has it on through its own handle
 * (sortham_optimizer_set_trajectory_validation).  Behind a round's grouped tick ONE
 * smpc_group_validate_trajectories call covers the members taken that have it on and did not fail; an
 * invalid member takes its own retry path (reset, a tick and a validation alone), the others are
 * untouched.  smpc_group_validation_counts summed over the groups the fleet has had: the grouped
 * validation calls (one per round, and one per retry of a member alone) and the members they carried.
 * Either pointer may be NULL. */
int sortham_fleet_validation_counts(const sortham_fleet* fleet, uint64_t* launches, uint64_t* members);
/* The table that rule gives member i of n (pure host code, no fleet needed): state[n] 0 never seen,
 * 1 standing, 2 moving; pose[n][3] x, y, yaw; u[n][3][time_steps]; model_dt[n]; holonomic[n];
 * robot_radius[n].  Out: xy [discs][time_steps][2] and radius [discs] (room for n - 1 discs), *discs. */
int sortham_fleet_avoidance_table(uint32_t i, uint32_t n, uint32_t time_steps, const uint8_t* state,
                                  const double* pose, const float* u, const float* model_dt,
                                  const uint8_t* holonomic, const float* robot_radius, float* xy,
                                  float* radius, uint32_t* discs);
/* FleetOptimizer::getCriticStats: sortham_optimizer_critic_stats for the members taken, the fleet
 * staying grouped (smpc.h: smpc_group_critic_breakdown).  ins[n], take[n] as for
 * sortham_fleet_eval_control; stats[n]; per_rollout: NULL, or n pointers of which any may be NULL,
 * else [SMPC_STATS_ROWS][batch_size] floats of that member; status[n]: SMPC_OK,
 * SORTHAM_FLEET_NOT_TAKEN (the member's entries are not written), or the SMPC_ERR_* that member's
 * sortham_optimizer_critic_stats would have returned — SMPC_ERR_STATE for a member that was shut
 * down or destroyed — with the text in that member's sortham_optimizer_last_error.  Changes
 * nothing: the next round returns what it would have returned without the call.  Returns SMPC_OK,
 * or the SMPC_ERR_* of a call that failed as a whole (sortham_fleet_last_error). */
int sortham_fleet_critic_stats(sortham_fleet* fleet, const smpc_tick_in* ins, const uint8_t* take,
                               smpc_critic_stats* stats, float* const* per_rollout, int32_t* status);
/* n_rounds rounds on the same inputs from a compiled caller (host/tick_loop.cpp), the results of
 * the last one in twists / outs / status (any may be NULL).  alone != 0: instead of the fleet round,
 * the members' own sortham_optimizer_eval_control one after the other on their ungrouped contexts
 * (the fleet regroups at its next round) — what a caller without the fleet runs, for timing the
 * two against each other.  *done (may be NULL) = rounds completed; returns the first SMPC_ERR_* of
 * a round as a whole. */
int sortham_fleet_run_rounds(sortham_fleet* fleet, const smpc_tick_in* ins, const uint8_t* take,
                             uint32_t n_rounds, int alone, double* twists, smpc_tick_out* outs,
                             int32_t* status, uint32_t* done);

/* ---- PathHandler for plain types [ref src/path_handler.cpp:25-220, tools/path_handler.hpp:46-165]
 * Poses are {x, y, yaw} triples of doubles.  What tf2 supplies in the reference comes in as
 * arguments: the robot pose already in the plan's frame and the rigid transform
 * {tx, ty, yaw} from the plan's frame to the costmap's (NULL = identity). */
typedef struct sortham_path_handler sortham_path_handler;
typedef struct sortham_path_handler_config {
  uint32_t costmap_size_x, costmap_size_y;          /* Costmap2D::getSizeInCellsX / Y                  */
  double costmap_resolution, costmap_origin_x, costmap_origin_y;
  double max_robot_pose_search_dist;                /* < 0: getMaxCostmapDist() [ref :39,166-171]       */
  double prune_distance;                            /* [ref :40] default 1.5                            */
  int32_t enforce_path_inversion;                   /* [ref :42]                                        */
  float inversion_xy_tolerance, inversion_yaw_tolerance; /* [ref :44-45]                                */
} sortham_path_handler_config;
void sortham_path_handler_config_default(sortham_path_handler_config* c);
int sortham_path_handler_create(const sortham_path_handler_config* cfg, sortham_path_handler** out);
void sortham_path_handler_destroy(sortham_path_handler* h);
const char* sortham_path_handler_last_error(const sortham_path_handler* h);
/* setPath [ref :173-180]: poses = n x {x, y, yaw} */
int sortham_path_handler_set_path(sortham_path_handler* h, const double* poses, uint32_t n);
/* getPath [ref :182] / the plan up to the first inversion: copies at most cap poses, returns the count */
uint32_t sortham_path_handler_get_path(const sortham_path_handler* h, int up_to_inversion, double* poses, uint32_t cap);
/* transformPath [ref :123-145]; SORTHAM_ERR_THROWN where the reference throws */
int sortham_path_handler_transform_path(sortham_path_handler* h, const double* robot_pose_in_plan_frame,
                                        const double* plan_to_costmap, double* poses_out, uint32_t cap,
                                        uint32_t* n_out);
/* getGlobalPlanConsideringBoundsInCostmapFrame [ref :48-103] without pruning; *closest = index of the
 * plan pose closest to the robot */
int sortham_path_handler_plan_in_bounds(sortham_path_handler* h, const double* robot_pose_in_plan_frame,
                                        const double* plan_to_costmap, double* poses_out, uint32_t cap,
                                        uint32_t* n_out, uint32_t* closest);
int sortham_path_handler_prune(sortham_path_handler* h, int up_to_inversion, uint32_t end);   /* prunePlan [ref :184-187] */
int sortham_path_handler_transformed_goal(sortham_path_handler* h, const double* plan_to_costmap, double* pose_out);
int sortham_path_handler_within_inversion_tolerances(const sortham_path_handler* h, const double* robot_pose);
double sortham_path_handler_max_costmap_dist(const sortham_path_handler* h);
/* utils::findFirstPathInversion / removePosesAfterFirstInversion [ref tools/utils.hpp:612-658];
 * the second edits poses in place and writes the new count to *n */
uint32_t sortham_utils_find_first_path_inversion(const double* poses, uint32_t n);
uint32_t sortham_utils_remove_poses_after_first_inversion(double* poses, uint32_t* n);

/* ---- TrajectoryVisualizer's marker lists [ref src/trajectory_visualizer.cpp:59-128] ----
 * A marker comes back as 10 doubles {id, x, y, z, scale x, y, z, g, b, a} (r is always 0). */
typedef struct sortham_trajectory_visualizer sortham_trajectory_visualizer;
int sortham_visualizer_create(const char* frame_id, int trajectory_step, int time_step,
                              sortham_trajectory_visualizer** out);
void sortham_visualizer_destroy(sortham_trajectory_visualizer* v);
/* add(optimal trajectory): n rows of `stride` floats, x and y first [ref :59-83] */
int sortham_visualizer_add_trajectory(sortham_trajectory_visualizer* v, const float* xy, uint32_t n, uint32_t stride);
/* add(candidate trajectories): x, y [B][T] [ref :85-107] */
int sortham_visualizer_add_candidates(sortham_trajectory_visualizer* v, const float* x, const float* y,
                                      uint32_t B, uint32_t T);
/* visualize() [ref :115-126]: what would be published; copies at most cap markers, returns the count, resets */
uint32_t sortham_visualizer_visualize(sortham_trajectory_visualizer* v, double* markers, uint32_t cap);
const char* sortham_visualizer_frame(const sortham_trajectory_visualizer* v);

#ifdef __cplusplus
}
#endif
#endif
