// optimizer.hpp — host side of the sampling-MPC controller above the C-ABI.
//
// Mirrors sortham::Optimizer of the reference (nav2_sortham_controller
// include/nav2_sortham_controller/optimizer.hpp:51-263, src/optimizer.cpp) with
// the same method names, argument meaning and error behaviour, minus the ROS
// types: poses arrive as (x, y, yaw) — tf2::getYaw is applied by the caller —
// and the costmap as a plain view.  Everything over [batch, time] happens in
// libsmpc.so (include/smpc.h); this class keeps what the reference keeps on the
// host: prepare / fallback / Savitzky-Golay filter / Twist extraction /
// sequence shift / speed limit / reset.
#ifndef SORTHAM_HOST_OPTIMIZER_HPP_
#define SORTHAM_HOST_OPTIMIZER_HPP_

#include <array>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/smpc.h"

// The class is sortham::Optimizer, like the reference's.  Inside the Nav2 package the
// ROS-typed adaptor of the same name wraps it (nav2_plugin/), which then builds this file
// with -DSORTHAM_HOST_NS=sortham_host.
#ifndef SORTHAM_HOST_NS
#define SORTHAM_HOST_NS sortham
#endif

namespace SORTHAM_HOST_NS
{

namespace models
{
// ref models/control_sequence.hpp:27-49
struct Control
{
  float vx, vy, wz;
};

struct ControlSequence
{
  std::vector<float> vx, vy, wz;
  void reset(unsigned int time_steps)
  {
    vx.assign(time_steps, 0.0f);
    vy.assign(time_steps, 0.0f);
    wz.assign(time_steps, 0.0f);
  }
};

// ref models/constraints.hpp:25-42
struct ControlConstraints
{
  float vx_max, vx_min, vy, wz;
};
struct SamplingStd
{
  float vx, vy, wz;
};

// ref models/optimizer_settings.hpp:28-41
struct OptimizerSettings
{
  ControlConstraints base_constraints{0, 0, 0, 0};
  ControlConstraints constraints{0, 0, 0, 0};
  SamplingStd sampling_std{0, 0, 0};
  float model_dt{0};
  float temperature{0};
  float gamma{0};
  unsigned int batch_size{0};
  unsigned int time_steps{0};
  unsigned int iteration_count{0};
  bool shift_control_sequence{false};
  size_t retry_attempt_limit{0};
};

// ref models/path.hpp:27-44 (utils::toTensor output)
struct Path
{
  std::vector<float> x, y, yaws;
};
}  // namespace models

struct Pose2D
{
  double x{0}, y{0};
  double yaw{0};  // tf2::getYaw(orientation)
};
struct Twist2D
{
  double vx{0}, vy{0}, wz{0};
};

// what the critics read from nav2_costmap_2d::Costmap2DROS
struct CostmapView
{
  const uint8_t * cells{nullptr};
  unsigned int size_x{0}, size_y{0};
  double origin_x{0}, origin_y{0}, resolution{0};
  bool track_unknown{false};
  float inscribed_radius{0};
  bool has_inflation_layer{false};
  // consider_footprint = true: costmap_ros->getRobotFootprint() as (x, y) pairs, the layered
  // costmap's circumscribed radius, the inflation layer's own cost_scaling_factor
  std::vector<double> footprint_xy;
  double circumscribed_radius{0};
  double layer_cost_scaling_factor{-1.0};
};

struct CriticsConfig
{
  std::vector<std::string> critics;  // YAML `critics` list, in order (critic_manager.cpp:36-41)
  smpc_critic_params params{};       // per-critic parameters (enabled is derived from `critics`)
  float cost_scaling_factor{10.0f};  // ObstaclesCritic params read with an InflationLayer
  float inflation_radius{0.55f};     // (obstacles_critic.cpp:76-80)
};

namespace utils
{
// ref tools/utils.hpp:442-605
void savitskyGolayFilter(
  models::ControlSequence & control_sequence, std::array<models::Control, 4> & control_history,
  const models::OptimizerSettings & settings);
}  // namespace utils

class Optimizer;

// integrateStateVelocities(trajectory, sequence) (ref optimizer.cpp:275-311) as a free function: the
// [T][3] x, y, yaw of a control sequence integrated from a pose, no measured-speed first column.  What
// Optimizer::getOptimizedTrajectory returns, and what a fleet predicts a member's motion with.
std::vector<std::array<float, 3>> integrateControlSequence(
  const models::ControlSequence & sequence, unsigned int time_steps, float model_dt,
  const Pose2D & pose, bool holonomic);

// the arguments of Optimizer::evalControl as one value (getCriticStats)
struct TickInput
{
  Pose2D robot_pose;
  Twist2D robot_speed;
  models::Path plan;
  Pose2D goal;
  float goal_checker_xy_tolerance{-1.0f};
};

// What passes between these values and the blocks of the C ABI, once each: the control sequence as
// u [3][T] (vx, vy, wz), a tick's arguments as a smpc_tick_in and back, the moving obstacles' value rule.
inline void packControls(const models::ControlSequence & s, size_t T, float * u)
{
  std::memcpy(u, s.vx.data(), T * sizeof(float));
  std::memcpy(u + T, s.vy.data(), T * sizeof(float));
  std::memcpy(u + 2 * T, s.wz.data(), T * sizeof(float));
}

// (a sequence that holds T steps already keeps its memory)
inline void unpackControls(const float * u, size_t T, models::ControlSequence & s)
{
  s.vx.assign(u, u + T);
  s.vy.assign(u + T, u + 2 * T);
  s.wz.assign(u + 2 * T, u + 3 * T);
}

// The smpc_tick_in of evalControl's arguments; the plan is pointed at, not copied.  fail_flag_in: sticky
// across a retry (critic_manager.cpp:70-73).
inline smpc_tick_in tickIn(
  const Pose2D & pose, const Twist2D & speed, const models::Path & plan, const Pose2D & goal,
  float goal_checker_xy_tolerance, bool fail_flag_in)
{
  smpc_tick_in in;
  std::memset(&in, 0, sizeof(in));   // (path_pts_valid stays null)
  in.pose_x = pose.x;
  in.pose_y = pose.y;
  in.pose_yaw = static_cast<float>(pose.yaw);   // float initial_yaw = tf2::getYaw(...)
  in.speed_vx = speed.vx;
  in.speed_vy = speed.vy;
  in.speed_wz = speed.wz;
  in.path_x = plan.x.data();
  in.path_y = plan.y.data();
  in.path_yaw = plan.yaws.data();
  in.path_len = static_cast<uint32_t>(plan.x.size());
  in.goal_x = goal.x;
  in.goal_y = goal.y;
  in.fail_flag_in = fail_flag_in ? 1 : 0;
  in.goal_checker_xy_tolerance = goal_checker_xy_tolerance;
  return in;
}

// The inverse, for the C faces: a smpc_tick_in taken apart into evalControl's arguments, in place (a
// plan that is assigned again keeps its capacity).  The goal's yaw is not in the block: 0.
inline void tickInputFrom(
  const smpc_tick_in & in, Pose2D & pose, Twist2D & speed, models::Path & plan, Pose2D & goal,
  float & goal_checker_xy_tolerance)
{
  pose = {in.pose_x, in.pose_y, static_cast<double>(in.pose_yaw)};
  goal = {in.goal_x, in.goal_y, 0.0};
  speed = {in.speed_vx, in.speed_vy, in.speed_wz};
  plan.x.assign(in.path_x, in.path_x + in.path_len);
  plan.y.assign(in.path_y, in.path_y + in.path_len);
  plan.yaws.assign(in.path_yaw, in.path_yaw + in.path_len);
  goal_checker_xy_tolerance = in.goal_checker_xy_tolerance;
}

inline TickInput tickInputFrom(const smpc_tick_in & in)
{
  TickInput ti;
  tickInputFrom(in, ti.robot_pose, ti.robot_speed, ti.plan, ti.goal, ti.goal_checker_xy_tolerance);
  return ti;
}

// smpc_set_moving_obstacles' rule for the parameters and the radii, for a table refused before a context sees it
inline bool movingObstacleValuesOk(const smpc_moving_obstacles_params & p, const std::vector<float> & radius)
{
  bool ok = std::isfinite(p.collision_cost) && std::isfinite(p.repulsion_weight) && std::isfinite(p.margin) &&
    p.collision_cost >= 0.0f && p.repulsion_weight >= 0.0f && p.margin > 0.0f;
  for (float r : radius) {
    ok = ok && std::isfinite(r) && r > 0.0f;
  }
  return ok;
}

// What an Optimizer asks of the fleet it is a member of (fleet.hpp: FleetOptimizer, N optimizers
// ticked through one smpc_group).  An interface, so that this class links without the fleet.
class FleetLink
{
public:
  virtual ~FleetLink() = default;
  // a member's context is about to be destroyed: the group goes first (smpc.h)
  virtual void dropGroup() = 0;
  virtual void memberDestroyed(Optimizer * member) = 0;
  // is this member's context in the fleet's group right now?
  virtual bool grouped(const Optimizer * member) const = 0;
  // one tick of this member alone through the group (smpc_optimize on its slot); throws on error
  virtual void tickAlone(Optimizer * member, const smpc_tick_in & in, float * u, smpc_tick_out & out) = 0;
  // one trajectory validation of this member alone through the group (smpc_group_validate_trajectories
  // with this member taken); throws on error
  virtual void validateAlone(
    Optimizer * member, const smpc_validation_params & params, const double * pose, const float * u,
    smpc_validation & out) = 0;
};

class FleetOptimizer;

class Optimizer
{
public:
  Optimizer() = default;
  ~Optimizer();
  Optimizer(const Optimizer &) = delete;
  Optimizer & operator=(const Optimizer &) = delete;

  // ref optimizer.cpp:35-55 + getParams :62-93 (parameters arrive resolved)
  void initialize(
    const models::OptimizerSettings & settings, const std::string & motion_model,
    double controller_frequency, const CriticsConfig & critics, bool regenerate_noises = false,
    uint64_t noise_seed = 0, int device = -1);
  void shutdown();  // ref :57-60

  // the caller holds the costmap mutex for the tick (controller.cpp:99-100)
  void setCostmap(const CostmapView & costmap);
  // parity runs: supply NoiseGenerator's tensors instead of drawing them
  void setNoise(const float * nvx, const float * nvy, const float * nwz);

  // ref :134-155; throws std::runtime_error exactly where the reference does
  // goal_checker_xy_tolerance: GoalChecker::getTolerances()'s pose_tolerance.position.x, < 0
  // when the controller server passes no goal checker (TwirlingCritic's gate)
  Twist2D evalControl(
    const Pose2D & robot_pose, const Twist2D & robot_speed, const models::Path & plan,
    const Pose2D & goal, float goal_checker_xy_tolerance = -1.0f);

  // Per-critic costs and effective samples (smpc_critic_breakdown) of the tick evalControl(in)
  // would run next: its first scoring pass, from the control sequence as it stands.  Changes
  // nothing: evalControl afterwards returns what it would have returned without the call.
  // per_rollout: null, or [SMPC_STATS_ROWS][batch_size] floats.  Throws for a fleet member whose
  // context is grouped (SMPC_ERR_STATE).
  smpc_critic_stats getCriticStats(const TickInput & in, float * per_rollout = nullptr);

  void setSpeedLimit(double speed_limit, bool percentage);  // ref :428-453
  // Acceleration limits on the sampled controls (smpc_set_acceleration_limits: ax_max > 0, ax_min < 0,
  // ay_max > 0, az_max > 0; all zero: off, the default).  Before or after initialize(); kept across
  // reset() and across whatever recreates the context.  Throws where the library refuses the values.
  void setAccelerationLimits(float ax_max, float ax_min, float ay_max, float az_max);
  // Moving obstacles (smpc_set_moving_obstacles): xy [n][T][2] disc centres per trajectory point in the
  // costmap's world frame, radius [n] centre-to-centre collision distances.  Before or after
  // initialize(); kept across reset() and across whatever recreates the context, as the limits are.
  // Throws where the library refuses the values (the table then stays what it was).
  void setMovingObstacles(
    const smpc_moving_obstacles_params & params, const std::vector<float> & xy,
    const std::vector<float> & radius);
  void clearMovingObstacles();
  // m [B] and hit [B] of the last tick's last iteration (smpc_get_moving_obstacle_costs)
  void getMovingObstacleCosts(std::vector<float> & m, std::vector<uint8_t> & hit);
  // Trajectory validation (smpc_validate_trajectory; upstream Nav2's optimal-trajectory validator):
  // with it on, evalControl checks the trajectory of the control sequence each optimize() left —
  // the costmap under its first collision_lookahead_time / model_dt poses, with the footprint if
  // asked, and the moving obstacles — and a colliding one takes the path of a tick whose rollouts
  // all collide: reset, retry, and past retry_attempt_limit the reference's exception.  Off by
  // default.  Before or after initialize(); kept across reset() and across whatever recreates the
  // context.  Throws for a lookahead that is not > 0 and finite.
  void setTrajectoryValidation(const smpc_validation_params & params);
  void clearTrajectoryValidation() {validate_on_ = false;}
  bool trajectoryValidation() const {return validate_on_;}
  // the verdict of the last validation (valid, nothing checked, before the first one)
  const smpc_validation & lastValidation() const {return last_validation_;}
  // validations run so far, and those that came back invalid
  uint64_t validationsRun() const {return validations_run_;}
  uint64_t validationsFailed() const {return validations_failed_;}
  void reset();                                             // ref :116-132

  // ref :345-360: [T][3] x, y, yaw of the optimal sequence
  std::vector<std::array<float, 3>> getOptimizedTrajectory();
  // ref :455-458 (needs visualize = true at initialize)
  void getGeneratedTrajectories(std::vector<float> & x, std::vector<float> & y, std::vector<float> & yaws);

  models::ControlSequence & controlSequence() {return control_sequence_;}
  const models::OptimizerSettings & settings() const {return settings_;}
  const smpc_tick_out & lastTick() const {return last_out_;}
  void setVisualize(bool v) {visualize_ = v;}
  // SMPC_FLAG_LANE_PER_ROLLOUT for the context initialize() creates (smpc.h); call before it
  void setLanePerRollout(bool v) {lane_per_rollout_ = v;}
  bool isHolonomic() const {return motion_model_ == SMPC_MODEL_OMNI;}   // ref :235
  // AckermannConstraints.min_turning_r (motion_models.hpp:91-95); call before initialize()
  void setAckermannMinTurningRadius(float r) {ackermann_min_turning_r_ = r;}

  bool initialized() const {return ctx_ != nullptr;}

protected:
  friend class FleetOptimizer;   // fleet.hpp
  void optimize();                         // ref :157-164 -> smpc_optimize
  // the three pieces of a tick around the scoring call, shared with FleetOptimizer:
  // the member's smpc_tick_in and u [3][T] from its state, constraints pushed
  void fillTick(smpc_tick_in & in, float * u);
  // a tick's result: u copied back, fail_flag_, last_out_, the regenerate_noises redraw
  void takeTick(const float * u, const smpc_tick_out & out);
  // ref :147-154: Savitzky-Golay filter, Twist, shift
  Twist2D finishTick();
  void destroyContext(smpc_ctx * ctx);     // tells the fleet first: its group goes before the context
  void configureContext();                 // initialize()'s tail, for a context kept and a new one alike
  bool fallback(bool fail);                // ref :166-183 (retry counter per object)
  // true unless validation is on, the tick did not fail, and the control sequence's trajectory collides
  bool validated();
  void takeValidation(const smpc_validation & v);
  void prepare(const Pose2D &, const Twist2D &, const models::Path &, const Pose2D &);  // ref :185-204
  void shiftControlSequence();             // ref :206-225
  Twist2D getControlFromSequenceAsTwist(); // ref :396-410
  void setOffset(double controller_frequency);  // ref :95-114
  void setMotionModel(const std::string & model);  // ref :412-426
  void pushConstraints();
  void pushAccelerationLimits();
  void pushMovingObstacles();

  models::OptimizerSettings settings_{};
  models::ControlSequence control_sequence_{};
  std::array<models::Control, 4> control_history_{};
  CriticsConfig critics_{};
  bool regenerate_noises_{false};
  uint32_t motion_model_{SMPC_MODEL_OMNI};
  float ackermann_min_turning_r_{0.2f};
  bool visualize_{false};
  bool lane_per_rollout_{false};
  std::array<float, 4> accel_limits_{{0.0f, 0.0f, 0.0f, 0.0f}};   // ax_max, ax_min, ay_max, az_max; all zero: off
  smpc_moving_obstacles_params moving_params_{};
  std::vector<float> moving_xy_, moving_radius_;   // empty: off
  bool validate_on_{false};
  smpc_validation_params validation_params_{};
  smpc_validation last_validation_{1, 0, 0, 0, 0, 0.0f};
  uint64_t validations_run_{0}, validations_failed_{0};
  uint64_t noise_seed_{0};
  bool supplied_noise_{false};
  int device_{-1};
  smpc_ctx * ctx_{nullptr};
  smpc_config built_cfg_{};     // what ctx_ was created with (initialize() keeps it for an identical one)
  uint64_t built_seed_{0};
  bool have_built_{false};

  // per-tick (CriticData)
  Pose2D pose_{}, goal_{};
  Twist2D speed_{};
  models::Path path_{};
  bool fail_flag_{false};
  float goal_checker_xy_tolerance_{-1.0f};
  size_t retry_counter_{0};
  smpc_tick_out last_out_{};
  FleetLink * fleet_{nullptr};   // set while the object is a fleet's member
};

}  // namespace SORTHAM_HOST_NS

#endif
