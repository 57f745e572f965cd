// optimizer.cpp — see optimizer.hpp.  Host orchestration of one
// computeVelocityCommands() tick over the libsmpc C-ABI.
#include "optimizer.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <stdexcept>
#include <utility>

namespace SORTHAM_HOST_NS
{

namespace
{
void ck(smpc_ctx * ctx, int rc, const char * what)
{
  if (rc != SMPC_OK) {
    throw std::runtime_error(std::string(what) + ": " + smpc_last_error(ctx));
  }
}
}  // namespace

Optimizer::~Optimizer()
{
  shutdown();
  if (fleet_) {
    fleet_->memberDestroyed(this);
  }
}

void Optimizer::shutdown()
{
  if (ctx_) {
    destroyContext(ctx_);
    ctx_ = nullptr;
  }
}

void Optimizer::destroyContext(smpc_ctx * ctx)
{
  // smpc.h: a group is destroyed before its members.  The fleet drops its group here and forms
  // a new one, over the contexts its members have by then, before its next round.
  if (fleet_) {
    fleet_->dropGroup();
  }
  smpc_destroy(ctx);
}

void Optimizer::setMotionModel(const std::string & model)
{
  // DiffDrive, Omni and Ackermann (optimizer.cpp:412-426).  Omni is the model the north star
  // names; the two non-holonomic ones run the same kernels with vy held at zero (smpc.h).
  const std::pair<const char *, uint32_t> known[] = {
    {"Omni", SMPC_MODEL_OMNI}, {"DiffDrive", SMPC_MODEL_DIFF_DRIVE}, {"Ackermann", SMPC_MODEL_ACKERMANN}};
  for (const auto & k : known) {
    if (model == k.first) {
      motion_model_ = k.second;
      return;
    }
  }
  throw std::runtime_error(
          std::string(
            "Model " + model + " is not valid! Valid options are DiffDrive, Omni, "
            "or Ackermann"));
}

void Optimizer::setOffset(double controller_frequency)
{
  const double controller_period = 1.0 / controller_frequency;
  constexpr double eps = 1e-6;
  if ((controller_period + eps) < settings_.model_dt) {
    // reference warns: "Controller period is less then model dt, consider setting it equal"
  } else if (std::abs(controller_period - settings_.model_dt) < eps) {
    settings_.shift_control_sequence = true;
  } else {
    throw std::runtime_error("Controller period more then model dt, set it equal to model dt");
  }
}

void Optimizer::initialize(
  const models::OptimizerSettings & settings, const std::string & motion_model,
  double controller_frequency, const CriticsConfig & critics, bool regenerate_noises,
  uint64_t noise_seed, int device)
{
  // A call with the configuration the device context was built for (the controller's reset()
  // after every idle period, src/controller.cpp:89-92, re-reads unchanged parameters) keeps the
  // context: decided below, once the new smpc_config is known.
  smpc_ctx * keep = ctx_;
  ctx_ = nullptr;
  struct Guard
  {
    Optimizer * self;
    smpc_ctx *& k;
    ~Guard() {if (k) {self->destroyContext(k);}}   // a throwing initialize() leaves no context behind, as before
  } guard{this, keep};
  settings_ = settings;
  settings_.constraints = settings_.base_constraints;
  setMotionModel(motion_model);
  setOffset(controller_frequency);
  critics_ = critics;
  regenerate_noises_ = regenerate_noises;
  noise_seed_ = noise_seed;
  device_ = device;

  // CriticManager::loadCritics (critic_manager.cpp:42-60): the YAML list decides which
  // critics exist; the ones outside the fused set cannot be scored here
  auto & p = critics_.params;
  const struct {const char * name; int32_t * enabled;} known[] = {
    {"ObstaclesCritic", &p.obstacles.enabled}, {"PathAlignCritic", &p.path_align.enabled},
    {"PathFollowCritic", &p.path_follow.enabled}, {"GoalAngleCritic", &p.goal_angle.enabled},
    {"PreferForwardCritic", &p.prefer_forward.enabled}, {"CostCritic", &p.cost.enabled},
    {"GoalCritic", &p.goal.enabled}, {"ConstraintCritic", &p.constraint.enabled},
    {"TwirlingCritic", &p.twirling.enabled}, {"PathAngleCritic", &p.path_angle.enabled},
    {"VelocityDeadbandCritic", &p.velocity_deadband.enabled}, {"PathAlignLegacyCritic", &p.path_align_legacy.enabled}};
  for (const auto & k : known) {
    *k.enabled = 0;
  }
  for (const auto & name : critics_.critics) {
    const auto k = std::find_if(std::begin(known), std::end(known), [&](const auto & e) {return name == e.name;});
    if (k == std::end(known)) {
      // (critics.xml registers twelve classes and all twelve are fused: what is left is a name
      // pluginlib would not find either, critic_manager.cpp:45-57)
      throw std::runtime_error(
              "Critic sortham::critics::" + name + " is not one of the registered critic classes (critics.xml)");
    }
    *k->enabled = 1;
  }

  smpc_config cfg;
  std::memset(&cfg, 0, sizeof(cfg));   // (compared byte for byte below: no stray padding)
  smpc_config_default(&cfg);
  cfg.batch_size = settings_.batch_size;
  cfg.time_steps = settings_.time_steps;
  cfg.iteration_count = settings_.iteration_count;
  cfg.motion_model = motion_model_;
  cfg.ackermann_min_turning_r = ackermann_min_turning_r_;
  cfg.model_dt = settings_.model_dt;
  cfg.temperature = settings_.temperature;
  cfg.gamma = settings_.gamma;
  cfg.vx_max = settings_.base_constraints.vx_max;
  cfg.vx_min = settings_.base_constraints.vx_min;
  cfg.vy_max = settings_.base_constraints.vy;
  cfg.wz_max = settings_.base_constraints.wz;
  cfg.vx_std = settings_.sampling_std.vx;
  cfg.vy_std = settings_.sampling_std.vy;
  cfg.wz_std = settings_.sampling_std.wz;
  cfg.device = device_;
  cfg.flags = (visualize_ ? SMPC_FLAG_STORE_TRAJECTORIES : 0u) | (lane_per_rollout_ ? SMPC_FLAG_LANE_PER_ROLLOUT : 0u);
  if (keep && have_built_ && std::memcmp(&cfg, &built_cfg_, sizeof(cfg)) == 0 && noise_seed_ == built_seed_) {
    // same shapes, model, sampling and seed: only the critics' parameters can differ.  What the
    // reference's reset() does (src/optimizer.cpp:116-132) is the reset() that ends configureContext(),
    // noise re-draw included.
    ctx_ = keep;
    keep = nullptr;
  } else {
    if (keep) {
      destroyContext(keep);
      keep = nullptr;
    }
    have_built_ = false;
    supplied_noise_ = false;
    if (smpc_create(&cfg, &ctx_) != SMPC_OK) {
      throw std::runtime_error(std::string("smpc_create: ") + smpc_last_error(nullptr));
    }
    built_cfg_ = cfg;
    built_seed_ = noise_seed_;
    have_built_ = true;
  }
  configureContext();
}

// what a context kept and a context just created both get: the critics, the limits and the table the
// object remembers, the seed's first epoch, the reset
void Optimizer::configureContext()
{
  ck(ctx_, smpc_set_critics(ctx_, &critics_.params), "smpc_set_critics");
  pushAccelerationLimits();
  pushMovingObstacles();
  // as a fresh context: noise supplied through setNoise() does not survive initialize(), and the
  // draw starts from the seed's first epoch again (same seed, same noise as a new object) ...
  supplied_noise_ = false;
  // ... NoiseGenerator::initialize draws once (noise_generator.cpp:26-42) ...
  ck(ctx_, smpc_seed(ctx_, noise_seed_), "smpc_seed");
  // ... and Optimizer::initialize ends in reset(), which draws again (H7)
  reset();
}

void Optimizer::pushConstraints()
{
  const auto & c = settings_.constraints;
  ck(ctx_, smpc_set_constraints(ctx_, c.vx_max, c.vx_min, c.vy, c.wz), "smpc_set_constraints");
}

void Optimizer::pushAccelerationLimits()
{
  const auto & a = accel_limits_;
  ck(ctx_, smpc_set_acceleration_limits(ctx_, a[0], a[1], a[2], a[3]), "smpc_set_acceleration_limits");
}

void Optimizer::setAccelerationLimits(float ax_max, float ax_min, float ay_max, float az_max)
{
  const std::array<float, 4> before = accel_limits_;
  if (!ctx_) {
    // no context yet to refuse them: the library's rule (smpc_set_acceleration_limits), so that
    // initialize() never meets values it cannot hand on
    const bool off = ax_max == 0.0f && ax_min == 0.0f && ay_max == 0.0f && az_max == 0.0f;
    const bool finite = std::isfinite(ax_max) && std::isfinite(ax_min) && std::isfinite(ay_max) && std::isfinite(az_max);
    if (!off && !(finite && ax_max > 0.0f && ax_min < 0.0f && ay_max > 0.0f && az_max > 0.0f)) {
      throw std::runtime_error(
              "setAccelerationLimits: ax_max > 0, ax_min < 0, ay_max > 0, az_max > 0, all finite (all four 0: off)");
    }
    accel_limits_ = {{ax_max, ax_min, ay_max, az_max}};
    return;   // initialize() hands them to the context it creates
  }
  accel_limits_ = {{ax_max, ax_min, ay_max, az_max}};
  try {
    pushAccelerationLimits();
  } catch (...) {
    accel_limits_ = before;   // refused: the context keeps what it had
    throw;
  }
}

void Optimizer::pushMovingObstacles()
{
  const uint32_t n = static_cast<uint32_t>(moving_radius_.size());
  if (moving_xy_.size() != static_cast<size_t>(n) * settings_.time_steps * 2) {
    throw std::runtime_error("moving obstacles: xy must hold [n][time_steps][2] floats");
  }
  ck(
    ctx_, smpc_set_moving_obstacles(ctx_, &moving_params_, n ? moving_xy_.data() : nullptr,
    n ? moving_radius_.data() : nullptr, n), "smpc_set_moving_obstacles");
}

void Optimizer::setMovingObstacles(
  const smpc_moving_obstacles_params & params, const std::vector<float> & xy,
  const std::vector<float> & radius)
{
  // the library's rules, so that a table set before initialize() is one the context will take
  const size_t n = radius.size();
  if (n > SMPC_MAX_MOVING_OBSTACLES) {
    throw std::runtime_error("setMovingObstacles: more than SMPC_MAX_MOVING_OBSTACLES obstacles");
  }
  if (n == 0 ? !xy.empty() : xy.size() % (2 * n) != 0 || (ctx_ && xy.size() != n * settings_.time_steps * 2)) {
    throw std::runtime_error("setMovingObstacles: xy must hold [n][time_steps][2] floats");
  }
  bool ok = movingObstacleValuesOk(params, radius);
  for (float v : xy) {ok = ok && std::isfinite(v);}
  if (n && !ok) {
    throw std::runtime_error(
            "setMovingObstacles: collision_cost >= 0, repulsion_weight >= 0, margin > 0, radius > 0, all finite");
  }
  const smpc_moving_obstacles_params p_before = moving_params_;
  std::vector<float> xy_before = std::move(moving_xy_), r_before = std::move(moving_radius_);
  moving_params_ = params;
  moving_xy_ = xy;
  moving_radius_ = radius;
  if (!ctx_) {return;}   // initialize() hands them to the context it creates
  try {
    pushMovingObstacles();
  } catch (...) {
    moving_params_ = p_before;   // refused: the context keeps what it had
    moving_xy_ = std::move(xy_before);
    moving_radius_ = std::move(r_before);
    throw;
  }
}

void Optimizer::clearMovingObstacles()
{
  moving_xy_.clear();
  moving_radius_.clear();
  if (ctx_) {pushMovingObstacles();}
}

void Optimizer::getMovingObstacleCosts(std::vector<float> & m, std::vector<uint8_t> & hit)
{
  m.resize(settings_.batch_size);
  hit.resize(settings_.batch_size);
  ck(ctx_, smpc_get_moving_obstacle_costs(ctx_, m.data(), hit.data()), "smpc_get_moving_obstacle_costs");
}

void Optimizer::reset()
{
  control_sequence_.reset(settings_.time_steps);
  control_history_.fill({0.0f, 0.0f, 0.0f});
  settings_.constraints = settings_.base_constraints;
  if (ctx_) {
    ck(ctx_, smpc_reset(ctx_), "smpc_reset");   // costs, noise re-draw (noise_generator.cpp:76-95)
  }
}

void Optimizer::setCostmap(const CostmapView & m)
{
  const bool infl = m.has_inflation_layer;
  ck(
    ctx_, smpc_set_costmap(
      ctx_, m.cells, m.size_x, m.size_y, m.origin_x, m.origin_y, m.resolution,
      m.track_unknown ? 1 : 0, m.inscribed_radius, infl ? critics_.cost_scaling_factor : 0.0f,
      infl ? critics_.inflation_radius : 0.0f), "smpc_set_costmap");
  if (!m.footprint_xy.empty()) {
    ck(
      ctx_, smpc_set_footprint(
        ctx_, m.footprint_xy.data(), static_cast<uint32_t>(m.footprint_xy.size() / 2),
        m.circumscribed_radius, infl ? m.layer_cost_scaling_factor : -1.0), "smpc_set_footprint");
  }
}

void Optimizer::setNoise(const float * nvx, const float * nvy, const float * nwz)
{
  ck(ctx_, smpc_set_noise(ctx_, nvx, nvy, nwz), "smpc_set_noise");
  supplied_noise_ = true;
}

void Optimizer::prepare(
  const Pose2D & robot_pose, const Twist2D & robot_speed, const models::Path & plan,
  const Pose2D & goal)
{
  pose_ = robot_pose;
  speed_ = robot_speed;
  path_ = plan;
  goal_ = goal;
  fail_flag_ = false;   // costs_.fill(0) and the CriticData caches are per smpc_optimize call
}

void Optimizer::fillTick(smpc_tick_in & in, float * u)
{
  in = tickIn(pose_, speed_, path_, goal_, goal_checker_xy_tolerance_, fail_flag_);   // (the flag: sticky across the retry)
  packControls(control_sequence_, settings_.time_steps, u);
  pushConstraints();
}

void Optimizer::takeTick(const float * u, const smpc_tick_out & out)
{
  unpackControls(u, settings_.time_steps, control_sequence_);
  last_out_ = out;
  fail_flag_ = last_out_.fail_flag != 0;
  if (regenerate_noises_ && !supplied_noise_) {
    // NoiseGenerator::generateNextNoises (noise_generator.cpp:54-63): next tick's noise, drawn
    // while this tick's result travels on (the reference's noise thread, :97-105)
    ck(ctx_, smpc_redraw_noise_async(ctx_), "smpc_redraw_noise_async");
  }
}

void Optimizer::optimize()
{
  smpc_tick_in in;
  std::vector<float> u(3 * settings_.time_steps);
  fillTick(in, u.data());
  smpc_tick_out out;
  if (fleet_ && fleet_->grouped(this)) {
    // a grouped context is not ticked through smpc_optimize directly (smpc.h): the group ticks
    // this member alone — smpc_optimize on its slot of the group's buffers, the same result
    fleet_->tickAlone(this, in, u.data(), out);
  } else {
    ck(ctx_, smpc_optimize(ctx_, &in, u.data(), &out), "smpc_optimize");
  }
  takeTick(u.data(), out);
}

smpc_critic_stats Optimizer::getCriticStats(const TickInput & ti, float * per_rollout)
{
  // the smpc_tick_in evalControl's first optimize() would hand over (prepare() clears the fail
  // flag), without touching the per-tick members
  const smpc_tick_in in =
    tickIn(ti.robot_pose, ti.robot_speed, ti.plan, ti.goal, ti.goal_checker_xy_tolerance, false);
  std::vector<float> u(3 * settings_.time_steps);
  packControls(control_sequence_, settings_.time_steps, u.data());
  pushConstraints();   // (what the tick pushes too: the same values)
  smpc_critic_stats stats;
  ck(ctx_, smpc_critic_breakdown(ctx_, &in, u.data(), &stats, per_rollout), "smpc_critic_breakdown");
  return stats;
}

void Optimizer::setTrajectoryValidation(const smpc_validation_params & params)
{
  if (!std::isfinite(params.collision_lookahead_time) || !(params.collision_lookahead_time > 0.0f)) {
    throw std::runtime_error("setTrajectoryValidation: collision_lookahead_time must be > 0 and finite");
  }
  validation_params_ = params;
  validate_on_ = true;
}

void Optimizer::takeValidation(const smpc_validation & v)
{
  last_validation_ = v;
  validations_run_++;
  if (!v.valid) {
    validations_failed_++;
  }
}

bool Optimizer::validated()
{
  if (!validate_on_ || fail_flag_) {
    return true;   // (a failed tick takes the fallback path as it is)
  }
  std::vector<float> u(3 * settings_.time_steps);
  packControls(control_sequence_, settings_.time_steps, u.data());
  smpc_validation v{};
  if (fleet_ && fleet_->grouped(this)) {
    const double pose[3] = {pose_.x, pose_.y, pose_.yaw};
    fleet_->validateAlone(this, validation_params_, pose, u.data(), v);
  } else {
    ck(
      ctx_, smpc_validate_trajectory(
        ctx_, &validation_params_, pose_.x, pose_.y, static_cast<float>(pose_.yaw), u.data(), &v, nullptr),
      "smpc_validate_trajectory");
  }
  takeValidation(v);
  return v.valid != 0;
}

bool Optimizer::fallback(bool fail)
{
  if (!fail) {
    retry_counter_ = 0;
    return false;
  }
  reset();
  if (++retry_counter_ > settings_.retry_attempt_limit) {
    retry_counter_ = 0;
    throw std::runtime_error("Optimizer fail to compute path");
  }
  return true;
}

Twist2D Optimizer::evalControl(
  const Pose2D & robot_pose, const Twist2D & robot_speed, const models::Path & plan,
  const Pose2D & goal, float goal_checker_xy_tolerance)
{
  goal_checker_xy_tolerance_ = goal_checker_xy_tolerance;
  prepare(robot_pose, robot_speed, plan, goal);
  do {
    optimize();
  } while (fallback(fail_flag_ || !validated()));
  return finishTick();
}

Twist2D Optimizer::finishTick()
{
  utils::savitskyGolayFilter(control_sequence_, control_history_, settings_);
  auto control = getControlFromSequenceAsTwist();
  if (settings_.shift_control_sequence) {
    shiftControlSequence();
  }
  return control;
}

void Optimizer::shiftControlSequence()
{
  auto roll = [](std::vector<float> & v) {
      if (v.size() < 2) {
        return;
      }
      for (size_t i = 0; i + 1 < v.size(); ++i) {
        v[i] = v[i + 1];
      }
      v[v.size() - 1] = v[v.size() - 2];
    };
  roll(control_sequence_.vx);
  roll(control_sequence_.wz);
  if (isHolonomic()) {
    roll(control_sequence_.vy);
  }
}

Twist2D Optimizer::getControlFromSequenceAsTwist()
{
  const unsigned int offset = settings_.shift_control_sequence ? 1 : 0;
  Twist2D t;
  t.vx = control_sequence_.vx.at(offset);
  t.wz = control_sequence_.wz.at(offset);
  // toTwistStamped(vx, wz, ...) leaves linear.y at 0 for a non-holonomic model (:404-409)
  t.vy = isHolonomic() ? control_sequence_.vy.at(offset) : 0.0f;
  return t;
}

void Optimizer::setSpeedLimit(double speed_limit, bool percentage)
{
  auto & s = settings_;
  constexpr double NO_SPEED_LIMIT = 0.0;   // nav2_costmap_2d filter_values.hpp
  if (speed_limit == NO_SPEED_LIMIT) {
    s.constraints = s.base_constraints;
  } else {
    const double ratio = percentage ? speed_limit / 100.0 : speed_limit / s.base_constraints.vx_max;
    s.constraints.vx_max = s.base_constraints.vx_max * ratio;
    s.constraints.vx_min = s.base_constraints.vx_min * ratio;
    s.constraints.vy = s.base_constraints.vy * ratio;
    s.constraints.wz = s.base_constraints.wz * ratio;
  }
}

std::vector<std::array<float, 3>> integrateControlSequence(
  const models::ControlSequence & sequence, unsigned int T, float dt, const Pose2D & pose, bool holonomic)
{
  // integrateStateVelocities(trajectory, sequence) — optimizer.cpp:275-311: the control
  // sequence itself is integrated (no measured-speed first column here)
  const float initial_yaw = static_cast<float>(pose.yaw);
  std::vector<std::array<float, 3>> traj(T);
  std::vector<float> yaws(T);
  float acc = 0.0f;
  for (unsigned int t = 0; t < T; ++t) {
    const float inc = sequence.wz[t] * dt;
    acc = t == 0 ? inc : acc + inc;
    yaws[t] = acc + initial_yaw;
  }
  float ax = 0.0f, ay = 0.0f;
  for (unsigned int t = 0; t < T; ++t) {
    const float c = t == 0 ? cosf(initial_yaw) : cosf(yaws[t - 1]);
    const float s = t == 0 ? sinf(initial_yaw) : sinf(yaws[t - 1]);
    float dx = sequence.vx[t] * c;
    float dy = sequence.vx[t] * s;
    if (holonomic) {
      dx = dx - sequence.vy[t] * s;
      dy = dy + sequence.vy[t] * c;
    }
    ax = t == 0 ? dx * dt : ax + dx * dt;
    ay = t == 0 ? dy * dt : ay + dy * dt;
    traj[t] = {static_cast<float>(pose.x + static_cast<double>(ax)),
      static_cast<float>(pose.y + static_cast<double>(ay)), yaws[t]};
  }
  return traj;
}

std::vector<std::array<float, 3>> Optimizer::getOptimizedTrajectory()
{
  return integrateControlSequence(control_sequence_, settings_.time_steps, settings_.model_dt, pose_, isHolonomic());
}

void Optimizer::getGeneratedTrajectories(
  std::vector<float> & x, std::vector<float> & y, std::vector<float> & yaws)
{
  const size_t n = static_cast<size_t>(settings_.batch_size) * settings_.time_steps;
  x.resize(n);
  y.resize(n);
  yaws.resize(n);
  ck(ctx_, smpc_get_trajectories(ctx_, x.data(), y.data(), yaws.data()), "smpc_get_trajectories");
}

namespace utils
{

void savitskyGolayFilter(
  models::ControlSequence & control_sequence, std::array<models::Control, 4> & control_history,
  const models::OptimizerSettings & settings)
{
  // Savitzky-Golay quadratic, 9 points: {-21,14,39,54,59,54,39,14,-21}/231, applied in
  // place front to back; the first four outputs lean on the last four executed controls,
  // the tail repeats the last sample; index T-5 is left as is (the reference's loop ends
  // one short and then steps over it, tools/utils.hpp:518-533)
  const unsigned int n = static_cast<unsigned int>(control_sequence.vx.size());
  if (n == 0 || n - 1 < 20) {
    return;
  }
  const unsigned int last = n - 1;
  float w[9] = {-21.0f, 14.0f, 39.0f, 54.0f, 59.0f, 54.0f, 39.0f, 14.0f, -21.0f};
  for (float & c : w) {
    c /= 231.0f;
  }
  auto run = [&](std::vector<float> & q, float h0, float h1, float h2, float h3) {
      const float hist[4] = {h0, h1, h2, h3};
      // sample at signed position i: history for i < 0, clamped to `last` beyond the end
      auto at = [&](int i) -> float {
          if (i < 0) {
            return hist[4 + i];
          }
          return q[static_cast<unsigned int>(i) > last ? last : static_cast<unsigned int>(i)];
        };
      for (unsigned int idx = 0; idx <= last; ++idx) {
        if (idx == last - 4) {
          continue;
        }
        float acc = 0.0f;
        for (int k = 0; k < 9; ++k) {
          acc += at(static_cast<int>(idx) + k - 4) * w[k];
        }
        q[idx] = acc;
      }
    };
  const auto & h = control_history;
  run(control_sequence.vx, h[0].vx, h[1].vx, h[2].vx, h[3].vx);
  run(control_sequence.vy, h[0].vy, h[1].vy, h[2].vy, h[3].vy);
  run(control_sequence.wz, h[0].wz, h[1].wz, h[2].wz, h[3].wz);
  const unsigned int offset = settings.shift_control_sequence ? 1 : 0;
  control_history[0] = control_history[1];
  control_history[1] = control_history[2];
  control_history[2] = control_history[3];
  control_history[3] = {control_sequence.vx[offset], control_sequence.vy[offset],
    control_sequence.wz[offset]};
}

}  // namespace utils
}  // namespace SORTHAM_HOST_NS
