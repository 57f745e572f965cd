// optimizer_c.cpp — extern "C" face of sortham_ns::Optimizer (include/smpc_host.h).
#include <cstring>
#include <exception>
#include <new>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/smpc_host.h"
#include "optimizer_c.hpp"

namespace
{
thread_local std::string g_err;

template<typename F>
int guarded(sortham_optimizer * o, F && f)
{
  try {
    f();
    return SMPC_OK;
  } catch (const std::exception & e) {
    if (o) {
      o->err = e.what();
    } else {
      g_err = e.what();
    }
    return SORTHAM_ERR_THROWN;
  }
}
}  // namespace

namespace {
// the parameter reads of the plugin's Optimizer::getParams() + reset() (nav2_plugin/src/optimizer.cpp)
void initialize_from(sortham_optimizer * o, const sortham_optimizer_config * cfg, const smpc_critic_params * critics)
{
  sortham_ns::models::OptimizerSettings s;
  const smpc_config & b = cfg->base;
  s.base_constraints = {b.vx_max, b.vx_min, b.vy_max, b.wz_max};
  s.sampling_std = {b.vx_std, b.vy_std, b.wz_std};
  s.model_dt = b.model_dt;
  s.temperature = b.temperature;
  s.gamma = b.gamma;
  s.batch_size = b.batch_size;
  s.time_steps = b.time_steps;
  s.iteration_count = b.iteration_count;
  s.retry_attempt_limit = cfg->retry_attempt_limit;
  sortham_ns::CriticsConfig cc;
  cc.params = *critics;
  for (uint32_t i = 0; i < cfg->n_critics && i < 16; ++i) {
    cc.critics.emplace_back(cfg->critics[i] ? cfg->critics[i] : "");
  }
  cc.cost_scaling_factor = cfg->cost_scaling_factor;
  cc.inflation_radius = cfg->inflation_radius;
  o->opt.setVisualize(cfg->visualize != 0);
  o->opt.setLanePerRollout((b.flags & SMPC_FLAG_LANE_PER_ROLLOUT) != 0);
  o->opt.setAckermannMinTurningRadius(b.ackermann_min_turning_r);
  o->opt.initialize(
    s, cfg->motion_model ? cfg->motion_model : "DiffDrive", cfg->controller_frequency, cc,
    cfg->regenerate_noises != 0, cfg->noise_seed, b.device);
  o->opt.applyFootprint(o->footprint_xy, o->circumscribed_radius, o->layer_cost_scaling_factor);
}
}  // namespace

extern "C" {

int sortham_optimizer_create(
  const sortham_optimizer_config * cfg, const smpc_critic_params * critics,
  sortham_optimizer ** out)
{
  if (!cfg || !critics || !out) {
    return SMPC_ERR_INVALID;
  }
  *out = nullptr;
  auto * o = new (std::nothrow) sortham_optimizer();
  if (!o) {
    return SMPC_ERR_NOMEM;
  }
  int rc = guarded(nullptr, [&]() {initialize_from(o, cfg, critics);});
  if (rc != SMPC_OK) {
    delete o;
    return rc;
  }
  *out = o;
  return SMPC_OK;
}

int sortham_optimizer_initialize(
  sortham_optimizer * o, const sortham_optimizer_config * cfg, const smpc_critic_params * critics)
{
  if (!o || !cfg || !critics) {
    return SMPC_ERR_INVALID;
  }
  return guarded(o, [&]() {initialize_from(o, cfg, critics);});
}

void sortham_optimizer_destroy(sortham_optimizer * o) {delete o;}

const char * sortham_optimizer_last_error(const sortham_optimizer * o)
{
  return o ? o->err.c_str() : g_err.c_str();
}

int sortham_optimizer_set_costmap(
  sortham_optimizer * o, const uint8_t * cells, uint32_t width, uint32_t height, double origin_x,
  double origin_y, double resolution, int track_unknown, float inscribed_radius,
  int has_inflation_layer)
{
  if (!o) {return SMPC_ERR_INVALID;}
  return guarded(
    o, [&]() {
      sortham_ns::CostmapView m;
      m.cells = cells;
      m.size_x = width;
      m.size_y = height;
      m.origin_x = origin_x;
      m.origin_y = origin_y;
      m.resolution = resolution;
      m.track_unknown = track_unknown != 0;
      m.inscribed_radius = inscribed_radius;
      m.has_inflation_layer = has_inflation_layer != 0;
      m.footprint_xy = o->footprint_xy;
      m.circumscribed_radius = o->circumscribed_radius;
      m.layer_cost_scaling_factor = o->layer_cost_scaling_factor;
      o->opt.setCostmap(m);
    });
}

int sortham_optimizer_set_footprint(
  sortham_optimizer * o, const double * xy, uint32_t n_points, double circumscribed_radius,
  double layer_cost_scaling_factor)
{
  if (!o || !xy || n_points == 0) {return SMPC_ERR_INVALID;}
  if (n_points > SMPC_MAX_FOOTPRINT) {return SMPC_ERR_UNSUPPORTED;}
  return guarded(
    o, [&]() {
      o->footprint_xy.assign(xy, xy + 2 * static_cast<size_t>(n_points));
      o->circumscribed_radius = circumscribed_radius;
      o->layer_cost_scaling_factor = layer_cost_scaling_factor;
      o->opt.applyFootprint(o->footprint_xy, circumscribed_radius, layer_cost_scaling_factor);
    });
}

int sortham_optimizer_set_noise(
  sortham_optimizer * o, const float * nvx, const float * nvy, const float * nwz)
{
  if (!o) {return SMPC_ERR_INVALID;}
  return guarded(o, [&]() {o->opt.setNoise(nvx, nvy, nwz);});
}

int sortham_optimizer_eval_control(
  sortham_optimizer * o, const smpc_tick_in * in, double * twist_out, smpc_tick_out * out)
{
  if (!o || !in || !twist_out) {return SMPC_ERR_INVALID;}
  return guarded(
    o, [&]() {
      const sortham_ns::TickInput ti = sortham_ns::tickInputFrom(*in);
      const sortham_ns::Twist2D t =
        o->opt.evalControl(ti.robot_pose, ti.robot_speed, ti.plan, ti.goal, ti.goal_checker_xy_tolerance);
      twist_out[0] = t.vx;
      twist_out[1] = t.vy;
      twist_out[2] = t.wz;
      if (out) {*out = o->opt.lastTick();}
    });
}

int sortham_optimizer_critic_stats(
  sortham_optimizer * o, const smpc_tick_in * in, smpc_critic_stats * stats, float * per_rollout)
{
  if (!o || !in || !stats) {return SMPC_ERR_INVALID;}
  return guarded(
    o, [&]() {*stats = o->opt.getCriticStats(sortham_ns::tickInputFrom(*in), per_rollout);});
}

int sortham_optimizer_last_tick(const sortham_optimizer * o, smpc_tick_out * out)
{
  if (!o || !out) {return SMPC_ERR_INVALID;}
  *out = o->opt.lastTick();
  return SMPC_OK;
}

int sortham_optimizer_set_acceleration_limits(
  sortham_optimizer * o, float ax_max, float ax_min, float ay_max, float az_max)
{
  if (!o) {return SMPC_ERR_INVALID;}
  return guarded(o, [&]() {o->opt.setAccelerationLimits(ax_max, ax_min, ay_max, az_max);});
}

int sortham_optimizer_set_moving_obstacles(
  sortham_optimizer * o, const smpc_moving_obstacles_params * params, const float * xy, const float * radius,
  uint32_t n, uint32_t time_steps)
{
  if (!o || (n && (!params || !xy || !radius || time_steps == 0))) {return SMPC_ERR_INVALID;}
  if (n > SMPC_MAX_MOVING_OBSTACLES) {return SMPC_ERR_UNSUPPORTED;}
  return guarded(
    o, [&]() {
      if (n == 0) {
        o->opt.clearMovingObstacles();
        return;
      }
      o->opt.setMovingObstacles(
        *params, std::vector<float>(xy, xy + static_cast<size_t>(n) * time_steps * 2),
        std::vector<float>(radius, radius + n));
    });
}

int sortham_optimizer_moving_obstacle_costs(sortham_optimizer * o, float * m, uint8_t * hit, uint32_t batch_size)
{
  if (!o || !m) {return SMPC_ERR_INVALID;}
  return guarded(
    o, [&]() {
      std::vector<float> vm;
      std::vector<uint8_t> vh;
      o->opt.getMovingObstacleCosts(vm, vh);
      if (vm.size() != batch_size) {throw std::runtime_error("moving_obstacle_costs: batch_size is not the optimizer's");}
      std::memcpy(m, vm.data(), vm.size() * sizeof(float));
      if (hit) {std::memcpy(hit, vh.data(), vh.size());}
    });
}

int sortham_optimizer_set_trajectory_validation(sortham_optimizer * o, const smpc_validation_params * params)
{
  if (!o) {return SMPC_ERR_INVALID;}
  return guarded(
    o, [&]() {
      if (params) {
        o->opt.setTrajectoryValidation(*params);
      } else {
        o->opt.clearTrajectoryValidation();
      }
    });
}

int sortham_optimizer_last_validation(
  const sortham_optimizer * o, smpc_validation * out, uint64_t * run, uint64_t * invalid)
{
  if (!o) {return SMPC_ERR_INVALID;}
  if (out) {*out = o->opt.lastValidation();}
  if (run) {*run = o->opt.validationsRun();}
  if (invalid) {*invalid = o->opt.validationsFailed();}
  return SMPC_OK;
}

int sortham_optimizer_set_speed_limit(sortham_optimizer * o, double speed_limit, int percentage)
{
  if (!o) {return SMPC_ERR_INVALID;}
  return guarded(o, [&]() {o->opt.setSpeedLimit(speed_limit, percentage != 0);});
}

int sortham_optimizer_reset(sortham_optimizer * o)
{
  if (!o) {return SMPC_ERR_INVALID;}
  return guarded(o, [&]() {o->opt.reset();});
}

int sortham_optimizer_get_control_sequence(sortham_optimizer * o, float * u)
{
  if (!o || !u) {return SMPC_ERR_INVALID;}
  const auto & cs = o->opt.controlSequence();
  sortham_ns::packControls(cs, cs.vx.size(), u);
  return SMPC_OK;
}

int sortham_optimizer_set_control_sequence(sortham_optimizer * o, const float * u)
{
  if (!o || !u) {return SMPC_ERR_INVALID;}
  auto & cs = o->opt.controlSequence();
  sortham_ns::unpackControls(u, cs.vx.size(), cs);
  return SMPC_OK;
}

int sortham_optimizer_get_constraints(sortham_optimizer * o, float * c4, int32_t * shift)
{
  if (!o || !c4) {return SMPC_ERR_INVALID;}
  const auto & s = o->opt.settings();
  c4[0] = s.constraints.vx_max;
  c4[1] = s.constraints.vx_min;
  c4[2] = s.constraints.vy;
  c4[3] = s.constraints.wz;
  if (shift) {*shift = s.shift_control_sequence ? 1 : 0;}
  return SMPC_OK;
}

int sortham_optimizer_get_optimized_trajectory(sortham_optimizer * o, float * xyyaw)
{
  if (!o || !xyyaw) {return SMPC_ERR_INVALID;}
  return guarded(
    o, [&]() {
      const auto tr = o->opt.getOptimizedTrajectory();
      for (size_t t = 0; t < tr.size(); ++t) {
        xyyaw[3 * t] = tr[t][0];
        xyyaw[3 * t + 1] = tr[t][1];
        xyyaw[3 * t + 2] = tr[t][2];
      }
    });
}

void sortham_utils_savitsky_golay(float * u, uint32_t T, float * history, int shift)
{
  sortham_ns::models::ControlSequence cs;
  sortham_ns::unpackControls(u, T, cs);
  std::array<sortham_ns::models::Control, 4> h;
  for (int i = 0; i < 4; ++i) {
    h[i] = {history[3 * i], history[3 * i + 1], history[3 * i + 2]};
  }
  sortham_ns::models::OptimizerSettings s;
  s.shift_control_sequence = shift != 0;
  sortham_ns::utils::savitskyGolayFilter(cs, h, s);
  sortham_ns::packControls(cs, T, u);
  for (int i = 0; i < 4; ++i) {
    history[3 * i] = h[i].vx;
    history[3 * i + 1] = h[i].vy;
    history[3 * i + 2] = h[i].wz;
  }
}

}  // extern "C"
