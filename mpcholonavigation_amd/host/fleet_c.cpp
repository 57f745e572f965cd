// fleet_c.cpp — extern "C" face of sortham_ns::FleetOptimizer (include/smpc_host.h).
#include <algorithm>
#include <exception>
#include <initializer_list>
#include <new>
#include <utility>

#include "fleet_c.hpp"

namespace
{
thread_local std::string g_fleet_err;

// the caller's blocks taken apart into the round's arguments, which the handle keeps between rounds;
// a member taken whose plan is missing refuses the call (text in f->err)
int unpackRound(sortham_fleet * f, const smpc_tick_in * ins, const uint8_t * take)
{
  for (size_t i = 0; i < f->handles.size(); ++i) {
    f->take[i] = (!take || take[i]) ? 1 : 0;
    if (!f->take[i]) {
      continue;
    }
    const smpc_tick_in & in = ins[i];
    if (in.path_len && (!in.path_x || !in.path_y || !in.path_yaw)) {
      f->err = "member " + std::to_string(i) + ": null plan";
      return SMPC_ERR_INVALID;
    }
    sortham_ns::tickInputFrom(in, f->poses[i], f->speeds[i], f->plans[i], f->goals[i], f->tolerances[i]);
  }
  return SMPC_OK;
}
// the fleet's counters asked for, each through a pointer that may be null
int putCounters(
  const sortham_fleet * f, std::initializer_list<std::pair<uint64_t *, uint64_t sortham_ns::FleetStats::*>> which)
{
  if (!f) {
    return SMPC_ERR_INVALID;
  }
  const sortham_ns::FleetStats s = f->fleet->stats();
  for (const auto & w : which) {
    if (w.first) {
      *w.first = s.*w.second;
    }
  }
  return SMPC_OK;
}
}  // namespace

extern "C" {

int sortham_fleet_create(sortham_optimizer * const * members, uint32_t n, sortham_fleet ** out)
{
  if (out) {
    *out = nullptr;
  }
  if (!members || n == 0 || !out) {
    g_fleet_err = "null argument";
    return SMPC_ERR_INVALID;
  }
  std::vector<sortham_ns::Optimizer *> opts;
  for (uint32_t i = 0; i < n; ++i) {
    if (!members[i]) {
      g_fleet_err = "member " + std::to_string(i) + " is null";
      return SMPC_ERR_INVALID;
    }
    opts.push_back(&members[i]->opt);
  }
  try {
    std::unique_ptr<sortham_fleet> f(new sortham_fleet());
    f->fleet.reset(new sortham_ns::FleetOptimizer(opts));
    f->handles.assign(members, members + n);
    f->poses.resize(n);
    f->goals.resize(n);
    f->speeds.resize(n);
    f->plans.resize(n);
    f->tolerances.assign(n, -1.0f);
    f->take.assign(n, 1);
    *out = f.release();
    return SMPC_OK;
  } catch (const sortham_ns::FleetError & e) {
    g_fleet_err = e.what();
    return e.code;
  } catch (const std::bad_alloc &) {
    g_fleet_err = "out of memory";
    return SMPC_ERR_NOMEM;
  } catch (const std::exception & e) {
    g_fleet_err = e.what();
    return SORTHAM_ERR_THROWN;
  }
}

void sortham_fleet_destroy(sortham_fleet * f) {delete f;}

const char * sortham_fleet_last_error(const sortham_fleet * f)
{
  return f ? f->err.c_str() : g_fleet_err.c_str();
}

int sortham_fleet_eval_control(
  sortham_fleet * f, const smpc_tick_in * ins, const uint8_t * take, double * twists,
  smpc_tick_out * outs, int32_t * status)
{
  if (!f || !ins || !twists || !status) {
    return SMPC_ERR_INVALID;
  }
  const size_t n = f->handles.size();
  try {
    int rc = unpackRound(f, ins, take);
    if (rc != SMPC_OK) {
      return rc;
    }
    rc = f->fleet->evalControl(f->poses, f->speeds, f->plans, f->goals, f->tolerances, f->take, f->results);
    if (rc != SMPC_OK) {
      f->err = f->fleet->lastError();
      return rc;
    }
  } catch (const std::exception & e) {
    f->err = e.what();
    return SORTHAM_ERR_THROWN;
  }
  for (size_t i = 0; i < n; ++i) {
    const sortham_ns::MemberResult & r = f->results[i];
    status[i] = r.status;
    if (r.status == sortham_ns::FLEET_NOT_TAKEN) {
      continue;
    }
    twists[3 * i] = r.twist.vx;
    twists[3 * i + 1] = r.twist.vy;
    twists[3 * i + 2] = r.twist.wz;
    if (outs) {
      outs[i] = r.out;
    }
    if (r.status == SORTHAM_ERR_THROWN && f->fleet->member(i)) {
      f->handles[i]->err = r.error;
    }
  }
  return SMPC_OK;
}

int sortham_fleet_critic_stats(
  sortham_fleet * f, const smpc_tick_in * ins, const uint8_t * take, smpc_critic_stats * stats,
  float * const * per_rollout, int32_t * status)
{
  if (!f || !ins || !stats || !status) {
    return SMPC_ERR_INVALID;
  }
  const size_t n = f->handles.size();
  std::vector<sortham_ns::MemberCriticStats> res;
  try {
    int rc = unpackRound(f, ins, take);
    if (rc != SMPC_OK) {
      return rc;
    }
    std::vector<float *> rows;
    if (per_rollout) {
      rows.assign(per_rollout, per_rollout + n);
    }
    rc = f->fleet->getCriticStats(f->poses, f->speeds, f->plans, f->goals, f->tolerances, f->take, res, rows);
    if (rc != SMPC_OK) {
      f->err = f->fleet->lastError();
      return rc;
    }
  } catch (const std::exception & e) {
    f->err = e.what();
    return SORTHAM_ERR_THROWN;
  }
  for (size_t i = 0; i < n; ++i) {
    status[i] = res[i].status;
    if (res[i].status == SMPC_OK) {
      stats[i] = res[i].stats;
    } else if (res[i].status != sortham_ns::FLEET_NOT_TAKEN && f->fleet->member(i)) {
      f->handles[i]->err = res[i].error;
    }
  }
  return SMPC_OK;
}

int sortham_fleet_set_mutual_avoidance(
  sortham_fleet * f, const smpc_moving_obstacles_params * params, const float * robot_radius, uint32_t n)
{
  if (!f || (n && (!params || !robot_radius))) {
    return SMPC_ERR_INVALID;
  }
  try {
    smpc_moving_obstacles_params p{};
    if (params) {
      p = *params;
    }
    f->fleet->setMutualAvoidance(p, n ? std::vector<float>(robot_radius, robot_radius + n) : std::vector<float>());
    return SMPC_OK;
  } catch (const sortham_ns::FleetError & e) {
    f->err = e.what();
    return e.code;
  } catch (const std::exception & e) {
    f->err = e.what();
    return SORTHAM_ERR_THROWN;
  }
}

int sortham_fleet_avoidance_table(
  uint32_t i, uint32_t n, uint32_t time_steps, const uint8_t * state, const double * pose, const float * u,
  const float * model_dt, const uint8_t * holonomic, const float * robot_radius, float * xy, float * radius,
  uint32_t * discs)
{
  if (!state || !pose || !u || !model_dt || !holonomic || !robot_radius || !xy || !radius || !discs || i >= n ||
    time_steps == 0)
  {
    return SMPC_ERR_INVALID;
  }
  std::vector<float> t_xy, t_r;
  sortham_ns::buildMutualAvoidanceTable(i, n, time_steps, state, pose, u, model_dt, holonomic, robot_radius, t_xy, t_r);
  std::copy(t_xy.begin(), t_xy.end(), xy);
  std::copy(t_r.begin(), t_r.end(), radius);
  *discs = static_cast<uint32_t>(t_r.size());
  return SMPC_OK;
}

int sortham_fleet_stats(
  const sortham_fleet * f, uint64_t * batched_launches, uint64_t * single_ticks, uint64_t * retries)
{
  using S = sortham_ns::FleetStats;
  return putCounters(f, {{batched_launches, &S::batched_launches}, {single_ticks, &S::single_ticks}, {retries, &S::retries}});
}

int sortham_fleet_validation_counts(const sortham_fleet * f, uint64_t * launches, uint64_t * members)
{
  using S = sortham_ns::FleetStats;
  return putCounters(f, {{launches, &S::validation_launches}, {members, &S::validated_members}});
}

int sortham_fleet_moving_launches(const sortham_fleet * f, uint64_t * grouped_launches, uint64_t * table_uploads)
{
  using S = sortham_ns::FleetStats;
  return putCounters(f, {{grouped_launches, &S::grouped_moving_launches}, {table_uploads, &S::moving_table_uploads}});
}

}  // extern "C"
