// fleet.cpp — see fleet.hpp.
#include "fleet.hpp"
#include "../../include/smpc_debug.h"   // smpc_debug_group_moving_launches

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <exception>

namespace SORTHAM_HOST_NS
{

// where member j is at each trajectory point, [T][2]: its control sequence integrated from its pose
// (moving), or the pose itself (standing)
static void peerTrack(
  uint32_t j, uint32_t T, const uint8_t * state, const double * pose, const float * u, const float * model_dt,
  const uint8_t * holonomic, float * out)
{
  const Pose2D at{pose[3 * j], pose[3 * j + 1], pose[3 * j + 2]};
  if (state[j] == FLEET_PEER_MOVING) {
    models::ControlSequence seq;
    const float * uj = u + static_cast<size_t>(j) * 3 * T;
    seq.vx.assign(uj, uj + T);
    seq.vy.assign(uj + T, uj + 2 * T);
    seq.wz.assign(uj + 2 * T, uj + 3 * T);
    const auto traj = integrateControlSequence(seq, T, model_dt[j], at, holonomic[j] != 0);
    for (uint32_t t = 0; t < T; ++t) {
      out[2 * t] = traj[t][0];
      out[2 * t + 1] = traj[t][1];
    }
  } else {
    for (uint32_t t = 0; t < T; ++t) {
      out[2 * t] = static_cast<float>(at.x);
      out[2 * t + 1] = static_cast<float>(at.y);
    }
  }
}

// member i's table from every seen member's track [n][T][2]: the others', in the order of j
static void assembleAvoidanceTable(
  uint32_t i, uint32_t n, uint32_t T, const uint8_t * state, const float * tracks, const float * robot_radius,
  std::vector<float> & xy, std::vector<float> & radius)
{
  xy.clear();
  radius.clear();
  for (uint32_t j = 0; j < n; ++j) {
    if (j == i || state[j] == FLEET_PEER_UNSEEN) {
      continue;
    }
    radius.push_back(robot_radius[i] + robot_radius[j]);
    const float * tr = tracks + static_cast<size_t>(j) * T * 2;
    xy.insert(xy.end(), tr, tr + static_cast<size_t>(T) * 2);
  }
}

void buildMutualAvoidanceTable(
  uint32_t i, uint32_t n, uint32_t T, const uint8_t * state, const double * pose, const float * u,
  const float * model_dt, const uint8_t * holonomic, const float * robot_radius, std::vector<float> & xy,
  std::vector<float> & radius)
{
  std::vector<float> tracks(static_cast<size_t>(n) * T * 2, 0.0f);
  for (uint32_t j = 0; j < n; ++j) {
    if (j != i && state[j] != FLEET_PEER_UNSEEN) {
      peerTrack(j, T, state, pose, u, model_dt, holonomic, &tracks[static_cast<size_t>(j) * T * 2]);
    }
  }
  assembleAvoidanceTable(i, n, T, state, tracks.data(), robot_radius, xy, radius);
}

void FleetOptimizer::setMutualAvoidance(
  const smpc_moving_obstacles_params & params, const std::vector<float> & robot_radius)
{
  if (robot_radius.empty()) {
    const bool was_on = !avoid_radius_.empty();
    avoid_radius_.clear();
    for (Optimizer * m : members_) {
      if (was_on && m) {
        m->clearMovingObstacles();
      }
    }
    return;
  }
  if (robot_radius.size() != members_.size()) {
    throw FleetError(SMPC_ERR_INVALID, "setMutualAvoidance: one radius per member");
  }
  if (members_.size() - 1 > SMPC_MAX_MOVING_OBSTACLES) {
    throw FleetError(SMPC_ERR_UNSUPPORTED, "setMutualAvoidance: more than SMPC_MAX_MOVING_OBSTACLES other members");
  }
  bool ok = std::isfinite(params.collision_cost) && std::isfinite(params.repulsion_weight) &&
    std::isfinite(params.margin) && params.collision_cost >= 0.0f && params.repulsion_weight >= 0.0f &&
    params.margin > 0.0f;
  for (float r : robot_radius) {
    ok = ok && std::isfinite(r) && r > 0.0f;
  }
  if (!ok) {
    throw FleetError(
            SMPC_ERR_INVALID,
            "setMutualAvoidance: collision_cost >= 0, repulsion_weight >= 0, margin > 0, every radius > 0, all finite");
  }
  avoid_params_ = params;
  avoid_radius_ = robot_radius;
}

FleetOptimizer::FleetOptimizer(const std::vector<Optimizer *> & members)
{
  if (members.empty()) {
    throw FleetError(SMPC_ERR_INVALID, "a fleet needs a member");
  }
  for (size_t i = 0; i < members.size(); ++i) {
    Optimizer * m = members[i];
    if (!m) {
      throw FleetError(SMPC_ERR_INVALID, "member " + std::to_string(i) + " is null");
    }
    if (std::find(members.begin(), members.begin() + i, m) != members.begin() + i) {
      throw FleetError(SMPC_ERR_INVALID, "member " + std::to_string(i) + " is listed twice");
    }
    if (!m->initialized()) {
      throw FleetError(SMPC_ERR_STATE, "member " + std::to_string(i) + " is not initialised");
    }
    if (m->fleet_) {
      throw FleetError(SMPC_ERR_STATE, "member " + std::to_string(i) + " is in a fleet already");
    }
  }
  members_ = members;
  for (Optimizer * m : members_) {
    m->fleet_ = this;
  }
  // SMPC_FLEET_AVOID=per_member: mutual avoidance keeps the per-member route (one
  // setMovingObstacles per member and round) — to measure the two routes in one process, and a way back
  const char * route = std::getenv("SMPC_FLEET_AVOID");
  avoid_per_member_ = route && std::string(route) == "per_member";
  group_table_.assign(members_.size(), 0);
  const int rc = regroup();
  if (rc != SMPC_OK) {
    for (Optimizer * m : members_) {
      m->fleet_ = nullptr;
    }
    throw FleetError(rc, err_);
  }
}

FleetOptimizer::~FleetOptimizer()
{
  dropGroup();   // smpc_group_destroy: every context back on its own stream
  for (Optimizer * m : members_) {
    if (m) {
      m->fleet_ = nullptr;
    }
  }
}

int FleetOptimizer::fail(int code, const std::string & what)
{
  err_ = what;
  return code;
}

void FleetOptimizer::dropGroup()
{
  if (!group_) {
    return;
  }
  uint64_t launches = 0, singles = 0;
  smpc_group_stats(group_, &launches, &singles);
  stats_.batched_launches += launches;
  stats_.single_ticks += singles;
  uint64_t moving = 0, uploads = 0;
  smpc_debug_group_moving_launches(group_, &moving, &uploads);
  stats_.grouped_moving_launches += moving;
  stats_.moving_table_uploads += uploads;
  uint64_t vlaunches = 0, vmembers = 0;
  smpc_group_validation_counts(group_, &vlaunches, &vmembers);
  stats_.validation_launches += vlaunches;
  stats_.validated_members += vmembers;
  smpc_group_destroy(group_);
  group_ = nullptr;
  // a table that lived in the group's buffer went with it (smpc.h): the member gets it back through
  // its own handle, so that the context goes on holding what the Optimizer remembers
  for (size_t i = 0; i < members_.size() && i < group_table_.size(); ++i) {
    Optimizer * m = members_[i];
    if (!group_table_[i]) {
      continue;
    }
    group_table_[i] = 0;
    if (m && m->ctx_ && !m->moving_radius_.empty()) {
      try {
        m->pushMovingObstacles();
      } catch (const std::exception &) {
        // (a device error, or a member in the middle of initialize() with another horizon: what it
        // remembers stays, and initialize() hands it to the new context or refuses it, as ever)
      }
    }
  }
}

void FleetOptimizer::memberDestroyed(Optimizer * member)
{
  // (its context is gone already, and the group with it: Optimizer::destroyContext)
  std::replace(members_.begin(), members_.end(), member, static_cast<Optimizer *>(nullptr));
}

// one group over the contexts the members have now; a member without one has no slot
int FleetOptimizer::regroup()
{
  dropGroup();
  const size_t n = members_.size();
  slot_.assign(n, -1);
  owner_.clear();
  std::vector<smpc_ctx *> ctxs;
  for (size_t i = 0; i < n; ++i) {
    if (members_[i] && members_[i]->ctx_) {
      slot_[i] = static_cast<int>(ctxs.size());
      ctxs.push_back(members_[i]->ctx_);
      owner_.push_back(i);
    }
  }
  if (ctxs.empty()) {
    return fail(SMPC_ERR_STATE, "no member of the fleet has a context");
  }
  const int rc = smpc_group_create(ctxs.data(), static_cast<uint32_t>(ctxs.size()), &group_);
  if (rc != SMPC_OK) {
    group_ = nullptr;
    return fail(rc, std::string("smpc_group_create: ") + smpc_last_error(nullptr));
  }
  if (avoid_per_member_) {
    smpc_debug_group_moving_per_member(group_, 1);   // the riders' moving-obstacle launches per member too
  }
  const size_t g = ctxs.size();
  ins_.assign(g, smpc_tick_in{});
  outs_.assign(g, smpc_tick_out{});
  take_.assign(g, 0);
  u_.resize(g);
  u_ptr_.resize(g);
  for (size_t s = 0; s < g; ++s) {
    u_[s].assign(3 * static_cast<size_t>(members_[owner_[s]]->settings_.time_steps), 0.0f);
    u_ptr_[s] = u_[s].data();
  }
  return SMPC_OK;
}

bool FleetOptimizer::grouped(const Optimizer * member) const
{
  if (!group_) {
    return false;
  }
  const size_t i = static_cast<size_t>(std::find(members_.begin(), members_.end(), member) - members_.begin());
  return i < members_.size() && slot_[i] >= 0;
}

void FleetOptimizer::tickAlone(Optimizer * member, const smpc_tick_in & in, float * u, smpc_tick_out & out)
{
  const size_t i = static_cast<size_t>(std::find(members_.begin(), members_.end(), member) - members_.begin());
  if (!group_ || i >= members_.size() || slot_[i] < 0) {
    throw std::runtime_error("smpc_optimize: the member has no slot in its fleet's group");
  }
  const size_t s = static_cast<size_t>(slot_[i]);
  std::vector<float *> ptrs(u_ptr_);
  ptrs[s] = u;
  std::fill(take_.begin(), take_.end(), 0);
  take_[s] = 1;
  ins_[s] = in;
  const int rc = smpc_group_optimize_some(group_, ins_.data(), ptrs.data(), outs_.data(), take_.data());
  if (rc != SMPC_OK) {
    throw std::runtime_error(std::string("smpc_optimize: ") + smpc_last_error(member->ctx_));
  }
  out = outs_[s];
}

void FleetOptimizer::validateAlone(
  Optimizer * member, const smpc_validation_params & params, const double * pose, const float * u,
  smpc_validation & out)
{
  const size_t i = static_cast<size_t>(std::find(members_.begin(), members_.end(), member) - members_.begin());
  if (!group_ || i >= members_.size() || slot_[i] < 0) {
    throw std::runtime_error("smpc_validate_trajectory: the member has no slot in its fleet's group");
  }
  const size_t s = static_cast<size_t>(slot_[i]), g = owner_.size();
  std::vector<smpc_validation_params> p(g, params);
  std::vector<double> ps(3 * g, 0.0);
  std::vector<const float *> us(g, nullptr);
  std::vector<uint8_t> tk(g, 0);
  std::vector<smpc_validation> outs(g);
  std::vector<int32_t> status(g, SMPC_OK);
  std::copy(pose, pose + 3, ps.begin() + 3 * s);
  us[s] = u;
  tk[s] = 1;
  const int rc = smpc_group_validate_trajectories(
    group_, p.data(), ps.data(), us.data(), tk.data(), outs.data(), nullptr, status.data());
  if (rc != SMPC_OK || status[s] != SMPC_OK) {
    throw std::runtime_error(
            std::string("smpc_validate_trajectory: ") + (rc != SMPC_OK && rc != SMPC_ERR_DEVICE ?
            smpc_last_error(nullptr) : smpc_last_error(member->ctx_)));
  }
  out = outs[s];
}

int FleetOptimizer::evalControl(
  const std::vector<Pose2D> & poses, const std::vector<Twist2D> & speeds,
  const std::vector<models::Path> & plans, const std::vector<Pose2D> & goals,
  const std::vector<float> & goal_checker_xy_tolerances, const std::vector<uint8_t> & take,
  std::vector<MemberResult> & results)
{
  const size_t n = members_.size();
  results.assign(n, MemberResult{});
  if (poses.size() < n || speeds.size() < n || plans.size() < n || goals.size() < n ||
    goal_checker_xy_tolerances.size() < n || (!take.empty() && take.size() < n))
  {
    return fail(SMPC_ERR_INVALID, "one pose, speed, plan, goal and tolerance per member");
  }
  auto taken = [&](size_t i) {return take.empty() || take[i] != 0;};
  bool any = false;
  for (size_t i = 0; i < n; ++i) {
    if (!taken(i)) {
      continue;
    }
    any = true;
    if (!members_[i] || !members_[i]->ctx_) {
      return fail(
        SMPC_ERR_STATE, "member " + std::to_string(i) + " was shut down or destroyed: it cannot be taken");
    }
  }
  if (!any) {
    return SMPC_OK;
  }
  // no group (a member's context went since the last round), or a member taken that had no
  // context when the group was formed and has been initialised since: form the group again
  bool stale = !group_;
  for (size_t i = 0; i < n && !stale; ++i) {
    stale = taken(i) && slot_[i] < 0;
  }
  if (stale) {
    const int rc = regroup();
    if (rc != SMPC_OK) {
      return rc;
    }
  }
  // ---- prepare, inputs, constraints [ref src/optimizer.cpp:141,185-204] -----------------------
  std::fill(take_.begin(), take_.end(), 0);
  for (size_t i = 0; i < n; ++i) {
    if (!taken(i)) {
      continue;
    }
    Optimizer * m = members_[i];
    const size_t s = static_cast<size_t>(slot_[i]);
    try {
      m->goal_checker_xy_tolerance_ = goal_checker_xy_tolerances[i];
      m->prepare(poses[i], speeds[i], plans[i], goals[i]);
      m->fillTick(ins_[s], u_[s].data());
    } catch (const std::exception & e) {
      return fail(SMPC_ERR_STATE, "member " + std::to_string(i) + ": " + e.what());
    }
    take_[s] = 1;
  }
  // ---- mutual avoidance: every member taken gets the others as moving obstacles ----------------
  seen_.resize(n, 0);
  last_pose_.resize(3 * n, 0.0);
  for (size_t i = 0; i < n; ++i) {
    if (taken(i)) {
      seen_[i] = 1;
      last_pose_[3 * i] = poses[i].x;
      last_pose_[3 * i + 1] = poses[i].y;
      last_pose_[3 * i + 2] = poses[i].yaw;
    }
  }
  if (!avoid_radius_.empty()) {
    const uint32_t T = members_[owner_[0]]->settings_.time_steps;   // (one for the whole group)
    std::vector<uint8_t> state(n, FLEET_PEER_UNSEEN), holo(n, 0);
    std::vector<float> u(n * 3 * static_cast<size_t>(T), 0.0f), dt(n, 0.0f);
    for (size_t j = 0; j < n; ++j) {
      const Optimizer * m = members_[j];
      if (!seen_[j] || !m) {
        continue;
      }
      state[j] = taken(j) ? FLEET_PEER_MOVING : FLEET_PEER_STANDING;
      holo[j] = m->isHolonomic() ? 1 : 0;
      dt[j] = m->settings_.model_dt;
      if (taken(j)) {
        std::memcpy(&u[j * 3 * T], m->control_sequence_.vx.data(), T * sizeof(float));
        std::memcpy(&u[j * 3 * T + T], m->control_sequence_.vy.data(), T * sizeof(float));
        std::memcpy(&u[j * 3 * T + 2 * T], m->control_sequence_.wz.data(), T * sizeof(float));
      }
    }
    // every seen member's track once per round; a member's table is the others' tracks put together
    std::vector<float> tracks(n * static_cast<size_t>(T) * 2, 0.0f);
    for (size_t j = 0; j < n; ++j) {
      if (state[j] != FLEET_PEER_UNSEEN) {
        peerTrack(
          static_cast<uint32_t>(j), T, state.data(), last_pose_.data(), u.data(), dt.data(), holo.data(),
          &tracks[j * static_cast<size_t>(T) * 2]);
      }
    }
    if (avoid_per_member_) {
      std::vector<float> xy, radius;
      for (size_t i = 0; i < n; ++i) {
        if (!taken(i)) {
          continue;
        }
        assembleAvoidanceTable(
          static_cast<uint32_t>(i), static_cast<uint32_t>(n), T, state.data(), tracks.data(), avoid_radius_.data(), xy,
          radius);
        try {
          if (radius.empty()) {
            members_[i]->clearMovingObstacles();
          } else {
            members_[i]->setMovingObstacles(avoid_params_, xy, radius);
          }
          group_table_[i] = 0;
        } catch (const std::exception & e) {
          return fail(SMPC_ERR_STATE, "member " + std::to_string(i) + ": " + e.what());
        }
      }
    } else {
      // every taken member's table as above, then ONE smpc_group_set_moving_obstacles for all of them:
      // one staging fill, one upload, one event, whatever the fleet's size
      const size_t g = owner_.size();
      tab_xy_.resize(n);
      tab_r_.resize(n);
      std::vector<smpc_moving_obstacles_params> params(g, avoid_params_);
      std::vector<const float *> xy_ptr(g, nullptr), r_ptr(g, nullptr);
      std::vector<uint32_t> discs(g, 0);
      for (size_t i = 0; i < n; ++i) {
        if (!taken(i)) {
          continue;
        }
        const size_t s = static_cast<size_t>(slot_[i]);
        assembleAvoidanceTable(
          static_cast<uint32_t>(i), static_cast<uint32_t>(n), T, state.data(), tracks.data(), avoid_radius_.data(),
          tab_xy_[i], tab_r_[i]);
        xy_ptr[s] = tab_xy_[i].data();
        r_ptr[s] = tab_r_[i].data();
        discs[s] = static_cast<uint32_t>(tab_r_[i].size());
      }
      const int rc = smpc_group_set_moving_obstacles(
        group_, params.data(), xy_ptr.data(), r_ptr.data(), discs.data(), take_.data());
      if (rc != SMPC_OK) {
        // all or nothing: no context has changed, and no member's remembered table either
        return fail(rc, smpc_last_error(nullptr));
      }
      // what each member remembers of its moving obstacles is what its context holds now (getters,
      // re-application after a context is rebuilt)
      for (size_t i = 0; i < n; ++i) {
        if (!taken(i)) {
          continue;
        }
        Optimizer * m = members_[i];
        m->moving_params_ = avoid_params_;
        m->moving_xy_.swap(tab_xy_[i]);
        m->moving_radius_.swap(tab_r_[i]);
        group_table_[i] = m->moving_radius_.empty() ? 0 : 1;
      }
    }
  }
  // ---- ONE grouped tick for all of them ------------------------------------------------------
  // (a context keeps the text of its last error: remembered, to tell which member met this one)
  errs_before_.resize(n);
  for (size_t i = 0; i < n; ++i) {
    if (taken(i)) {
      errs_before_[i] = smpc_last_error(members_[i]->ctx_);
    }
  }
  const int rc = smpc_group_optimize_some(group_, ins_.data(), u_ptr_.data(), outs_.data(), take_.data());
  if (rc != SMPC_OK) {
    // nothing was taken over from the round: every member's control sequence, history and retry
    // counter are what they were.  The error text is on the context that met it.
    std::string what;
    for (int fresh = 1; fresh >= 0 && what.empty(); --fresh) {
      for (size_t i = 0; i < n && what.empty(); ++i) {
        if (!taken(i)) {
          continue;
        }
        const std::string now = smpc_last_error(members_[i]->ctx_);
        if (!now.empty() && (!fresh || now != errs_before_[i])) {
          what = "member " + std::to_string(i) + ": " + now;
        }
      }
    }
    return fail(rc, "smpc_group_optimize_some: " + what);
  }
  // ---- every member's result taken over, then ONE grouped validation of the round's results -----
  // (the members taken that have trajectory validation on and whose tick did not fail: one upload,
  // one launch, one wait for all of them)
  const size_t g = owner_.size();
  std::vector<uint8_t> vtake(g, 0), checked(n, 0);
  bool any_v = false;
  for (size_t i = 0; i < n; ++i) {
    if (!taken(i)) {
      continue;
    }
    Optimizer * m = members_[i];
    const size_t s = static_cast<size_t>(slot_[i]);
    try {
      m->takeTick(u_[s].data(), outs_[s]);
    } catch (const std::exception & e) {
      results[i].status = FLEET_THROWN;
      results[i].error = e.what();
      continue;
    }
    if (m->validate_on_ && !m->fail_flag_) {
      vtake[s] = 1;
      any_v = true;
    }
  }
  if (any_v) {
    // (u_ holds the sequences the round returned: what takeTick copied into the members)
    std::vector<smpc_validation_params> vp(g);
    std::vector<double> vpose(3 * g, 0.0);
    std::vector<const float *> vu(g, nullptr);
    std::vector<smpc_validation> vout(g);
    std::vector<int32_t> vstatus(g, SMPC_OK);
    for (size_t s = 0; s < g; ++s) {
      if (!vtake[s]) {
        continue;
      }
      const Optimizer * m = members_[owner_[s]];
      vp[s] = m->validation_params_;
      vpose[3 * s] = m->pose_.x;
      vpose[3 * s + 1] = m->pose_.y;
      vpose[3 * s + 2] = m->pose_.yaw;
      vu[s] = u_[s].data();
    }
    const int vrc = smpc_group_validate_trajectories(
      group_, vp.data(), vpose.data(), vu.data(), vtake.data(), vout.data(), nullptr, vstatus.data());
    for (size_t s = 0; s < g; ++s) {
      if (!vtake[s]) {
        continue;
      }
      const size_t i = owner_[s];
      if (vrc != SMPC_OK || vstatus[s] != SMPC_OK) {
        // what evalControl would have thrown for this member
        results[i].status = FLEET_THROWN;
        results[i].error = std::string("smpc_validate_trajectory: ") +
          (vrc != SMPC_OK && vrc != SMPC_ERR_DEVICE ? smpc_last_error(nullptr) : smpc_last_error(members_[i]->ctx_));
        continue;
      }
      members_[i]->takeValidation(vout[s]);
      checked[i] = 1;
    }
  }
  // ---- per member: the reference's loop [ref src/optimizer.cpp:143-154,166-183] ---------------
  for (size_t i = 0; i < n; ++i) {
    if (!taken(i)) {
      continue;
    }
    Optimizer * m = members_[i];
    MemberResult & r = results[i];
    r.out = m->last_out_;
    if (r.status == FLEET_THROWN) {
      continue;
    }
    try {
      bool failed = m->fail_flag_ || (checked[i] && !m->last_validation_.valid);
      while (m->fallback(failed)) {
        stats_.retries++;
        m->optimize();   // alone, fail_flag_in sticky (Optimizer::optimize -> tickAlone)
        failed = m->fail_flag_ || !m->validated();   // (alone too: validateAlone)
      }
      r.twist = m->finishTick();
      r.status = SMPC_OK;
    } catch (const std::exception & e) {
      r.status = FLEET_THROWN;
      r.error = e.what();
    }
    r.out = m->last_out_;
  }
  return SMPC_OK;
}

int FleetOptimizer::getCriticStats(
  const std::vector<Pose2D> & poses, const std::vector<Twist2D> & speeds,
  const std::vector<models::Path> & plans, const std::vector<Pose2D> & goals,
  const std::vector<float> & goal_checker_xy_tolerances, const std::vector<uint8_t> & take,
  std::vector<MemberCriticStats> & out, const std::vector<float *> & per_rollout)
{
  const size_t n = members_.size();
  out.assign(n, MemberCriticStats{});
  if (poses.size() < n || speeds.size() < n || plans.size() < n || goals.size() < n ||
    goal_checker_xy_tolerances.size() < n || (!take.empty() && take.size() < n) ||
    (!per_rollout.empty() && per_rollout.size() < n))
  {
    return fail(SMPC_ERR_INVALID, "one pose, speed, plan, goal and tolerance per member");
  }
  auto taken = [&](size_t i) {return take.empty() || take[i] != 0;};
  bool any = false;
  for (size_t i = 0; i < n; ++i) {
    if (!taken(i)) {
      continue;
    }
    if (!members_[i] || !members_[i]->ctx_) {
      out[i].status = SMPC_ERR_STATE;
      out[i].error = "member " + std::to_string(i) + " was shut down or destroyed: it has no context";
      continue;
    }
    any = true;
  }
  if (!any) {
    return SMPC_OK;
  }
  // (as a round: no group, or a member taken that got its context after the group was formed)
  bool stale = !group_;
  for (size_t i = 0; i < n && !stale; ++i) {
    stale = taken(i) && out[i].status != SMPC_ERR_STATE && slot_[i] < 0;
  }
  if (stale) {
    const int rc = regroup();
    if (rc != SMPC_OK) {
      return rc;
    }
  }
  // the smpc_tick_in evalControl's first optimize() would hand over (prepare() clears the fail
  // flag), without touching the members' per-tick state: Optimizer::getCriticStats, per slot
  const size_t g = owner_.size();
  std::vector<smpc_tick_in> ins(g);
  std::vector<std::vector<float>> u(g);
  std::vector<const float *> u_ptr(g, nullptr);
  std::vector<uint8_t> tk(g, 0);
  std::vector<smpc_critic_stats> st(g);
  std::vector<float *> rows(g, nullptr);
  std::vector<int32_t> status(g, SMPC_OK);
  for (size_t i = 0; i < n; ++i) {
    if (!taken(i) || out[i].status == SMPC_ERR_STATE) {
      continue;
    }
    Optimizer * m = members_[i];
    const size_t s = static_cast<size_t>(slot_[i]);
    smpc_tick_in & in = ins[s];
    std::memset(&in, 0, sizeof(in));
    in.pose_x = poses[i].x;
    in.pose_y = poses[i].y;
    in.pose_yaw = static_cast<float>(poses[i].yaw);
    in.speed_vx = speeds[i].vx;
    in.speed_vy = speeds[i].vy;
    in.speed_wz = speeds[i].wz;
    in.path_x = plans[i].x.data();
    in.path_y = plans[i].y.data();
    in.path_yaw = plans[i].yaws.data();
    in.path_len = static_cast<uint32_t>(plans[i].x.size());
    in.goal_x = goals[i].x;
    in.goal_y = goals[i].y;
    in.goal_checker_xy_tolerance = goal_checker_xy_tolerances[i];
    const unsigned int T = m->settings_.time_steps;
    u[s].resize(3 * static_cast<size_t>(T));
    std::memcpy(u[s].data(), m->control_sequence_.vx.data(), T * sizeof(float));
    std::memcpy(u[s].data() + T, m->control_sequence_.vy.data(), T * sizeof(float));
    std::memcpy(u[s].data() + 2 * T, m->control_sequence_.wz.data(), T * sizeof(float));
    u_ptr[s] = u[s].data();
    try {
      m->pushConstraints();   // (what the tick pushes too: the same values)
    } catch (const std::exception & e) {
      return fail(SMPC_ERR_STATE, "member " + std::to_string(i) + ": " + e.what());
    }
    tk[s] = 1;
    rows[s] = per_rollout.empty() ? nullptr : per_rollout[i];
  }
  const int rc = smpc_group_critic_breakdown(
    group_, ins.data(), u_ptr.data(), tk.data(), st.data(), per_rollout.empty() ? nullptr : rows.data(),
    status.data());
  if (rc != SMPC_OK) {
    std::string what = smpc_last_error(nullptr);
    for (size_t s = 0; s < g && rc == SMPC_ERR_DEVICE; ++s) {
      const std::string now = tk[s] ? smpc_last_error(members_[owner_[s]]->ctx_) : "";
      if (!now.empty()) {
        what = "member " + std::to_string(owner_[s]) + ": " + now;
        break;
      }
    }
    return fail(rc, "smpc_group_critic_breakdown: " + what);
  }
  for (size_t s = 0; s < g; ++s) {
    if (!tk[s]) {
      continue;
    }
    MemberCriticStats & r = out[owner_[s]];
    r.status = status[s];
    if (status[s] == SMPC_OK) {
      r.stats = st[s];
    } else {
      r.error = std::string("smpc_critic_breakdown: ") + smpc_last_error(members_[owner_[s]]->ctx_);
    }
  }
  return SMPC_OK;
}

FleetStats FleetOptimizer::stats() const
{
  FleetStats s = stats_;
  if (group_) {
    uint64_t launches = 0, singles = 0;
    smpc_group_stats(group_, &launches, &singles);
    s.batched_launches += launches;
    s.single_ticks += singles;
    uint64_t moving = 0, uploads = 0;
    smpc_debug_group_moving_launches(group_, &moving, &uploads);
    s.grouped_moving_launches += moving;
    s.moving_table_uploads += uploads;
    uint64_t vlaunches = 0, vmembers = 0;
    smpc_group_validation_counts(group_, &vlaunches, &vmembers);
    s.validation_launches += vlaunches;
    s.validated_members += vmembers;
  }
  return s;
}

}  // namespace SORTHAM_HOST_NS
