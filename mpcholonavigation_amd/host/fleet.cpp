// fleet.cpp — see fleet.hpp.
#include "fleet.hpp"
#include "../../include/smpc_debug.h"   // smpc_debug_group_moving_launches

#include <algorithm>
#include <cstdlib>
#include <exception>

namespace SORTHAM_HOST_NS
{

// where a member is at each trajectory point, [T][2]: its control sequence integrated from its pose
// (moving), or the pose itself (standing)
static void memberTrack(
  uint8_t state, const models::ControlSequence & seq, uint32_t T, float model_dt, const Pose2D & at, bool holonomic,
  float * out)
{
  const bool moving = state == FLEET_PEER_MOVING;
  std::vector<std::array<float, 3>> traj;
  if (moving) {
    traj = integrateControlSequence(seq, T, model_dt, at, holonomic);
  }
  for (uint32_t t = 0; t < T; ++t) {
    out[2 * t] = moving ? traj[t][0] : static_cast<float>(at.x);
    out[2 * t + 1] = moving ? traj[t][1] : static_cast<float>(at.y);
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
    if (j == i || state[j] == FLEET_PEER_UNSEEN) {continue;}
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
  models::ControlSequence seq;
  for (uint32_t j = 0; j < n; ++j) {
    if (j != i && state[j] != FLEET_PEER_UNSEEN) {
      if (state[j] == FLEET_PEER_MOVING) {
        unpackControls(u + static_cast<size_t>(j) * 3 * T, T, seq);
      }
      memberTrack(
        state[j], seq, T, model_dt[j], Pose2D{pose[3 * j], pose[3 * j + 1], pose[3 * j + 2]}, holonomic[j] != 0,
        &tracks[static_cast<size_t>(j) * T * 2]);
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
  if (!movingObstacleValuesOk(params, robot_radius)) {
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

// what the group at hand has counted, on top of s
void FleetOptimizer::addGroupCounters(FleetStats & s) const
{
  if (!group_) {return;}
  uint64_t a = 0, b = 0;
  smpc_group_stats(group_, &a, &b);
  s.batched_launches += a;
  s.single_ticks += b;
  a = b = 0;
  smpc_debug_group_moving_launches(group_, &a, &b);
  s.grouped_moving_launches += a;
  s.moving_table_uploads += b;
  a = b = 0;
  smpc_group_validation_counts(group_, &a, &b);
  s.validation_launches += a;
  s.validated_members += b;
}

void FleetOptimizer::dropGroup()
{
  if (!group_) {return;}
  addGroupCounters(stats_);
  smpc_group_destroy(group_);
  group_ = nullptr;
  // a table that lived in the group's buffer went with it (smpc.h): the member gets it back through
  // its own handle, so that the context goes on holding what the Optimizer remembers
  for (size_t i = 0; i < members_.size() && i < group_table_.size(); ++i) {
    Optimizer * m = members_[i];
    if (!group_table_[i]) {continue;}
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
  Round & r = round_;
  r.ins.assign(g, smpc_tick_in{});
  r.outs.assign(g, smpc_tick_out{});
  r.take.assign(g, 0);
  r.u.resize(g);
  r.u_ptr.resize(g);
  for (size_t s = 0; s < g; ++s) {
    r.u[s].assign(3 * static_cast<size_t>(members_[owner_[s]]->settings_.time_steps), 0.0f);
    r.u_ptr[s] = r.u[s].data();
  }
  r.vtake.assign(g, 0);
  r.vp.resize(g);
  r.vpose.resize(3 * g);
  r.vu.resize(g);
  r.vout.resize(g);
  r.vstatus.resize(g);
  r.stats.resize(g);
  r.rows.resize(g);
  r.status.resize(g);
  return SMPC_OK;
}

int FleetOptimizer::slotOf(const Optimizer * member, const char * call) const
{
  const size_t i = group_ ? static_cast<size_t>(std::find(members_.begin(), members_.end(), member) - members_.begin()) :
    members_.size();   // (no group: no search either)
  const int s = i < members_.size() ? slot_[i] : -1;
  if (s < 0 && call) {
    throw std::runtime_error(std::string(call) + ": the member has no slot in its fleet's group");
  }
  return s;
}

bool FleetOptimizer::grouped(const Optimizer * member) const {return slotOf(member) >= 0;}

void FleetOptimizer::tickAlone(Optimizer * member, const smpc_tick_in & in, float * u, smpc_tick_out & out)
{
  const size_t s = static_cast<size_t>(slotOf(member, "smpc_optimize"));
  Round & r = round_;
  std::fill(r.take.begin(), r.take.end(), 0);
  r.take[s] = 1;
  r.ins[s] = in;
  std::swap(r.u_ptr[s], u);   // (the caller's sequence, for this call)
  const int rc = smpc_group_optimize_some(group_, r.ins.data(), r.u_ptr.data(), r.outs.data(), r.take.data());
  std::swap(r.u_ptr[s], u);
  if (rc != SMPC_OK) {
    throw std::runtime_error(std::string("smpc_optimize: ") + smpc_last_error(member->ctx_));
  }
  out = r.outs[s];
}

// slot s of the next smpc_group_validate_trajectories call
void FleetOptimizer::Round::wantValidation(
  size_t s, const smpc_validation_params & params, const double * pose, const float * u_s)
{
  vtake[s] = 1;
  vp[s] = params;
  std::copy(pose, pose + 3, vpose.begin() + 3 * s);
  vu[s] = u_s;
}

// what a validation that did not run leaves as its text: the call's own error, or the member's context's
static std::string validationError(int rc, smpc_ctx * ctx)
{
  return std::string("smpc_validate_trajectory: ") +
         (rc != SMPC_OK && rc != SMPC_ERR_DEVICE ? smpc_last_error(nullptr) : smpc_last_error(ctx));
}

void FleetOptimizer::validateAlone(
  Optimizer * member, const smpc_validation_params & params, const double * pose, const float * u,
  smpc_validation & out)
{
  const size_t s = static_cast<size_t>(slotOf(member, "smpc_validate_trajectory"));
  Round & r = round_;
  std::fill(r.vtake.begin(), r.vtake.end(), 0);
  r.wantValidation(s, params, pose, u);
  const int rc = smpc_group_validate_trajectories(
    group_, r.vp.data(), r.vpose.data(), r.vu.data(), r.vtake.data(), r.vout.data(), nullptr, r.vstatus.data());
  if (rc != SMPC_OK || r.vstatus[s] != SMPC_OK) {
    throw std::runtime_error(validationError(rc, member->ctx_));
  }
  out = r.vout[s];
}

// ---- the stages of a round (evalControl) and of a statistics call (getCriticStats) ------------------

// Both calls' opening: one entry per member in every argument (sizes_ok: what Args does not hold), who
// is worked on — the members taken that have a context — and the group formed again where it is stale.
// A member taken that has no context refuses the call (a round), or with `without_context` given gets
// SMPC_ERR_STATE there and the call goes on without it.  round_.any: somebody is left to work on.
int FleetOptimizer::enter(const Args & a, bool sizes_ok, std::vector<MemberCriticStats> * without_context)
{
  const size_t n = members_.size();
  Round & r = round_;
  r.any = false;
  if (!sizes_ok || a.poses.size() < n || a.speeds.size() < n || a.plans.size() < n || a.goals.size() < n ||
    a.tolerances.size() < n || (!a.take.empty() && a.take.size() < n))
  {
    return fail(SMPC_ERR_INVALID, "one pose, speed, plan, goal and tolerance per member");
  }
  r.on.assign(n, 0);
  for (size_t i = 0; i < n; ++i) {
    if (!a.taken(i)) {continue;}
    r.on[i] = members_[i] && members_[i]->ctx_;
    if (r.on[i]) {
      r.any = true;
    } else if (without_context) {
      (*without_context)[i].status = SMPC_ERR_STATE;
      (*without_context)[i].error = "member " + std::to_string(i) + " was shut down or destroyed: it has no context";
    } else {
      return fail(
        SMPC_ERR_STATE, "member " + std::to_string(i) + " was shut down or destroyed: it cannot be taken");
    }
  }
  if (!r.any) {
    return SMPC_OK;
  }
  // no group (a member's context went since the last round), or a member worked on that had no
  // context when the group was formed and has been initialised since: form the group again
  bool stale = !group_;
  for (size_t i = 0; i < n && !stale; ++i) {
    stale = r.on[i] && slot_[i] < 0;
  }
  return stale ? regroup() : SMPC_OK;
}

// prepare, inputs, constraints [ref src/optimizer.cpp:141,185-204]: per member its tolerance, prepare()
// and fillTick() into its slot
int FleetOptimizer::prepareMembers(const Args & a)
{
  Round & r = round_;
  std::fill(r.take.begin(), r.take.end(), 0);
  for (size_t i = 0; i < members_.size(); ++i) {
    if (!r.on[i]) {continue;}
    Optimizer * m = members_[i];
    const size_t s = static_cast<size_t>(slot_[i]);
    try {
      m->goal_checker_xy_tolerance_ = a.tolerances[i];
      m->prepare(a.poses[i], a.speeds[i], a.plans[i], a.goals[i]);
      m->fillTick(r.ins[s], r.u[s].data());
    } catch (const std::exception & e) {
      return fail(SMPC_ERR_STATE, "member " + std::to_string(i) + ": " + e.what());
    }
    r.take[s] = 1;
  }
  return SMPC_OK;
}

// Mutual avoidance: every member taken gets the others as moving obstacles.  Where each member was
// seen last; then, with avoidance on, every seen member's track once per round and every taken
// member's table, the others' tracks put together; then the tables to the library on one of two routes.
int FleetOptimizer::avoidance(const Args & a)
{
  const size_t n = members_.size();
  Round & r = round_;
  seen_.resize(n, 0);
  last_pose_.resize(n);
  for (size_t i = 0; i < n; ++i) {
    if (r.on[i]) {
      seen_[i] = 1;
      last_pose_[i] = a.poses[i];
    }
  }
  if (avoid_radius_.empty()) {
    return SMPC_OK;
  }
  const uint32_t T = members_[owner_[0]]->settings_.time_steps;   // (one for the whole group)
  r.peer.assign(n, FLEET_PEER_UNSEEN);
  r.tracks.assign(n * static_cast<size_t>(T) * 2, 0.0f);
  for (size_t j = 0; j < n; ++j) {
    const Optimizer * m = members_[j];
    if (!seen_[j] || !m) {continue;}
    r.peer[j] = r.on[j] ? FLEET_PEER_MOVING : FLEET_PEER_STANDING;
    memberTrack(
      r.peer[j], m->control_sequence_, T, m->settings_.model_dt, last_pose_[j], m->isHolonomic(),
      &r.tracks[j * static_cast<size_t>(T) * 2]);
  }
  r.tab_xy.resize(n);
  r.tab_r.resize(n);
  for (size_t i = 0; i < n; ++i) {
    if (r.on[i]) {
      assembleAvoidanceTable(
        static_cast<uint32_t>(i), static_cast<uint32_t>(n), T, r.peer.data(), r.tracks.data(), avoid_radius_.data(),
        r.tab_xy[i], r.tab_r[i]);
    }
  }
  return avoid_per_member_ ? avoidPerMember() : avoidGrouped();
}

// SMPC_FLEET_AVOID=per_member: one Optimizer::setMovingObstacles per member
int FleetOptimizer::avoidPerMember()
{
  Round & r = round_;
  for (size_t i = 0; i < members_.size(); ++i) {
    if (!r.on[i]) {continue;}
    try {
      if (r.tab_r[i].empty()) {
        members_[i]->clearMovingObstacles();
      } else {
        members_[i]->setMovingObstacles(avoid_params_, r.tab_xy[i], r.tab_r[i]);
      }
      group_table_[i] = 0;
    } catch (const std::exception & e) {
      return fail(SMPC_ERR_STATE, "member " + std::to_string(i) + ": " + e.what());
    }
  }
  return SMPC_OK;
}

// ONE smpc_group_set_moving_obstacles for all the tables: one staging fill, one upload, one event,
// whatever the fleet's size
int FleetOptimizer::avoidGrouped()
{
  const size_t n = members_.size(), g = owner_.size();
  Round & r = round_;
  r.mov_params.assign(g, avoid_params_);
  r.xy_ptr.assign(g, nullptr);
  r.r_ptr.assign(g, nullptr);
  r.discs.assign(g, 0);
  for (size_t i = 0; i < n; ++i) {
    if (r.on[i]) {
      const size_t s = static_cast<size_t>(slot_[i]);
      r.xy_ptr[s] = r.tab_xy[i].data();
      r.r_ptr[s] = r.tab_r[i].data();
      r.discs[s] = static_cast<uint32_t>(r.tab_r[i].size());
    }
  }
  const int rc = smpc_group_set_moving_obstacles(
    group_, r.mov_params.data(), r.xy_ptr.data(), r.r_ptr.data(), r.discs.data(), r.take.data());
  if (rc != SMPC_OK) {
    // all or nothing: no context has changed, and no member's remembered table either
    return fail(rc, smpc_last_error(nullptr));
  }
  // what each member remembers of its moving obstacles is what its context holds now (getters,
  // re-application after a context is rebuilt)
  for (size_t i = 0; i < n; ++i) {
    if (r.on[i]) {
      Optimizer * m = members_[i];
      m->moving_params_ = avoid_params_;
      m->moving_xy_.swap(r.tab_xy[i]);
      m->moving_radius_.swap(r.tab_r[i]);
      group_table_[i] = m->moving_radius_.empty() ? 0 : 1;
    }
  }
  return SMPC_OK;
}

// ONE grouped tick for all of them
int FleetOptimizer::tick()
{
  const size_t n = members_.size();
  Round & r = round_;
  // (a context keeps the text of its last error: remembered, to tell which member met this one)
  r.errs_before.resize(n);
  for (size_t i = 0; i < n; ++i) {
    if (r.on[i]) {
      r.errs_before[i] = smpc_last_error(members_[i]->ctx_);
    }
  }
  const int rc = smpc_group_optimize_some(group_, r.ins.data(), r.u_ptr.data(), r.outs.data(), r.take.data());
  if (rc == SMPC_OK) {
    return SMPC_OK;
  }
  // nothing was taken over from the round: every member's control sequence, history and retry
  // counter are what they were.  The error text is on the context that met it: a fresh one first,
  // then any that is not empty.
  std::string what;
  for (int fresh = 1; fresh >= 0 && what.empty(); --fresh) {
    for (size_t i = 0; i < n && what.empty(); ++i) {
      if (!r.on[i]) {continue;}
      const std::string now = smpc_last_error(members_[i]->ctx_);
      if (!now.empty() && (!fresh || now != r.errs_before[i])) {
        what = "member " + std::to_string(i) + ": " + now;
      }
    }
  }
  return fail(rc, "smpc_group_optimize_some: " + what);
}

// every member's result taken over (takeTick: the redraw of its noise goes out here); who is
// validated: the members that have trajectory validation on and whose tick did not fail
void FleetOptimizer::takeResults(std::vector<MemberResult> & results)
{
  Round & r = round_;
  r.any_v = false;
  std::fill(r.vtake.begin(), r.vtake.end(), 0);
  for (size_t i = 0; i < members_.size(); ++i) {
    if (!r.on[i]) {continue;}
    Optimizer * m = members_[i];
    const size_t s = static_cast<size_t>(slot_[i]);
    try {
      m->takeTick(r.u[s].data(), r.outs[s]);
    } catch (const std::exception & e) {
      results[i].status = FLEET_THROWN;
      results[i].error = e.what();
      continue;
    }
    if (m->validate_on_ && !m->fail_flag_) {
      // (r.u holds the sequences the round returned: what takeTick copied into the members)
      const double pose[3] = {m->pose_.x, m->pose_.y, m->pose_.yaw};
      r.wantValidation(s, m->validation_params_, pose, r.u[s].data());
      r.any_v = true;
    }
  }
}

// ONE grouped validation of the round's results: one upload, one launch, one wait for all of them
void FleetOptimizer::validateRound(std::vector<MemberResult> & results)
{
  Round & r = round_;
  r.checked.assign(members_.size(), 0);
  if (!r.any_v) {
    return;
  }
  const int rc = smpc_group_validate_trajectories(
    group_, r.vp.data(), r.vpose.data(), r.vu.data(), r.vtake.data(), r.vout.data(), nullptr, r.vstatus.data());
  for (size_t s = 0; s < owner_.size(); ++s) {
    if (!r.vtake[s]) {continue;}
    const size_t i = owner_[s];
    if (rc != SMPC_OK || r.vstatus[s] != SMPC_OK) {
      // what evalControl would have thrown for this member
      results[i].status = FLEET_THROWN;
      results[i].error = validationError(rc, members_[i]->ctx_);
      continue;
    }
    members_[i]->takeValidation(r.vout[s]);
    r.checked[i] = 1;
  }
}

// per member: the reference's loop [ref src/optimizer.cpp:143-154,166-183]
void FleetOptimizer::finishMembers(std::vector<MemberResult> & results)
{
  for (size_t i = 0; i < members_.size(); ++i) {
    if (!round_.on[i]) {continue;}
    Optimizer * m = members_[i];
    MemberResult & res = results[i];
    res.out = m->last_out_;
    if (res.status == FLEET_THROWN) {continue;}
    try {
      bool failed = m->fail_flag_ || (round_.checked[i] && !m->last_validation_.valid);
      while (m->fallback(failed)) {
        stats_.retries++;
        m->optimize();   // alone, fail_flag_in sticky (Optimizer::optimize -> tickAlone)
        failed = m->fail_flag_ || !m->validated();   // (alone too: validateAlone)
      }
      res.twist = m->finishTick();
      res.status = SMPC_OK;
    } catch (const std::exception & e) {
      res.status = FLEET_THROWN;
      res.error = e.what();
    }
    res.out = m->last_out_;
  }
}

int FleetOptimizer::evalControl(
  const std::vector<Pose2D> & poses, const std::vector<Twist2D> & speeds,
  const std::vector<models::Path> & plans, const std::vector<Pose2D> & goals,
  const std::vector<float> & goal_checker_xy_tolerances, const std::vector<uint8_t> & take,
  std::vector<MemberResult> & results)
{
  const Args a{poses, speeds, plans, goals, goal_checker_xy_tolerances, take};
  results.assign(members_.size(), MemberResult{});
  int rc = enter(a, true, nullptr);
  if (rc != SMPC_OK || !round_.any) {
    return rc;
  }
  rc = prepareMembers(a);
  rc = rc == SMPC_OK ? avoidance(a) : rc;
  rc = rc == SMPC_OK ? tick() : rc;
  if (rc != SMPC_OK) {
    return rc;   // the round failed as a whole: no member's result was taken over
  }
  takeResults(results);
  validateRound(results);
  finishMembers(results);
  return SMPC_OK;
}

// the smpc_tick_in evalControl's first optimize() would hand over (prepare() clears the fail flag),
// without touching the members' per-tick state: Optimizer::getCriticStats, per slot
int FleetOptimizer::breakdownFill(const Args & a, const std::vector<float *> & per_rollout)
{
  Round & r = round_;
  std::fill(r.take.begin(), r.take.end(), 0);
  std::fill(r.rows.begin(), r.rows.end(), nullptr);
  std::fill(r.status.begin(), r.status.end(), SMPC_OK);
  for (size_t i = 0; i < members_.size(); ++i) {
    if (!r.on[i]) {continue;}
    Optimizer * m = members_[i];
    const size_t s = static_cast<size_t>(slot_[i]);
    r.ins[s] = tickIn(a.poses[i], a.speeds[i], a.plans[i], a.goals[i], a.tolerances[i], false);
    packControls(m->control_sequence_, m->settings_.time_steps, r.u[s].data());
    try {
      m->pushConstraints();   // (what the tick pushes too: the same values)
    } catch (const std::exception & e) {
      return fail(SMPC_ERR_STATE, "member " + std::to_string(i) + ": " + e.what());
    }
    r.take[s] = 1;
    r.rows[s] = per_rollout.empty() ? nullptr : per_rollout[i];
  }
  return SMPC_OK;
}

// ONE smpc_group_critic_breakdown (a device error is on the context that met it), and every member's entry
int FleetOptimizer::breakdownRun(bool rows, std::vector<MemberCriticStats> & out)
{
  Round & r = round_;
  const int rc = smpc_group_critic_breakdown(
    group_, r.ins.data(), r.u_ptr.data(), r.take.data(), r.stats.data(), rows ? r.rows.data() : nullptr,
    r.status.data());
  if (rc != SMPC_OK) {
    std::string what = smpc_last_error(nullptr);
    for (size_t s = 0; s < owner_.size() && rc == SMPC_ERR_DEVICE; ++s) {
      const std::string now = r.take[s] ? smpc_last_error(members_[owner_[s]]->ctx_) : "";
      if (!now.empty()) {
        what = "member " + std::to_string(owner_[s]) + ": " + now;
        break;
      }
    }
    return fail(rc, "smpc_group_critic_breakdown: " + what);
  }
  for (size_t s = 0; s < owner_.size(); ++s) {
    if (!r.take[s]) {continue;}
    MemberCriticStats & res = out[owner_[s]];
    res.status = r.status[s];
    if (r.status[s] == SMPC_OK) {
      res.stats = r.stats[s];
    } else {
      res.error = std::string("smpc_critic_breakdown: ") + smpc_last_error(members_[owner_[s]]->ctx_);
    }
  }
  return SMPC_OK;
}

int FleetOptimizer::getCriticStats(
  const std::vector<Pose2D> & poses, const std::vector<Twist2D> & speeds,
  const std::vector<models::Path> & plans, const std::vector<Pose2D> & goals,
  const std::vector<float> & goal_checker_xy_tolerances, const std::vector<uint8_t> & take,
  std::vector<MemberCriticStats> & out, const std::vector<float *> & per_rollout)
{
  const Args a{poses, speeds, plans, goals, goal_checker_xy_tolerances, take};
  const size_t n = members_.size();
  out.assign(n, MemberCriticStats{});
  int rc = enter(a, per_rollout.empty() || per_rollout.size() >= n, &out);
  if (rc != SMPC_OK || !round_.any) {
    return rc;
  }
  rc = breakdownFill(a, per_rollout);
  return rc == SMPC_OK ? breakdownRun(!per_rollout.empty(), out) : rc;
}

FleetStats FleetOptimizer::stats() const
{
  FleetStats s = stats_;
  addGroupCounters(s);
  return s;
}

}  // namespace SORTHAM_HOST_NS
