// fleet.cpp — see fleet.hpp.
#include "fleet.hpp"

#include <algorithm>
#include <exception>

namespace SORTHAM_HOST_NS
{

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
  smpc_group_destroy(group_);
  group_ = nullptr;
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
  // ---- per member: the reference's loop [ref src/optimizer.cpp:143-154,166-183] ---------------
  for (size_t i = 0; i < n; ++i) {
    if (!taken(i)) {
      continue;
    }
    Optimizer * m = members_[i];
    const size_t s = static_cast<size_t>(slot_[i]);
    MemberResult & r = results[i];
    try {
      m->takeTick(u_[s].data(), outs_[s]);
      while (m->fallback(m->fail_flag_)) {
        stats_.retries++;
        m->optimize();   // alone, fail_flag_in sticky (Optimizer::optimize -> tickAlone)
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

FleetStats FleetOptimizer::stats() const
{
  FleetStats s = stats_;
  if (group_) {
    uint64_t launches = 0, singles = 0;
    smpc_group_stats(group_, &launches, &singles);
    s.batched_launches += launches;
    s.single_ticks += singles;
  }
  return s;
}

}  // namespace SORTHAM_HOST_NS
