// fleet.hpp — Optimizer::evalControl for N robots through one grouped tick.
//
// A fleet host holds N sortham::Optimizer objects, one per robot.  FleetOptimizer ticks the ones
// a round takes with ONE smpc_group_optimize_some call (include/smpc.h: one upload, one scoring
// launch per instance, one reduction for all of them) and then runs, per member, exactly what
// Optimizer::evalControl runs around its own smpc_optimize call [ref src/optimizer.cpp:134-225]:
// fallback / reset / retry / throw, the Savitzky-Golay filter, Twist extraction, the shift.  The
// pieces are the members' own (Optimizer::fillTick / takeTick / fallback / finishTick): a member of
// a fleet computes what it computes alone, bit for bit.  A round is a list of stages (fleet.cpp; DESIGN.md
// §4.7a): enter -> prepareMembers -> avoidance -> tick -> takeResults -> validateRound -> finishMembers;
// getCriticStats is enter -> breakdownFill -> breakdownRun.  Their state is one Round, kept between rounds.
//
// The caller keeps ownership of the optimizers and goes on using them through their own
// interface between rounds (setCostmap, setSpeedLimit, reset, setNoise, controlSequence(),
// initialize() again, shutdown()).  Single-threaded: one round, or one member call, at a time.
// Order of destruction: any; a member that is shut down or destroyed leaves the fleet's group
// first (smpc.h: the group goes before its contexts), and destroying the fleet hands every
// context back to its own stream.
#ifndef SORTHAM_HOST_FLEET_HPP_
#define SORTHAM_HOST_FLEET_HPP_

#include <stdexcept>
#include <string>
#include <vector>

#include "optimizer.hpp"

namespace SORTHAM_HOST_NS
{

// A member's status after a round: SMPC_OK, FLEET_NOT_TAKEN (positive: nothing of its changed) or
// FLEET_THROWN where evalControl would have thrown (the text is in MemberResult::error).
constexpr int FLEET_NOT_TAKEN = 1;
constexpr int FLEET_THROWN = -10;   // SORTHAM_ERR_THROWN of include/smpc_host.h

struct FleetError : std::runtime_error
{
  FleetError(int c, const std::string & what)
  : std::runtime_error(what), code(c) {}
  int code;   // SMPC_ERR_*
};

struct MemberResult
{
  Twist2D twist{};
  smpc_tick_out out{};
  int status{FLEET_NOT_TAKEN};
  std::string error;
};

// A member's entry of FleetOptimizer::getCriticStats: status SMPC_OK with the statistics,
// FLEET_NOT_TAKEN (nothing written), or the SMPC_ERR_* Optimizer::getCriticStats would have thrown
// with (the text in error); SMPC_ERR_STATE for a member without a context.
struct MemberCriticStats
{
  smpc_critic_stats stats{};
  int status{FLEET_NOT_TAKEN};
  std::string error;
};

struct FleetStats
{
  uint64_t batched_launches{0};   // smpc_group_stats, summed over the groups the fleet has had
  uint64_t single_ticks{0};       // (the retries below included: they are ticked alone)
  uint64_t retries{0};            // optimize() calls of the fallback loop
  // mutual avoidance on the grouped route (smpc_debug_group_moving_launches, summed like the above):
  uint64_t grouped_moving_launches{0};   // launches of the grouped moving-obstacle kernels
  uint64_t moving_table_uploads{0};      // uploads of a group's table buffer (one per round)
  // trajectory validation (smpc_group_validation_counts, summed like the above):
  uint64_t validation_launches{0};       // grouped validation calls that had a member to check: one per round, and
                                         // one per retry of a member alone
  uint64_t validated_members{0};         // the members they carried
};

// What a fleet knows of member j when it builds the others' obstacle tables.
constexpr uint8_t FLEET_PEER_UNSEEN = 0;     // never taken: left out
constexpr uint8_t FLEET_PEER_STANDING = 1;   // not taken this round: a disc standing at its last pose
constexpr uint8_t FLEET_PEER_MOVING = 2;     // taken this round: its control sequence integrated from this round's pose

// The moving-obstacle table of member i (smpc_set_moving_obstacles) from what the fleet knows of the
// n members: one disc per other member j that has been seen, in the order of j, radius
// robot_radius[i] + robot_radius[j]; a moving j by integrateControlSequence on u[j] = [3][T] (vx, vy,
// wz) from pose[j] = {x, y, yaw}, a standing j at pose[j] for every t.  xy: [discs][T][2], radius:
// [discs].  Pure host code: no context, no device.
void buildMutualAvoidanceTable(
  uint32_t i, uint32_t n, uint32_t time_steps, const uint8_t * state, const double * pose, const float * u,
  const float * model_dt, const uint8_t * holonomic, const float * robot_radius, std::vector<float> & xy,
  std::vector<float> & radius);

class FleetOptimizer : public FleetLink
{
public:
  // Throws FleetError: SMPC_ERR_INVALID for no member, a null one or one listed twice,
  // SMPC_ERR_STATE for one that is not initialised or is in a fleet already; what
  // smpc_group_create refuses (members on different devices or with different time_steps), with
  // its message.
  explicit FleetOptimizer(const std::vector<Optimizer *> & members);
  ~FleetOptimizer() override;
  FleetOptimizer(const FleetOptimizer &) = delete;
  FleetOptimizer & operator=(const FleetOptimizer &) = delete;

  size_t size() const {return members_.size();}
  // null once the member was destroyed
  Optimizer * member(size_t i) const {return members_[i];}

  // One round.  Every vector has size() entries; the entries of a member that is not taken are
  // not looked at.  take: one byte per member, empty = everybody.  Returns SMPC_OK, or the
  // SMPC_ERR_* of a round that failed as a whole (text in lastError()): then no member's control
  // sequence, filter history or retry counter has moved, and the next round is safe to run.
  // A round that takes a member which was shut down or destroyed is SMPC_ERR_STATE.
  // Trajectory validation (Optimizer::setTrajectoryValidation on the members): behind the grouped tick
  // ONE smpc_group_validate_trajectories call covers the members taken that have it on and did not
  // fail; an invalid member takes its own retry path — reset, a tick and a validation alone — and
  // the others are untouched.
  int evalControl(
    const std::vector<Pose2D> & poses, const std::vector<Twist2D> & speeds,
    const std::vector<models::Path> & plans, const std::vector<Pose2D> & goals,
    const std::vector<float> & goal_checker_xy_tolerances, const std::vector<uint8_t> & take,
    std::vector<MemberResult> & results);

  // Optimizer::getCriticStats for the members taken, the fleet staying grouped (smpc.h:
  // smpc_group_critic_breakdown — launches whose number does not depend on the fleet's size): per
  // member the statistics of the tick the next evalControl round would run first, from its control
  // sequence as it stands, its constraints pushed as getCriticStats pushes them.  Arguments as
  // evalControl's; per_rollout: empty, or one pointer per member (null, or
  // [SMPC_STATS_ROWS][batch_size] floats).  Regroups first if the fleet is ungrouped.  Changes
  // nothing: the next round returns what it would have returned without the call.  Returns SMPC_OK,
  // or the SMPC_ERR_* of a call that failed as a whole (text in lastError()).
  int getCriticStats(
    const std::vector<Pose2D> & poses, const std::vector<Twist2D> & speeds,
    const std::vector<models::Path> & plans, const std::vector<Pose2D> & goals,
    const std::vector<float> & goal_checker_xy_tolerances, const std::vector<uint8_t> & take,
    std::vector<MemberCriticStats> & out, const std::vector<float *> & per_rollout = {});

  // Mutual avoidance: before a round's ticks every member taken gets the others as moving obstacles
  // (buildMutualAvoidanceTable; the tables of all members taken go to the library in ONE
  // smpc_group_set_moving_obstacles call — one upload for the fleet — and each replaces whatever the
  // member had, in the context and in what the Optimizer remembers alike; with SMPC_FLEET_AVOID=per_member
  // in the environment when the fleet is created: one Optimizer::setMovingObstacles per member, the
  // same tables and results).  robot_radius: one per member, > 0; empty: off — the default — and every member's
  // table is cleared.  Throws FleetError(SMPC_ERR_INVALID) for a wrong count or values the library
  // would refuse.  Members share time_steps (smpc_group_create) and are expected to share model_dt:
  // trajectory point t of one member is then the time of point t of another.
  void setMutualAvoidance(const smpc_moving_obstacles_params & params, const std::vector<float> & robot_radius);

  FleetStats stats() const;
  const std::string & lastError() const {return err_;}

  // the members' contexts back on their own streams until the next round (which regroups): for a
  // caller that wants to tick members through their own evalControl on the ungrouped path
  void ungroup() {dropGroup();}

  // FleetLink
  void dropGroup() override;
  void memberDestroyed(Optimizer * member) override;
  bool grouped(const Optimizer * member) const override;
  void tickAlone(Optimizer * member, const smpc_tick_in & in, float * u, smpc_tick_out & out) override;
  void validateAlone(
    Optimizer * member, const smpc_validation_params & params, const double * pose, const float * u,
    smpc_validation & out) override;

private:
  // the caller's arguments of a round or a statistics call, as the stages pass them on
  struct Args
  {
    const std::vector<Pose2D> & poses;
    const std::vector<Twist2D> & speeds;
    const std::vector<models::Path> & plans;
    const std::vector<Pose2D> & goals;
    const std::vector<float> & tolerances;
    const std::vector<uint8_t> & take;
    bool taken(size_t i) const {return take.empty() || take[i] != 0;}
  };
  // What one call's stages hand on.  A member of the fleet, so that its vectors keep their capacity
  // from round to round: a round in the steady state allocates nothing here.  tickAlone and
  // validateAlone, a retry's calls, borrow the per-slot arrays once the round is done with them.
  struct Round
  {
    bool any{false}, any_v{false};       // somebody to work on (enter), somebody to validate (takeResults)
    // per member: taken and with a context (enter); FLEET_PEER_* and the tracks [T][2] (avoidance), the
    // table while it is assembled; the error text before the grouped tick; its verdict was taken over
    std::vector<uint8_t> on, peer, checked;
    std::vector<float> tracks;
    std::vector<std::vector<float>> tab_xy, tab_r;
    std::vector<std::string> errs_before;
    // per group slot, sized by regroup(): the arguments of the grouped tick (u: [3][T] each) ...
    std::vector<smpc_tick_in> ins;
    std::vector<smpc_tick_out> outs;
    std::vector<std::vector<float>> u;
    std::vector<float *> u_ptr;
    std::vector<uint8_t> take;
    // ... of smpc_group_set_moving_obstacles ...
    std::vector<smpc_moving_obstacles_params> mov_params;
    std::vector<const float *> xy_ptr, r_ptr;
    std::vector<uint32_t> discs;
    // ... of smpc_group_validate_trajectories (vpose: [3] each; one slot: wantValidation) ...
    std::vector<uint8_t> vtake;
    std::vector<smpc_validation_params> vp;
    std::vector<double> vpose;
    std::vector<const float *> vu;
    std::vector<smpc_validation> vout;
    // ... and what smpc_group_critic_breakdown returns
    std::vector<smpc_critic_stats> stats;
    std::vector<float *> rows;
    std::vector<int32_t> vstatus, status;
    void wantValidation(size_t s, const smpc_validation_params & params, const double * pose, const float * u_s);
  };

  int regroup();
  int fail(int code, const std::string & what);
  // the member's slot in the group; without one -1, or with `call` given what that call throws
  int slotOf(const Optimizer * member, const char * call = nullptr) const;
  void addGroupCounters(FleetStats & s) const;
  // the stages of a call (fleet.cpp, in this order)
  int enter(const Args & a, bool sizes_ok, std::vector<MemberCriticStats> * without_context);
  int prepareMembers(const Args & a);
  int avoidance(const Args & a);
  int avoidPerMember();
  int avoidGrouped();
  int tick();
  void takeResults(std::vector<MemberResult> & results);
  void validateRound(std::vector<MemberResult> & results);
  void finishMembers(std::vector<MemberResult> & results);
  int breakdownFill(const Args & a, const std::vector<float *> & per_rollout);
  int breakdownRun(bool rows, std::vector<MemberCriticStats> & out);

  std::vector<Optimizer *> members_;
  smpc_group * group_{nullptr};
  std::vector<int> slot_;             // member -> index in the group, -1: no context
  std::vector<size_t> owner_;         // group index -> member
  Round round_;
  // mutual avoidance: the parameters, one radius per member (empty: off), and where each member was seen last
  smpc_moving_obstacles_params avoid_params_{};
  std::vector<float> avoid_radius_;
  std::vector<uint8_t> seen_;
  bool avoid_per_member_{false};      // SMPC_FLEET_AVOID=per_member, read when the fleet is created
  std::vector<uint8_t> group_table_;  // per member: its table lives in the group's buffer
  std::vector<Pose2D> last_pose_;     // per member
  FleetStats stats_{};                // of the groups already dropped, and the retries
  std::string err_;
};

}  // namespace SORTHAM_HOST_NS

#endif
