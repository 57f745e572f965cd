// smpc_group.h — the group object behind smpc_group_* (include/smpc.h), shared by smpc_group.cpp
// (rounds of ticks) and smpc_stats.cpp (smpc_group_critic_breakdown).  Internal: not part of the
// C-ABI.
#ifndef SMPC_GROUP_H_
#define SMPC_GROUP_H_

#include "smpc_ctx.h"
#include "smpc_group_layout.h"

#pragma GCC visibility push(hidden)

// ---- the group's parts, as the context's (smpc_ctx.h): each owns what it allocates (smpc_own.h) ----
namespace smpc_impl {

// n tick blocks, then SmpcDev[n], SmpcReduceArgs[n], SmpcWaveGeom[n], SmpcMovingMember[n].  While the group stands, each
// member's tick views (smpc_ctx.h: TickBlock) point at its slot of the two; the group owns them.
// Behind `at.round` (a round never uploads them) the further argument arrays of
// smpc_group_critic_breakdown: the pre-pass's parameter blocks and geometry, the members' rows, the
// reduction's arguments.  Where each stands: GroupLayout (smpc_group_layout.h); what each is, here.
struct GroupArrays {
  PinnedBuf<uint8_t> h_all;
  DevBuf<uint8_t> d_all;
  GroupLayout at;
  // The tick slots take the MEMBER index i (a member's views point at its slot for the group's life).
  uint8_t* h_slot(uint32_t i) const {return h_all.get() + at.slot * i;}
  uint8_t* d_slot(uint32_t i) const {return d_all.get() + at.slot * i;}
  // The argument arrays take the RIDER position j (GroupPartition::order, or a breakdown's order): a
  // launch reads the run [first, first + count) of them.  h_*: the pinned copy a call fills; d_*: the
  // device copy from rider `first` on, what a launch is given.
  SmpcDev* h_dev() const {return host<SmpcDev>(at.dev);}
  SmpcReduceArgs* h_red() const {return host<SmpcReduceArgs>(at.red);}
  SmpcWaveGeom* h_geo() const {return host<SmpcWaveGeom>(at.geo);}
  SmpcMovingMember* h_mov() const {return host<SmpcMovingMember>(at.mov);}   // (position among the members of its form, the forms in turn)
  const SmpcDev* d_dev(uint32_t first = 0) const {return dev<SmpcDev>(at.dev) + first;}
  const SmpcReduceArgs* d_red() const {return dev<SmpcReduceArgs>(at.red);}
  const SmpcWaveGeom* d_geo(uint32_t first = 0) const {return dev<SmpcWaveGeom>(at.geo) + first;}
  const SmpcMovingMember* d_mov(uint32_t first = 0) const {return dev<SmpcMovingMember>(at.mov) + first;}
  // the breakdown's own (the pre-pass's two: position among the members that need a furthest point)
  SmpcDev* h_fdev() const {return host<SmpcDev>(at.fdev);}
  SmpcWaveGeom* h_fgeo() const {return host<SmpcWaveGeom>(at.fgeo);}
  SmpcStatsDst* h_sdst() const {return host<SmpcStatsDst>(at.sdst);}
  SmpcStatsReduceArgs* h_sred() const {return host<SmpcStatsReduceArgs>(at.sred);}
  const SmpcDev* d_fdev() const {return dev<SmpcDev>(at.fdev);}
  const SmpcWaveGeom* d_fgeo() const {return dev<SmpcWaveGeom>(at.fgeo);}
  const SmpcStatsDst* d_sdst() const {return dev<SmpcStatsDst>(at.sdst);}
  const SmpcStatsReduceArgs* d_sred() const {return dev<SmpcStatsReduceArgs>(at.sred);}

 private:
  template <typename X> X* host(size_t off) const {return reinterpret_cast<X*>(h_all.get() + off);}
  template <typename X> const X* dev(size_t off) const {return reinterpret_cast<const X*>(d_all.get() + off);}
};

// ---- moving obstacles (smpc_group_set_moving_obstacles; the grouped launch of a round) ----
// the members' tables back to back: ONE device allocation (n x the capacity of a member's own), ONE
// upload on the group's stream and the event behind it.  The staging buffer comes in two copies
// that take turns: a call packs into the one the last upload did not read, and carries the tables
// of the members it does not take over from the other (at / used: where a member's table
// stands, in floats).  The members' table views (smpc_ctx.h: MovingObstacles) point into tab.
struct GroupMoving {
  Event ev_up;
  PinnedBuf<float> stage[2];
  int cur = 0;                          // the staging copy the last upload read
  DevBuf<float> tab;
  std::vector<size_t> at, used;
  bool up_recorded = false;
  bool per_member = false;   // smpc_debug_group_moving_per_member: use_moving_seed per rider, no grouped launch
};

// ---- smpc_group_critic_breakdown (smpc_stats.cpp) ----
// the members' float regions in ONE allocation (GroupStatsArena in smpc_stats.cpp), sized at the
// first grouped breakdown and again when the members taken or their batch sizes ask for more; the
// reduction's double partials likewise; the results' pinned landing place
struct GroupStatsBufs {
  DevBuf<float> d_stats;
  DevBuf<double> d_part;
  PinnedBuf<float> h_out;
  bool lds_set = false;
};

struct GroupCounters {
  uint64_t batched_ticks = 0, single_ticks = 0;
  uint64_t batched_launches = 0;   // scoring launches that carried two or more members (smpc_group_stats)
  uint64_t moving_launches = 0, moving_uploads = 0;   // smpc_debug_group_moving_launches
  uint64_t breakdown_batched = 0, breakdown_single = 0;   // member-breakdowns by route (smpc_group_breakdown_counts)
  uint64_t validate_launches = 0, validate_members = 0;   // smpc_group_validation_counts
};

}  // namespace smpc_impl

extern "C" {

struct smpc_group {
  std::vector<smpc_ctx*> ctxs;
  std::vector<hipStream_t> saved_stream;
  hipStream_t stream = nullptr;   // the first member's own stream: not the group's to destroy
  // a batched launch went out and not every riding member's fetch_out has returned since: a round
  // abandoned on an error leaves it set, and the next round waits for the stream before it writes
  // the arrays again
  bool launched = false;
  smpc_impl::GroupArrays arr;
  smpc_impl::GroupMoving mov;
  smpc_impl::GroupStatsBufs stats;
  smpc_impl::ValidateBufs val;    // smpc_group_validate_trajectories
  smpc_impl::GroupCounters count;
};

}  // extern "C"

namespace smpc_impl {

// ---- what the entry points of a group share (smpc_group.cpp) ----
inline bool group_takes(const uint8_t* take, uint32_t i) {return !take || take[i] != 0;}
// The opening of a call on the members taken: *c0 the first member taken — errors of the call as a
// whole are reported on it — or null when nobody is (nothing else done: what that means is the
// caller's); its device current; an abandoned round's launches waited for.
int group_enter(smpc_group* g, const uint8_t* take, smpc_ctx** c0);
// ONE hand-over of what a call wrote: the tick slot of every rider (`order`: member indices) and the
// argument arrays up to `extent` (at.round or at.breakdown).  CPU stores through the BAR — only the
// tick.used bytes of a slot: it is sized for the longest path, 25 KB, a tick fills ~4 — and the flush;
// else one copy of [0, extent) on the group's stream.  The caller has made sure nothing reads either.
int group_hand_over(smpc_group* g, smpc_ctx* c0, const std::vector<uint32_t>& order, size_t extent);

}  // namespace smpc_impl

#pragma GCC visibility pop

#endif  // SMPC_GROUP_H_
