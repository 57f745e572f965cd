// smpc_group.h — the group object behind smpc_group_* (include/smpc.h), shared by smpc_group.cpp
// (rounds of ticks) and smpc_stats.cpp (smpc_group_critic_breakdown).  Internal: not part of the
// C-ABI.
#ifndef SMPC_GROUP_H_
#define SMPC_GROUP_H_

#include "smpc_ctx.h"

#pragma GCC visibility push(hidden)

extern "C" {

struct smpc_group {
  std::vector<smpc_ctx*> ctxs;
  std::vector<hipStream_t> saved_stream;
  // n tick blocks, then SmpcDev[n], SmpcReduceArgs[n], SmpcWaveGeom[n], SmpcMovingMember[n].  While the group stands, each
  // member's tick views (smpc_ctx.h: TickBlock) point at its slot of the two; the group owns them
  smpc_impl::PinnedBuf<uint8_t> h_all;
  smpc_impl::DevBuf<uint8_t> d_all;
  size_t slot = 0, off_dev = 0, off_red = 0, off_geo = 0, off_mov = 0, total = 0;
  hipStream_t stream = nullptr;   // the first member's own stream: not the group's to destroy
  uint64_t batched_ticks = 0, single_ticks = 0;
  uint64_t batched_launches = 0;   // scoring launches that carried two or more members (smpc_group_stats)
  // a batched launch went out and not every riding member's fetch_out has returned since: a round
  // abandoned on an error leaves it set, and the next round waits for the stream before it writes
  // h_all / d_all again
  bool launched = false;
  // ---- moving obstacles (smpc_group_set_moving_obstacles; the grouped launch of a round) ----
  // the members' tables back to back: ONE device allocation (n x the capacity of a member's own), ONE
  // upload on the group's stream and the event behind it.  The staging buffer comes in two copies
  // that take turns: a call packs into the one the last upload did not read, and carries the tables
  // of the members it does not take over from the other (mov_at / mov_used: where a member's table
  // stands, in floats).  The members' table views (smpc_ctx.h: MovingObstacles) point into mov_tab.
  smpc_impl::Event mov_ev_up;
  smpc_impl::PinnedBuf<float> mov_stage[2];
  int mov_cur = 0;                          // the staging copy the last upload read
  smpc_impl::DevBuf<float> mov_tab;
  std::vector<size_t> mov_at, mov_used;
  bool mov_up_recorded = false;
  uint64_t moving_launches = 0, moving_uploads = 0;   // smpc_debug_group_moving_launches
  bool moving_per_member = false;   // smpc_debug_group_moving_per_member: use_moving_seed per rider, no grouped launch
  // ---- smpc_group_critic_breakdown (smpc_stats.cpp) ----
  // further argument arrays in h_all / d_all, behind `total` (a round never uploads them): the
  // pre-pass's parameter blocks and geometry, the members' rows, the reduction's arguments
  size_t off_fdev = 0, off_fgeo = 0, off_sdst = 0, off_sred = 0, total_stats = 0;
  // the members' float regions in ONE allocation (GroupStatsArena in smpc_stats.cpp), sized at the
  // first grouped breakdown and again when the members taken or their batch sizes ask for more; the
  // reduction's double partials likewise; the results' pinned landing place
  smpc_impl::DevBuf<float> d_stats;
  smpc_impl::DevBuf<double> d_stats_part;
  smpc_impl::PinnedBuf<float> h_stats_out;
  bool stats_lds_set = false;
  uint64_t breakdown_batched = 0, breakdown_single = 0;   // member-breakdowns by route (smpc_group_breakdown_counts)
};

}  // extern "C"

#pragma GCC visibility pop

#endif  // SMPC_GROUP_H_
