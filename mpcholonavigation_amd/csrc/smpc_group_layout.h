// smpc_group_layout.h — the two pieces of an smpc_group that are pure arithmetic: where its arrays
// stand in the group's one pinned and one device allocation (GroupLayout), and which members of a
// round ride which launch (group_partition).  No HIP call, no smpc_ctx: a plain C++ compiler builds
// it (tests/group_check).  Internal: not part of the C-ABI.
#ifndef SMPC_GROUP_LAYOUT_H_
#define SMPC_GROUP_LAYOUT_H_

#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

// not part of the C-ABI: what the compiler does not inline stays out of the dynamic symbol table
#pragma GCC visibility push(hidden)

namespace smpc_impl {

// ---- the layout -----------------------------------------------------------------------------------
// Offsets in bytes from the start of h_all and of d_all alike, every one a multiple of 256:
//   n tick slots of `slot` bytes                                    index: the MEMBER, i
//   SmpcDev[n], SmpcReduceArgs[n], SmpcWaveGeom[n], SmpcMovingMember[n]   index: the RIDER position, j
//     — up to `round`: what a round hands over
//   SmpcDev[n], SmpcWaveGeom[n] (the furthest-point pre-pass), SmpcStatsDst[n], SmpcStatsReduceArgs[n]
//     — up to `breakdown`: what smpc_group_critic_breakdown hands over (a round never uploads them)
// The typed views are GroupArrays' (smpc_group.h); this is only where they start.
struct GroupElemSizes {
  size_t dev, red, geo, mov, sdst, sred;   // sizeof SmpcDev, SmpcReduceArgs, SmpcWaveGeom, SmpcMovingMember, SmpcStatsDst, SmpcStatsReduceArgs
};
struct GroupLayout {
  uint32_t n = 0;
  size_t slot = 0;
  size_t dev = 0, red = 0, geo = 0, mov = 0;
  size_t round = 0;       // extent of a round's upload: [0, round)
  size_t fdev = 0, fgeo = 0, sdst = 0, sred = 0;
  size_t breakdown = 0;   // extent of a breakdown's upload, and of the two allocations: [0, breakdown)
};
inline size_t group_align(size_t bytes) {return (bytes + 255) / 256 * 256;}
inline GroupLayout group_layout(size_t slot_cap, uint32_t n, const GroupElemSizes& s)
{
  GroupLayout l;
  l.n = n;
  l.slot = group_align(slot_cap);
  l.dev = l.slot * n;
  l.red = l.dev + group_align(s.dev * n);
  l.geo = l.red + group_align(s.red * n);
  l.mov = l.geo + group_align(s.geo * n);
  l.round = l.mov + group_align(s.mov * n);
  l.fdev = l.round;
  l.fgeo = l.fdev + group_align(s.dev * n);
  l.sdst = l.fgeo + group_align(s.geo * n);
  l.sred = l.sdst + group_align(s.sdst * n);
  l.breakdown = l.sred + group_align(s.sred * n);
  return l;
}

// ---- the partition of a round ---------------------------------------------------------------------
// One member as the partition sees it.  `inst`: the row of the grouped instance its own plan asks for
// (a LaneInst for a lane member, a WaveInst for a wave member; compared, never read); null: no grouped
// instance, ticked alone.
struct GroupMemberPlan {
  bool taken = false;      // not taken: never looked at
  bool eligible = false;   // may ride a batched launch at all
  bool lane = false;       // rides the lane launch (else: the wave launch of `inst`)
  const void* inst = nullptr;
  uint32_t grid = 0;       // of its own launch of that pass
  // a lane member
  uint32_t window_bytes = 0, block = 0, P = 0;
  bool obst = false, dep = false;   // of its LaneInst row
  // a wave member
  uint32_t lds = 0;        // its own launch's LDS total
};
// riders [first, first + count) of `order` in one launch of `inst`, on the maxima of their grids and LDS
struct GroupLaunch {
  const void* inst;
  bool lane;
  uint32_t first, count, grid, lds;
};
// what the lane members have in common (first == n: there is none)
struct GroupLaneCommon {
  const void* inst = nullptr;
  uint32_t Pmax = 0, grid = 0, block = 0, window_bytes = 0, first = 0;
};
struct GroupPartition {
  std::vector<uint32_t> order;         // the riders, by member index: order[j] is rider j
  std::vector<GroupLaunch> launches;
  GroupLaneCommon lane;
};
// LDS bytes of a lane launch (lane_lds(...).total, smpc_prepare.cpp), handed in so that this file stays alone
typedef uint32_t (*GroupLaneLds)(uint32_t window_bytes, uint32_t Pmax, uint32_t T);

// The rules:
//   * order: the lane members first, in member order; then the wave instances by first appearance,
//     the members of each in member order;
//   * the lane launch exists with ONE rider too (whether it counts as batched is the caller's);
//   * lane members that disagree on the window, the block or `obst`, or whose launch would need more
//     LDS than lds_limit, are all ticked alone: no lane launch, none of them in `order`;
//   * the lane instance is the first lane member's row, unless a later member's row has `dep`: the
//     last such row wins;
//   * a wave instance that only one member chose gets no launch: that member is ticked alone.
inline GroupPartition group_partition(const GroupMemberPlan* mem, uint32_t n, uint32_t T, GroupLaneLds lane_lds_total,
                                      uint32_t lds_limit)
{
  GroupPartition p;
  GroupLaneCommon& lane = p.lane;
  lane.first = n;
  auto rides = [&](uint32_t i) {return mem[i].taken && mem[i].eligible && mem[i].inst;};
  bool lane_ok = true, inst_obst = false;
  for (uint32_t i = 0; i < n; ++i) {
    const GroupMemberPlan& m = mem[i];
    if (!rides(i) || !m.lane) continue;
    if (lane.first == n) {
      lane.first = i;
      lane.window_bytes = m.window_bytes;
      lane.block = m.block;
    }
    else if (m.window_bytes != lane.window_bytes || m.obst != inst_obst || m.block != lane.block)
      lane_ok = false;
    if (!lane.inst || m.dep) {
      lane.inst = m.inst;
      inst_obst = m.obst;
    }
    lane.Pmax = std::max(lane.Pmax, m.P);
    lane.grid = std::max(lane.grid, m.grid);
  }
  if (lane.first != n) {
    const uint32_t lds = lane_lds_total(lane.window_bytes, lane.Pmax, T);
    if (lds > lds_limit) lane_ok = false;
    if (lane_ok) {
      for (uint32_t i = 0; i < n; ++i)
        if (rides(i) && mem[i].lane) p.order.push_back(i);
      p.launches.push_back({lane.inst, true, 0, static_cast<uint32_t>(p.order.size()), lane.grid, lds});
    }
  }
  for (uint32_t i = 0; i < n; ++i) {
    if (!rides(i) || mem[i].lane) continue;
    bool seen = false;
    for (const GroupLaunch& l : p.launches) seen = seen || (!l.lane && l.inst == mem[i].inst);
    if (seen) continue;
    GroupLaunch l{mem[i].inst, false, static_cast<uint32_t>(p.order.size()), 0, 0, 0};
    for (uint32_t j = i; j < n; ++j) {
      if (!rides(j) || mem[j].lane || mem[j].inst != mem[i].inst) continue;
      p.order.push_back(j);
      l.count++;
      l.grid = std::max(l.grid, mem[j].grid);
      l.lds = std::max(l.lds, mem[j].lds);
    }
    if (l.count >= 2) p.launches.push_back(l);
    else p.order.pop_back();   // alone on its instance: ticked alone
  }
  return p;
}

}  // namespace smpc_impl

#pragma GCC visibility pop

#endif  // SMPC_GROUP_LAYOUT_H_
