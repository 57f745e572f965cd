// group_check — csrc/smpc_group_layout.h on the CPU: the layout of a group's arrays against the
// formulas it replaced (restated here, not taken from the header), and the partition of a round on
// cases whose riding order and launches are written out by hand.  No GPU and no HIP: the header is
// arithmetic.  Built with -fsanitize=address,undefined by tests/test_group_plan_cpu.py.  Exit status
// 0: every check held.
#include "../../mpcholonavigation_amd/csrc/smpc_group_layout.h"

#include <cstdio>
#include <initializer_list>

using namespace smpc_impl;

namespace {

int g_failed = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);           \
      g_failed++;                                                          \
    }                                                                      \
  } while (0)

// ---- the layout -------------------------------------------------------------------------------------
// the formulas smpc_group_create computed inline before there was a header
uint32_t up256(uint32_t v) {return (v + 255u) / 256u * 256u;}

void check_layout(size_t cap, uint32_t n)
{
  // element sizes of the kind the product has: none a divisor of 256, one above it
  const GroupElemSizes s{424, 88, 52, 120, 16, 72};
  const GroupLayout l = group_layout(cap, n, s);
  const size_t at[] = {0, l.dev, l.red, l.geo, l.mov, l.fdev, l.fgeo, l.sdst, l.sred, l.breakdown};
  const size_t need[] = {l.slot * n, s.dev * n, s.red * n, s.geo * n, s.mov * n, s.dev * n, s.geo * n, s.sdst * n, s.sred * n};
  CHECK(l.n == n);
  CHECK(l.slot % 256 == 0 && l.slot >= cap && l.slot < cap + 256);
  for (int k = 0; k < 9; ++k) {
    CHECK(at[k] % 256 == 0);
    CHECK(at[k + 1] >= at[k] + need[k]);   // ascending, room for n elements, no overlap
  }
  CHECK(l.round == l.mov + up256(static_cast<uint32_t>(s.mov) * n));   // exactly behind the moving-member array
  CHECK(l.round % 256 == 0 && l.breakdown % 256 == 0);
  for (size_t off : {l.fdev, l.fgeo, l.sdst, l.sred}) CHECK(off >= l.round && off < l.breakdown);
  CHECK(l.breakdown >= l.sred + s.sred * n);
  // the parent's values
  const size_t slot = up256(static_cast<uint32_t>(cap));
  const size_t off_dev = slot * n;
  const size_t off_red = off_dev + up256(static_cast<uint32_t>(s.dev) * n);
  const size_t off_geo = off_red + up256(static_cast<uint32_t>(s.red) * n);
  const size_t off_mov = off_geo + up256(static_cast<uint32_t>(s.geo) * n);
  const size_t total = off_mov + up256(static_cast<uint32_t>(s.mov) * n);
  const size_t off_fdev = total;
  const size_t off_fgeo = off_fdev + up256(static_cast<uint32_t>(s.dev) * n);
  const size_t off_sdst = off_fgeo + up256(static_cast<uint32_t>(s.geo) * n);
  const size_t off_sred = off_sdst + up256(static_cast<uint32_t>(s.sdst) * n);
  const size_t total_stats = off_sred + up256(static_cast<uint32_t>(s.sred) * n);
  CHECK(l.slot == slot && l.dev == off_dev && l.red == off_red && l.geo == off_geo && l.mov == off_mov && l.round == total);
  CHECK(l.fdev == off_fdev && l.fgeo == off_fgeo && l.sdst == off_sdst && l.sred == off_sred && l.breakdown == total_stats);
}

// ---- the partition ----------------------------------------------------------------------------------
const char kInst[4] = {};   // four instance keys: only their addresses matter
const void* const LA = &kInst[0];
const void* const LB = &kInst[1];
const void* const WA = &kInst[2];
const void* const WB = &kInst[3];

constexpr uint32_t kT = 56, kLimit = 160 * 1024;
// a stand-in for lane_lds(...).total that grows with the path length as the real one does
uint32_t lds_of(uint32_t window_bytes, uint32_t Pmax, uint32_t T) {return window_bytes + 16 * Pmax + 12 * T;}

GroupMemberPlan lane_member(const void* inst, uint32_t P, uint32_t grid, uint32_t window = 9216, uint32_t block = 512,
                            bool obst = true, bool dep = false)
{
  GroupMemberPlan m;
  m.taken = m.eligible = m.lane = true;
  m.inst = inst;
  m.P = P; m.grid = grid; m.window_bytes = window; m.block = block; m.obst = obst; m.dep = dep;
  return m;
}
GroupMemberPlan wave_member(const void* inst, uint32_t grid, uint32_t lds)
{
  GroupMemberPlan m;
  m.taken = m.eligible = true;
  m.inst = inst;
  m.grid = grid; m.lds = lds;
  return m;
}
GroupMemberPlan untaken()
{
  // everything else set as if it rode: a member not taken is never looked at
  GroupMemberPlan m = lane_member(LB, 4000, 4000, 1, 1, false, true);
  m.taken = false;
  return m;
}

GroupPartition run(const std::vector<GroupMemberPlan>& mem)
{
  return group_partition(mem.data(), static_cast<uint32_t>(mem.size()), kT, lds_of, kLimit);
}
bool same(const GroupLaunch& l, const void* inst, bool lane, uint32_t first, uint32_t count, uint32_t grid, uint32_t lds)
{
  return l.inst == inst && l.lane == lane && l.first == first && l.count == count && l.grid == grid && l.lds == lds;
}
typedef std::vector<uint32_t> Order;

void check_partition()
{
  {  // a: nobody eligible
    std::vector<GroupMemberPlan> mem{lane_member(LA, 10, 8), wave_member(WA, 4, 100), wave_member(WA, 4, 100)};
    for (GroupMemberPlan& m : mem) m.eligible = false;
    const GroupPartition p = run(mem);
    CHECK(p.order.empty() && p.launches.empty() && p.lane.first == 3);
  }
  {  // b: three lane members that agree
    const GroupPartition p = run({lane_member(LA, 10, 8), lane_member(LA, 40, 6), lane_member(LA, 25, 12)});
    CHECK(p.order == (Order{0, 1, 2}));
    CHECK(p.launches.size() == 1 && same(p.launches[0], LA, true, 0, 3, 12, lds_of(9216, 40, kT)));
    CHECK(p.lane.inst == LA && p.lane.Pmax == 40 && p.lane.grid == 12 && p.lane.block == 512 && p.lane.window_bytes == 9216 &&
          p.lane.first == 0);
  }
  {  // c: one lane member only: a launch of count 1
    const GroupPartition p = run({wave_member(nullptr, 4, 100), lane_member(LA, 10, 8)});
    CHECK(p.order == (Order{1}));
    CHECK(p.launches.size() == 1 && same(p.launches[0], LA, true, 0, 1, 8, lds_of(9216, 10, kT)));
    CHECK(p.lane.first == 1);
  }
  {  // d: two window sizes (and, likewise, two blocks, or a row that scores no costmap lookup)
    GroupPartition p = run({lane_member(LA, 10, 8), lane_member(LA, 10, 8, 20736), lane_member(LA, 10, 8)});
    CHECK(p.order.empty() && p.launches.empty());
    p = run({lane_member(LA, 10, 8), lane_member(LA, 10, 8, 9216, 1024)});
    CHECK(p.order.empty() && p.launches.empty());
    p = run({lane_member(LA, 10, 8), lane_member(LB, 10, 8, 9216, 512, false)});
    CHECK(p.order.empty() && p.launches.empty());
    // ... and the wave members beside them still ride
    p = run({lane_member(LA, 10, 8), wave_member(WA, 4, 100), lane_member(LA, 10, 8, 20736), wave_member(WA, 5, 90)});
    CHECK(p.order == (Order{1, 3}));
    CHECK(p.launches.size() == 1 && same(p.launches[0], WA, false, 0, 2, 5, 100));
  }
  {  // e: Pmax past the LDS limit
    const uint32_t P_over = (kLimit - 9216 - 12 * kT) / 16 + 1;
    CHECK(lds_of(9216, P_over, kT) > kLimit && lds_of(9216, P_over - 1, kT) <= kLimit);
    GroupPartition p = run({lane_member(LA, 10, 8), lane_member(LA, P_over, 8)});
    CHECK(p.order.empty() && p.launches.empty());
    p = run({lane_member(LA, 10, 8), lane_member(LA, P_over - 1, 8)});   // at the limit: rides
    CHECK(p.order == (Order{0, 1}) && p.launches.size() == 1);
  }
  {  // f: wave members on instances A, B, A, B
    const GroupPartition p = run({wave_member(WA, 4, 100), wave_member(WB, 9, 300), wave_member(WA, 7, 80), wave_member(WB, 3, 350)});
    CHECK(p.order == (Order{0, 2, 1, 3}));
    CHECK(p.launches.size() == 2 && same(p.launches[0], WA, false, 0, 2, 7, 100) && same(p.launches[1], WB, false, 2, 2, 9, 350));
    CHECK(p.lane.first == 4);
  }
  {  // g: a wave instance with one member
    GroupPartition p = run({wave_member(WA, 4, 100)});
    CHECK(p.order.empty() && p.launches.empty());
    p = run({wave_member(WA, 4, 100), wave_member(WB, 9, 300), wave_member(WA, 7, 80)});   // B alone between two of A
    CHECK(p.order == (Order{0, 2}));
    CHECK(p.launches.size() == 1 && same(p.launches[0], WA, false, 0, 2, 7, 100));
  }
  {  // h: lane and wave mixed, members not taken in between
    const GroupPartition p = run({wave_member(WA, 4, 100), untaken(), lane_member(LA, 10, 8), wave_member(WA, 6, 120), untaken(),
                                  lane_member(LA, 30, 5), wave_member(nullptr, 50, 5000)});
    CHECK(p.order == (Order{2, 5, 0, 3}));
    CHECK(p.launches.size() == 2 && same(p.launches[0], LA, true, 0, 2, 8, lds_of(9216, 30, kT)) &&
          same(p.launches[1], WA, false, 2, 2, 6, 120));
    CHECK(p.lane.first == 2 && p.lane.Pmax == 30 && p.lane.grid == 8);
  }
  {  // i: `dep` on the second of three lane members, then on none
    GroupPartition p = run({lane_member(LA, 10, 8), lane_member(LB, 10, 8, 9216, 512, true, true), lane_member(LA, 10, 8)});
    CHECK(p.lane.inst == LB && p.launches.size() == 1 && p.launches[0].inst == LB && p.order == (Order{0, 1, 2}));
    p = run({lane_member(LA, 10, 8), lane_member(LB, 10, 8), lane_member(LA, 10, 8)});
    CHECK(p.lane.inst == LA && p.launches.size() == 1 && p.launches[0].inst == LA && p.order == (Order{0, 1, 2}));
    // (two rows with dep: the last one)
    p = run({lane_member(LA, 10, 8, 9216, 512, true, true), lane_member(LA, 10, 8), lane_member(LB, 10, 8, 9216, 512, true, true)});
    CHECK(p.lane.inst == LB);
  }
}

}  // namespace

int main()
{
  for (uint32_t n : {1u, 2u, 16u, 37u})
    for (size_t cap : {static_cast<size_t>(25088), static_cast<size_t>(25104)}) check_layout(cap, n);   // 98 x 256; 16 more
  check_partition();
  if (g_failed) fprintf(stderr, "group_check: %d checks failed\n", g_failed);
  return g_failed ? 1 : 0;
}
