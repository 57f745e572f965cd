// smpc_ctx.h — what the translation units behind include/smpc.h share: the context object,
// the launchers of the .hip files, and the host-side helpers (smpc_impl).  Internal: not part of
// the C-ABI.
//   smpc_api.cpp          lifecycle, setters, the costmap, the single-GPU tick (smpc_optimize), launch helpers
//   smpc_noise.cpp        the stored noise: smpc_set_noise, the device RNG's draws, the background redraw
//   smpc_limit_host.cpp   acceleration limits: the setters and the limiter's launch (use_limited_noise)
//   smpc_moving_host.cpp  moving obstacles: the table's upload and the seed kernel's launch (use_moving_seed)
//   smpc_validate_host.cpp  the trajectory validator: smpc_validate_trajectory and the group's one call
//   smpc_debug.cpp        the smpc_selftest_* and smpc_debug_* entries (include/smpc_debug.h)
//   smpc_prepare.cpp      per-tick host work: gates, path tables, lookup tables, LDS carve-up
//   smpc_shard.cpp        batch-sharded tick, RCCL resolved at run time
//   smpc_group.cpp        several planning instances per launch (the group object: smpc_group.h; where its
//                         arrays stand and who rides which launch: smpc_group_layout.h)
//   smpc_stats.cpp        per-critic breakdown of a tick (smpc_critic_breakdown) and of a group's
//                         members (smpc_group_critic_breakdown)
// What they allocate is held by the holders of smpc_own.h, as members of the context's parts below.
#ifndef SMPC_CTX_H_
#define SMPC_CTX_H_

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>   // types only: RCCL itself is resolved at run time (dlopen)
#include <dlfcn.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <new>
#include <string>
#include <vector>

#include "../../include/smpc.h"
#include "smpc_dev.h"
#include "smpc_inst.h"   // the scoring-pass instances: tables, selectors, launch
#include "smpc_limit.h"  // smpc_limit_noise: its arguments
#include "smpc_moving.h" // smpc_moving_cost: its arguments
#include "smpc_validate.h" // smpc_validate: its arguments
#include "smpc_own.h"    // DevBuf, PinnedBuf, Event, Stream

// nothing below is part of the C-ABI: keep it out of the dynamic symbol table
#pragma GCC visibility push(hidden)

hipError_t smpc_launch_reduce(const float* partials, uint32_t nblk, uint32_t T,
                              float neg_inv_temp, float* tuple, const SmpcFinal& fin,
                              hipStream_t st);
hipError_t smpc_launch_combine(const float* tuples, uint32_t G, uint32_t T, float neg_inv_temp,
                               float vx_max, float vx_min, float vy_max, float wz_max,
                               float* u_out, float* result, const float* furthest_used,
                               float* host_out, uint32_t seq, hipStream_t st);
hipError_t smpc_launch_fill_noise(float* out, uint64_t n, uint64_t base, uint64_t seed,
                                  uint32_t stream, uint32_t epoch, float sigma, hipStream_t st);
hipError_t smpc_launch_fill_noise_tm(float* dst, uint32_t B, uint32_t T, uint64_t base, uint64_t seed,
                                     uint32_t stream, uint32_t epoch, float sigma, hipStream_t st);
hipError_t smpc_launch_ackermann(float* u_dev, float* u_host, uint32_t T, float min_r, uint32_t seq,
                                 hipStream_t st);
hipError_t smpc_launch_p2p_exchange(const float* my_tuple, const SmpcP2P& x, uint32_t T, int mode,
                                    float* d_furthest, float neg_inv_temp, float vx_max, float vx_min,
                                    float vy_max, float wz_max, float* u_out, float* result,
                                    const float* furthest_used, float* host_out, uint32_t seq,
                                    hipStream_t st);

hipError_t smpc_launch_relayout(const float* src, float* dst, uint32_t B, uint32_t T, bool to_gm, hipStream_t st);
uint32_t smpc_lane_block();
uint32_t smpc_lane_block_rr();
hipError_t smpc_launch_lane_reduce(const float* v, const float* w, float* out, hipStream_t st);
// smpc_split.hip: lane = (rollout, quarter of the horizon), for batches of at most one round of waves
hipError_t smpc_launch_row_reduce(const float* v, float* out, uint32_t n, hipStream_t st);
uint32_t smpc_split_block();
uint32_t smpc_split_rollouts_per_block(uint32_t nseg);
hipError_t smpc_launch_reduce_many(const SmpcReduceArgs* d_many, uint32_t n, uint32_t T, hipStream_t st);
hipError_t smpc_launch_sincos(const float* x, uint32_t n, float* sn, float* cs, hipStream_t st);
hipError_t smpc_launch_philox(const uint32_t* ctr, uint32_t k0, uint32_t k1, uint32_t n, uint32_t* out,
                              hipStream_t st);
hipError_t smpc_launch_box_muller(const uint32_t* r0, const uint32_t* r1, uint32_t n, float* z0, float* z1,
                                  hipStream_t st);

// smpc_limit.hip: the stored noise of an iteration into its limited noise, in either layout
hipError_t smpc_launch_limit_noise(const SmpcLimitArgs& a, bool group_major, hipStream_t st);
// smpc_moving.hip: the moving-obstacle term of an iteration into the passes' starting costs, from either layout
hipError_t smpc_launch_moving_cost(const SmpcMovingArgs& a, bool group_major, hipStream_t st);
// smpc_moving_many.hip: the same for `count` members of a group that take one form, in one launch
hipError_t smpc_launch_moving_cost_many(const SmpcMovingMember* d_many, uint32_t count, uint32_t grid, SmpcMovingForm form,
                                        uint32_t T, hipStream_t st);
// smpc_validate.hip: the collision check of `count` control sequences' trajectories, a block each
hipError_t smpc_launch_validate(const SmpcValidateArgs* d_many, uint32_t count, hipStream_t st);

namespace smpc_impl {

extern thread_local std::string g_create_error;


// RCCL entry points, resolved once.  The library is not a link-time dependency: a process
// that already holds RCCL (torch.distributed's "nccl" backend IS RCCL on ROCm) shares that
// copy, a single-GPU user never loads it.
struct RcclApi {
  ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
  ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
  ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
  ncclResult_t (*AllGather)(const void*, void*, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*AllReduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t,
                            hipStream_t) = nullptr;
  const char* (*GetErrorString)(ncclResult_t) = nullptr;
};
const RcclApi* rccl();   // smpc_shard.cpp; null when RCCL cannot be loaded

// threads per block of the streaming pass: 16 waves share one costmap window and produce one
// partial (fewer partials to reduce); T > 128 needs more registers per lane than 16 waves allow
inline uint32_t pass_block(int R) {return R == 4 ? 512u : 1024u;}
constexpr uint32_t kLaneMinBatch = 60u * 1024u;   // lane-per-rollout pass from this batch size up (measured crossover ~50k: 65 536 x 64 takes 35.9 us against 40.4 us)
constexpr uint32_t kSplitMinBatch = 12u * 1024u;  // smpc_pass_split (T = 64) from this batch size up to one group per wave (measured: 16 384 x 64
                                                  // 38.9 -> 36.2 us per tick, 32 768: 44.7 -> 36.7; 4 096: no gain)
constexpr uint32_t kSplitMinBatchShort = 20000u;  // the same for 36 <= T < 64 (idle step slots are masked, not skipped)
constexpr uint32_t kLaneMaxT = 128;       // T <= 64: 3 x 64 noised controls parked per lane (or re-read); T <= 128: re-read
constexpr uint32_t kPollWords = SMPC_BLOCK_DONE_WORDS;   // completion words from slot SMPC_R_BLOCK_DONE of h_out on: room for
                                                         // smpc_reduce_blocks(T) of them (T = 64: 7, T = 128: 13, T = 256: 25)
static_assert(SMPC_TUPLE_HEADER == SMPC_R_F_USED, "the shard tuple's header is the first four result slots, in their order");
constexpr uint32_t kMaxGrid = SMPC_MAX_GRID;   // smpc_reduce_partials stages this many factors
constexpr uint32_t kWindowBytes = 96 * 96;  // costmap window staged in LDS: 4.8 m x 4.8 m at
                                           // 0.05 m around the robot; the rest is read from HBM/L2
constexpr uint32_t kWindowSideMax = 144;       // T > 64: up to 144 x 144 cells (20 KB, +-3.6 m at 0.05 m: measured optimum, smpc_prepare.cpp)
constexpr uint32_t kLdsPerCu = 160 * 1024;

inline uint32_t align_up(uint32_t v, uint32_t a) {return (v + a - 1) / a * a;}

struct HostCostmap {
  PinnedBuf<uint8_t> cells;   // pinned mirror of the device copy: the host-side lookups read it
                              // (path validity, first rollout point) and uploads DMA out of it
  uint32_t W = 0, H = 0;
  double ox = 0, oy = 0, res = 1;
  bool track_unknown = false;
  float inscribed_radius = 0, cost_scaling_factor = 0, inflation_radius = 0;
  bool set = false;
};

// Costmap2D::worldToMap (nav2_costmap_2d, Humble); call sites tools/utils.hpp:365-372
inline bool world_to_map(const HostCostmap& c, double wx, double wy, unsigned& mx, unsigned& my)
{
  if (wx < c.ox || wy < c.oy) return false;
  const double qx = (wx - c.ox) / c.res, qy = (wy - c.oy) / c.res;
  if (!(qx < 4294967296.0) || !(qy < 4294967296.0)) return false;
  mx = static_cast<unsigned>(qx);
  my = static_cast<unsigned>(qy);
  return mx < c.W && my < c.H;
}

// utils::withinPositionGoalTolerance(float, Pose, Pose) (tools/utils.hpp:233-249)
inline bool within_tol(float tol, double rx, double ry, double gx, double gy)
{
  const double dist_sq = std::pow(gx - rx, 2) + std::pow(gy - ry, 2);
  const float tol_sq = tol * tol;
  return dist_sq < tol_sq;
}

// Developer knobs: read from the environment once, when the context is created (read_knobs,
// smpc_api.cpp), never per tick.  Experiments and tests; the defaults are the product.
struct Knobs {
  enum Pass {kAuto, kWave, kLane, kSplit} pass = kAuto;   // SMPC_PASS=wave|lane|split: the streaming pass, whatever the batch
  bool no_split = false;           // SMPC_NO_SPLIT=1
  uint32_t split_nseg = 0;         // SMPC_SPLIT_NSEG=2|4
  bool lane_reread = false;        // SMPC_LANE_REREAD=1: the re-read form for T = 64 too
  bool half_blocks = true;         // SMPC_NO_HALF_BLOCKS=1 turns it off
  uint32_t max_blocks_per_cu = 0;  // SMPC_MAX_BLOCKS_PER_CU
  bool balanced_grid = true;       // SMPC_NO_BALANCED_GRID=1 turns it off: re-read form, launch only the waves that fill every round
  bool fused_reduce = false;       // SMPC_FUSED_REDUCE=1: smpc_grid_tail reduces inside the scoring launch (an experiment
                                   // that measured no faster than the separate launch: DESIGN.md 4.3)
  bool no_inline_tick = false;     // SMPC_NO_INLINE_TICK
  bool pinned_tick = false;        // SMPC_PINNED_TICK=1: kernels read the tick block from pinned host memory
  bool poll = true;                // SMPC_NO_POLL=1 disables completion polling on the host-mapped result
  bool bar_tick = true;            // SMPC_NO_BAR_TICK=1: the per-tick upload as a copy on the stream
  bool hdp_flush = true;           // SMPC_NO_HDP_FLUSH=1: the BAR stores without the flush (the canary then guards every tick)
  bool repeat_pass = false;        // SMPC_DEBUG_REPEAT_PASS=1 (tests): every iteration's scoring pass is launched twice
  uint32_t stale_tick = 0;         // SMPC_DEBUG_STALE_TICK=n (tests): the BAR hand-over skips tick n's block
  bool small_window = false;       // SMPC_SMALL_WINDOW: the 96-cell costmap window for T > 64 too
  int window_side_max = -1;        // SMPC_WINDOW_SIDE_MAX=cells, < 0: kWindowSideMax
  bool furthest_prune = true;      // SMPC_FURTHEST_PRUNE=0: the lane pass's prune table is written empty (every entry "never
                                   // prune"): same kernel, every group scans — the A/B switch and the tests' unpruned answer
  bool footprint_general = false;  // SMPC_FOOTPRINT_PASS=general: consider_footprint ticks keep the general pass (MODE 2)
                                   // instead of the lean MODE 4 — to measure the two routes in one process, and a way back
  bool nonholo_omni = false;       // SMPC_NONHOLO_PASS=omni: DiffDrive and Ackermann ticks keep the Omni-form lane rows (the
                                   // zero vy stream read and carried along) instead of smpc_pass_lane_nh — to measure the
                                   // two routes in one process, and a way back
};

// blocks per CU of the instance asked about last (the answer moves with the LDS a tick needs)
struct OccCache {
  const void* fn = nullptr;
  uint32_t block = 0, lds = 0;
  uint32_t blocks = 1;
  uint32_t get(const void* f, uint32_t blk, uint32_t lds_bytes)
  {
    if (f != fn || blk != block || lds_bytes != lds) {
      int nb = 0;
      if (inst_occupancy(f, blk, lds_bytes, &nb) != hipSuccess || nb < 1) nb = 1;
      fn = f; block = blk; lds = lds_bytes;
      blocks = static_cast<uint32_t>(nb);
    }
    return blocks;
  }
};

// Which scoring pass takes the tick, and its launch geometry.  Written by plan_launch
// (smpc_prepare.cpp) only; pass_for (smpc_api.cpp) picks the instance for a pass's flags from it.
struct PassGeom {
  uint32_t grid = 0, block = 0;
  SmpcLds lds{};
};
struct PassPlan {
  enum Kind : uint32_t {kWave = 0, kLane = 1, kSplit = 2};   // (the values of smpc_tick_out.pass_kind)
  Kind kind = kWave;
  PassGeom wave;              // planned for every tick: a pass whose flags have no lane instance falls back to it
  PassGeom lane;              // kind != kWave (a split tick whose flags were stripped takes the lane pass)
  PassGeom split;             // kind == kSplit
  bool rr = false;            // the lane pass in its re-read form (no parked controls; T > 64 or SMPC_LANE_REREAD=1)
  bool pow = false;           // the lane pass scores with cost powers other than 1: the rows of smpc_pass_lane_pow
  bool nh = false;            // the lane pass of a non-holonomic model without the vy stream: the rows of smpc_pass_lane_nh
  uint32_t split_nseg = 4;    // lanes per rollout of the split pass: 4 or 2
  uint32_t window_bytes = 0;  // first LDS region of the lane pass
};

// The furthest-point predictor: everything remember_furthest and predict_hint (smpc_prepare.cpp) own.
// Who else writes it: smpc_reset (forget), a sharded tick whose exchange timed out (drop_hint), the
// sharded tick and the group after a miss (hint, hint_F, hint_is_this_ticks); smpc_critic_breakdown
// saves and restores it whole.
struct FurthestPredictor {
  // the index this tick is scored with first (predict_hint: last tick's value carried forward by the
  // robot's motion and the plan's shift)
  bool hint_valid = false;
  uint32_t hint = 0;
  // what the prediction starts from: the last known F = index + fraction (smpc_dev.h) and the
  // tick inputs it was measured on
  float hint_F = 0.f;
  float hint_Fp = 0.f;       // the last prediction, unrounded; valid when hint_Fp_valid
  bool hint_Fp_valid = false;
  bool hint_is_this_ticks = false;   // set by the group's re-run of a missed member (predict_hint)
  float hint_drift = 0.f;    // last tick's (true - predicted): how fast the endpoints drift relative to the robot
  bool anchor_valid = false;
  double anchor_x = 0, anchor_y = 0;
  // endpoint of the NOMINAL rollout (the control sequence a tick starts from, no noise) of the last
  // remembered tick and of the tick at hand: what carries the furthest point from tick to tick
  double anchor_ex = 0, anchor_ey = 0, cur_ex = 0, cur_ey = 0;
  bool anchor_e_valid = false, cur_e_valid = false;
  std::vector<float> anchor_px, anchor_py;
  uint32_t noise_gen_remembered = 0;   // NoiseStore::noise_gen as of the last remember_furthest
  // smpc_reset: no prediction and no drift; the anchor stays (unread while hint_valid is false, and
  // the next remember_furthest overwrites it)
  void forget()
  {
    hint_valid = false;
    hint_Fp_valid = false;
    hint_is_this_ticks = false;
    hint_drift = 0.f;
  }
  // the tick's furthest point never became known: the next tick does not speculate
  void drop_hint() {hint_valid = false;}
};

}  // namespace smpc_impl

// ---- the context's parts.  Each owns what it allocates (smpc_own.h): a buffer is one declaration,
// and free_ctx names none of them.  In every part the events and streams stand in front of the
// buffers, so that the buffers go first when the part is destroyed. ----
namespace smpc_impl {

// One set of noise tensors: the three [B,T] tensors, and the group-major copies (smpc_dev.h:
// SMPC_GM_INDEX) for the lane-per-rollout and split passes in ONE allocation, tvx, that vy and wz
// follow (tvy and twz: views into it).
struct NoiseSet {
  DevBuf<float> nvx, nvy, nwz;
  DevBuf<float> tvx;
  float* tvy = nullptr;
  float* twz = nullptr;
};

// The stored noise.  Written by smpc_noise.cpp: smpc_set_noise, the device RNG's draws (smpc_seed,
// smpc_redraw_noise[_async], draw_noise) and absorb_redraw at the head of a tick.  Two writers in
// smpc_api.cpp: smpc_create allocates `cur` and decides use_tpr, and smpc_reset advances `epoch`
// itself before it calls draw_noise.
struct NoiseStore {
  // smpc_redraw_noise_async (regenerate_noises = true): the next epoch is drawn into `next` on
  // fill_stream while the host and the device go on; the next tick's stream waits for ev_fill and
  // the sets change places (absorb_redraw).
  Stream fill_stream;
  Event ev_fill;
  NoiseSet cur;              // what the ticks score with
  NoiseSet next;             // the background draw (allocated by the first one)
  bool redraw_pending = false, redraw_rm_valid = true;
  uint32_t noise_gen = 0;    // counts changes of the noise the ticks score with (pred.noise_gen_remembered:
                             // as of the last remember_furthest)
  bool use_tpr = false;      // group-major noise kept: the lane-per-rollout pass may run
  bool rm_valid = true;      // the [B,T] tensors hold the current noise (a device-RNG draw fills the
                             // group-major copy only; ensure_row_major() makes the other on demand)
  bool have_noise = false, rng_mode = false;
  uint64_t seed = 0;
  uint32_t epoch = 0;
};

// Acceleration limits (smpc_set_acceleration_limits).  While `on`, every pass reads
// the LIMITED noise of its iteration in place of the stored noise: use_limited_noise makes it, once
// per iteration and layout, in front of the first pass that reads that layout.  Buffers: allocated at
// the first tick that reads their layout.  Written by the functions of smpc_limit_host.cpp only;
// begin_limit_iteration is called by prepare_tick (every tick) and by smpc_optimize (iterations > 0).
// smpc_critic_breakdown runs prepare_tick and use_limited_noise like a tick and does NOT put the
// counters back: it advances `iter`, leaves `rm_iter` at it, and smpc_get_limited_noise after a
// breakdown hands out the breakdown's limited noise.
struct Limiter {
  Event ev[2];                      // SMPC_FLAG_PROFILE: around the last limiter launch
  bool on = false;
  float lim[4] = {0.f, 0.f, 0.f, 0.f};   // ax_max, ax_min, ay_max, az_max
  DevBuf<float> l_rm[3];            // [B,T] each (vy: holonomic models only)
  DevBuf<float> l_gm;               // group-major, vx | vy | wz back to back like NoiseSet::tvx (vy of a non-holonomic model: zeros)
  const float* u_dev = nullptr;     // the iteration's u on the device; null: the tick block's host copy (iteration 0)
  uint32_t iter = 0;                // counts iterations (begin_limit_iteration); never 0 once a tick ran
  uint32_t rm_iter = 0, gm_iter = 0;   // the iteration each layout's buffer holds (0: none)
};

// Moving obstacles (smpc_set_moving_obstacles).  While K > 0, every iteration's
// passes start their costs from the moving-obstacle term: use_moving_seed launches smpc_moving_cost
// once per iteration, in front of the first pass, into the buffer the passes read as costs_prev.
// Buffers: allocated by the first smpc_set_moving_obstacles with n > 0, each on its own.  Written by
// the functions of smpc_moving_host.cpp only.  smpc_critic_breakdown seeds through seed_own_costs,
// which writes stats_seed and leaves iter, scored, m and hit alone: they stay the last tick's.
// `tk` / `tab_kt` / `disc` are the VIEWS the launches read (like TickBlock's): into the context's own
// allocation tab_tk, or — after smpc_group_set_moving_obstacles, `group_table` — into the group's
// (smpc_group.cpp: the group owns that table; smpc_group_destroy switches the term off).
struct MovingObstacles {
  Event ev_up;                      // behind the last upload
  Event ev[2];                      // SMPC_FLAG_PROFILE: around the last smpc_moving_cost launch
  uint32_t K = 0;                   // discs in the table; 0: off
  smpc_moving_obstacles_params par{};
  DevBuf<float> tab_tk;             // [T][K]{x, y, guarded squared reach, radius}: the group-major launch's table;
                                    // the ONE device allocation of the ctx's own table
  float* tk = nullptr;              // the [T][K] table in use: tab_tk, or a region of a group's allocation
  float* tab_kt = nullptr;          // [K][T]{x, y}: the row-major launch's
  float* disc = nullptr;            // [K]{radius, radius + margin, guarded squared reach, 0}
  PinnedBuf<float> stage;           // the same three regions, what the uploads read
  bool up_recorded = false;
  hipStream_t up_stream = nullptr;  // the stream it went out on (a kernel on another stream waits for the event)
  bool group_table = false;         // the views point into a group's allocation, uploaded on the group's stream
  DevBuf<float> m;                  // [B] m of the last scored iteration
  DevBuf<uint8_t> hit;              // [B] its hits
  DevBuf<float> stats_seed;         // [B] the seed of smpc_critic_breakdown's own cost buffer (first use)
  uint32_t iter = 0;                // the iteration (Limiter::iter) whose seed is in place (0: none)
  bool scored = false;              // m and hit hold a tick's values
};

// The batch-sharded tick's links to the other shards.  Written by smpc_shard.cpp only.
struct ShardLink {
  // native RCCL exchange (smpc_shard_tick)
  ncclComm_t comm = nullptr;
  int comm_rank = 0, comm_world = 0;
  DevBuf<float> d_all;         // [world][SMPC_TUPLE_HEADER + 3T] gathered shard tuples
  // collective-free exchange (smpc_shard_p2p_*): the own mailbox (fine-grained device memory,
  // exported over IPC) and the peers' mailboxes as mapped into this process (free_ctx unmaps them)
  DevBuf<float> p2p_mailbox;
  SmpcP2P p2p{};               // world == 0: not set up
  uint32_t p2p_xseq = 0;
  uint32_t p2p_timeout_ms = 10000;   // bound of the in-kernel wait for the peers (smpc_shard_p2p_set_timeout)
  bool p2p_failed = false;           // an exchange timed out: no further mailbox tick until re-init
  smpc_tick_in step_in{};       // step-wise sharded API: this tick's inputs (smpc_shard_begin .. smpc_shard_combine),
  std::vector<float> step_px, step_py;   // with the path it points at copied here
  bool step_remembered = false;
};

// smpc_critic_breakdown's buffers of its own, allocated at the first call: the 13 rows and the
// totals [14][ld], the pass's partials, a furthest-point word, the result (one float allocation),
// and the reduction's double partials.  Written by smpc_stats.cpp only.
struct BreakdownBufs {
  Event ev[4];                 // SMPC_FLAG_PROFILE: around the scoring pass and around the reduction
  DevBuf<float> d_stats;
  DevBuf<double> d_part;
  uint32_t ld = 0;
  float pass_ms = 0.f, reduce_ms = 0.f;
};

// The trajectory validator's buffers (smpc_validate_trajectory; a group has a set of its own),
// allocated at the first call.  Written by smpc_validate_host.cpp only.
struct ValidateBufs {
  PinnedBuf<uint8_t> h_in;     // SmpcValidateArgs[cap], then the control sequences [cap][3T]: what the ONE upload reads
  DevBuf<uint8_t> d_in;
  PinnedBuf<uint8_t> h_out;    // per member {smpc_validation, xyyaw[T][3]}, mapped into the device: the kernel writes here
  uint8_t* h_out_dev = nullptr;
  uint32_t cap = 0;            // members the three hold
};

// The per-tick block.  `own_d` / `own_h` are the context's own block, allocated by smpc_create and
// the context's for life.  `d_tick` / `h_tick` are the VIEWS everything else reads and writes
// (prepare_tick, the kernels' parameter blocks, the limiter's u): the own block, or — while the
// context is a group's member — its slot of the group's arena.  smpc_group_create repoints the
// views, smpc_group_destroy points them back at the owner; nobody frees through a view.
struct TickBlock {
  DevBuf<uint8_t> own_d;
  PinnedBuf<uint8_t> own_h;
  uint8_t* d_tick = nullptr;
  uint8_t* h_tick = nullptr;
  void view_own() {d_tick = own_d.get(); h_tick = own_h.get();}
  size_t cap = 0;
  // The per-tick upload as CPU stores straight into device memory (large-BAR systems: every
  // MI355X host maps the whole HBM) instead of a copy on the stream: no blit kernel (3.4 us) and
  // no dependent-dispatch gap (4 us) in front of the scoring pass.  SMPC_NO_BAR_TICK=1: the copy.
  // (Tick state, not a knob: a device capability, cleared at run time when a hand-over fails.)
  bool bar_tick = false;
  volatile uint32_t* hdp_flush = nullptr;   // HDP_MEM_FLUSH_CNTL of this device, or null
  size_t used = 0;              // bytes of the tick block this tick fills (a multiple of 16)
  uint32_t no = 0;              // number of the tick block last handed over (its canary word)
  uint32_t canary_expect = 0;   // != 0: fetch_out checks the pass's echo against it
};

}  // namespace smpc_impl

struct smpc_ctx {
  smpc_config cfg{};
  smpc_critic_params critics{};
  float c_vx_max = 0, c_vx_min = 0, c_vy = 0, c_wz = 0;
  int device = 0;
  int num_cu = 256;
  // streams and events first: the buffers below go before them
  smpc_impl::Stream own_stream;
  hipStream_t stream = nullptr;   // the one the ticks run on: own_stream, a caller's (smpc_set_stream) or a group's
  smpc_impl::Event ev0, ev1;
  smpc_impl::Event evp[8];   // SMPC_FLAG_PROFILE: pairs around up to 4 scoring passes
  uint32_t evp_used = 0;
  smpc_impl::Event ev_map;           // behind the last costmap upload
  smpc_impl::NoiseStore noise;
  smpc_impl::Knobs knobs;
  smpc_impl::PassPlan plan;              // this tick's scoring pass (plan_launch)
  smpc_impl::OccCache occ_wave, occ_lane, occ_split;
  bool lane_forced = false;              // SMPC_FLAG_LANE_PER_ROLLOUT / SMPC_PASS=lane|split: the lane pass below kLaneMinBatch too
  bool two_coll_fp = false;              // this tick: BOTH collision critics scored and a consider_footprint switch set —
                                         // they then disagree on which rollouts collide (smpc_optimize: a counting pass)
  uint32_t last_pass_kind = 0;
  // member of a smpc_group: the group uploads every member's tick block in one copy
  bool defer_upload = false;
  // consider_footprint: robot footprint (smpc_set_footprint) and the LUT pair built for it
  std::vector<double> fp_x, fp_y;
  double fp_circumscribed_radius = 0.0, fp_layer_scale = -1.0;
  smpc_impl::DevBuf<SmpcLut> d_lut_fp;      // [2][256]
  smpc_impl::PinnedBuf<SmpcLut> h_lut_fp;
  smpc_impl::ShardLink shard;
  bool pang_any = false;        // this tick: PathAngleCritic is live for some candidate furthest point (prepare_tick, from
                                // path_angle_gates; plan_launch reads it)
  // the lane pass's prune table as last built, and what it was built for (prepare_tick)
  float prune_table[SMPC_PRUNE_FLOATS] = {};
  std::vector<float> prune_px, prune_py;
  uint32_t prune_k0 = 0;
  bool in_group = false;        // member of an smpc_group: full-size blocks always (the group fills the CUs by itself)
  smpc_impl::DevBuf<float> d_costs[2];
  smpc_impl::DevBuf<float> d_traj[3];
  int costs_cur = 0;
  // costmap
  smpc_impl::HostCostmap map;
  smpc_impl::DevBuf<uint8_t> d_map;
  bool map_pending = false;          // the last upload may still be reading the pinned mirror
  uint64_t map_bytes_last = 0, map_bytes_total = 0;   // uploaded by the last call / so far
  smpc_impl::DevBuf<unsigned long long> d_timeline;   // SMPC_LANE_TIMELINE=1 (developer aid)
  // per-tick block
  smpc_impl::DevBuf<SmpcLut> d_lut;
  smpc_impl::PinnedBuf<SmpcLut> h_lut;
  uint64_t lut_key = 0, map_version = 1, critics_version = 1;
  bool lut_valid = false;
  smpc_impl::TickBlock tick;
  bool launched = false;        // kernels of this ctx may still be reading the tick block
  // reductions / outputs
  smpc_impl::DevBuf<float> d_partials;
  smpc_impl::DevBuf<float> d_tuple;
  smpc_impl::DevBuf<float> d_out;       // [SMPC_RESULT_FLOATS(T)]: u, then the result slots (smpc_dev.h)
  smpc_impl::DevBuf<float> d_u_iter;    // [3T] the control sequence iteration it > 0 starts from: a copy of d_out, so that a
                                        // second pass of the same iteration (a re-score) reads what the first one read
  smpc_impl::PinnedBuf<float> h_out;    // [SMPC_RESULT_HOST_FLOATS(T)] device-mapped: kernels write the result here
  float* h_out_dev = nullptr;   // its device-side address
  smpc_impl::DevBuf<float> d_furthest;  // the furthest point, and behind it the other device scratch words (smpc_dev.h: SMPC_SCRATCH_*)
  int R = 1;                 // horizon in chunks of 64 steps per wave of the wave-per-rollout pass: 1, 2 or 4
  // per-tick prepared state
  SmpcDev dev{};
  uint32_t gate_flags = 0;   // critics past their host-side gates this tick
  int score_mode = 0;        // this tick's wave-pass MODE (wave_mode in plan_launch): 0, 3, 4 lean (every cost_power == 1), 2 general
  static int score_mode_for(const smpc_critic_params& cr)
  {
    return (cr.obstacles.cost_power == 1 && cr.path_align.cost_power == 1 &&
           cr.path_follow.cost_power == 1 && cr.goal_angle.cost_power == 1 &&
           cr.prefer_forward.cost_power == 1) ? 0 : 2;
  }
  bool tick_ready = false;
  bool fail_in = false;
  uint32_t P = 0;
  uint32_t passes = 0;
  // speculation on furthest_reached_path_point: the index this tick is scored with first is pred.hint
  smpc_impl::FurthestPredictor pred;
  uint64_t spec_misses = 0;
  // Optimizer::isHolonomic (optimizer.cpp:235).  A non-holonomic model is the Omni data path
  // with the vy noise, control_sequence.vy and state.vy[:,0] all zero: then state.vy = 0,
  // dx = vx cos - 0 sin, the vy gamma term and the weighted vy update are exactly 0 — what the
  // reference's isHolonomic() branches compute (optimizer.cpp:220-224,241-243,264-266,334-337,
  // 374-389), without a second set of kernels.
  bool holonomic = true;
  float acker_r = -1.f;      // Ackermann min_turning_r, < 0 for the other models
  uint32_t acker_seq = 0;    // completion word the Ackermann launch publishes this tick
  uint32_t seq = 0, poll_seq = 0;
  uint32_t poll_words = 0;   // > 0: the tick's completion arrives as this many words, from slot SMPC_R_BLOCK_DONE of h_out on
  smpc_impl::BreakdownBufs stats;
  smpc_impl::Limiter lim;
  smpc_impl::MovingObstacles mov;
  smpc_impl::ValidateBufs val;
  std::string err;
};

namespace smpc_impl {

int fail(smpc_ctx* c, int code, const std::string& msg);

#define HIPCK(ctx, call)                                                               \
  do {                                                                                 \
    hipError_t e__ = (call);                                                           \
    if (e__ != hipSuccess)                                                             \
      return fail(ctx, SMPC_ERR_DEVICE,                                                \
                  std::string(#call) + ": " + hipGetErrorString(e__));                \
  } while (0)

int wait_map_upload(smpc_ctx* c);
// n bytes (a multiple of 16, both 16-byte aligned) from pinned host memory into BAR-mapped device
// memory: streaming stores, fenced before the caller rings any doorbell
void bar_copy(void* dev_dst, const void* host_src, size_t n);
// ... and the device's host-data-path flush behind them (HSA_AMD_AGENT_INFO_HDP_FLUSH), where the
// runtime exposes one
void bar_flush(const smpc_ctx* c);
void free_ctx(smpc_ctx* c);

// tick block layout (offsets in bytes), sized for the ctx's T and SMPC_MAX_PATH
struct TickLayout {
  size_t u, px, py, pyaw, D, pf_idx, pvalid, pa_active, pang_active, pal_active, lut_cost, canary, prune, total;
};
TickLayout tick_layout(uint32_t T, uint32_t P);
// the lane pass's furthest-point prune table for K = k0 .. k0 + 15 (out: SMPC_PRUNE_FLOATS floats)
void build_prune_table(const float* px, const float* py, uint32_t P, uint32_t k0, bool on, float* out);

// LDS carve-up of the streaming pass.  nsamp = PathAlign samples per rollout (0: off).
SmpcLds make_lds(uint32_t window_bytes, uint32_t P, uint32_t T, uint32_t nwave, bool with_map,
                 uint32_t nsamp = 0);
SmpcLds lane_lds(uint32_t window_bytes, uint32_t P, uint32_t T, bool rr = false);
SmpcLds split_lds(uint32_t window_bytes, uint32_t P, uint32_t T, uint32_t nseg);

int check_tick(smpc_ctx* c, const smpc_tick_in* in);
// the furthest point F (index + fraction) is now known for the tick inputs `in`: the next
// prediction starts from here
void remember_furthest(smpc_ctx* c, const smpc_tick_in* in, float F);
void predict_hint(smpc_ctx* c, const smpc_tick_in* in, const float* u_in);
int prepare_tick(smpc_ctx* c, const smpc_tick_in* in, const float* u_in);

int launch_furthest(smpc_ctx* c, float* d_furthest);
void fill_score_args(smpc_ctx* c, uint32_t flags, const float* u_dev, const float* d_furthest,
                     uint32_t furthest_hint, bool finish, const float* finish_furthest, SmpcDev& d,
                     SmpcFinal& fin);
int launch_score(smpc_ctx* c, uint32_t flags, const float* u_dev, const float* d_furthest,
                 uint32_t furthest_hint, float* d_tuple, bool finish = false,
                 const float* finish_furthest = nullptr);
int launch_combine(smpc_ctx* c, const float* d_tuples, uint32_t n, const float* d_furthest_used);
void store_control_sequence(const smpc_ctx* c, float* u_inout);
int fetch_out(smpc_ctx* c);

// ---- the tick protocol its drivers share (smpc_optimize, smpc_group_optimize_some, smpc_shard_tick,
// smpc_shard_begin .. smpc_shard_combine) ----
// a tick starts: the per-tick host work and upload (prepare_tick), then the per-tick counters at zero
int begin_tick(smpc_ctx* c, const smpc_tick_in* in, const float* u_in);
// what no sharded tick takes (after begin_tick)
int refuse_sharded(smpc_ctx* c);
// the next completion sequence number (never 0), which fetch_out then waits for
uint32_t next_seq(smpc_ctx* c);
// device scratch word k of the ctx (smpc_dev.h: SMPC_SCRATCH_*)
inline uint32_t* scratch_word(const smpc_ctx* c, uint32_t k) {return reinterpret_cast<uint32_t*>(c->d_furthest.get()) + k;}
// The result block of the tick fetched last, read in place in the host mirror (no copy: a later
// fetch_out of the same tick shows through the same view).
struct TickResult {
  const float* slot;   // h_out + SMPC_RESULT_AT(T)
  float min_cost() const {return slot[SMPC_R_MIN_COST];}
  float sum_w() const {return slot[SMPC_R_SUM_W];}
  float F_local() const {return slot[SMPC_R_F_LOCAL];}
  float non_colliding() const {return slot[SMPC_R_NON_COLLIDING];}
  float F_used() const {return slot[SMPC_R_F_USED];}
  float mark() const {return slot[SMPC_R_MARK];}
};
inline TickResult tick_result(const smpc_ctx* c) {return TickResult{c->h_out.get() + SMPC_RESULT_AT(c->cfg.time_steps)};}
// *out (may be null) of a finished tick.  What differs between the drivers comes in: the fail flag,
// whether a furthest point was evaluated and the index reported, and a non-colliding count that
// overrides the block's (null: the block's); device_ms: also the call's GPU time, first upload to
// last kernel, when profiling (smpc_optimize).  The rest comes from the block and the ctx.
int fill_tick_out(smpc_ctx* c, smpc_tick_out* out, bool fail_flag, bool furthest_valid, uint32_t furthest,
                  const float* non_colliding = nullptr, bool device_ms = false);
float profile_pass_ms(smpc_ctx* c);
uint32_t fail_only_flags(const smpc_ctx* c);
uint32_t scoring_flags(const smpc_ctx* c, bool fail_sticky);
// ---- acceleration limits ----
// a tick (u_dev null: u is the tick block's) or a later iteration starts: the limited noise of the
// iteration before is stale
void begin_limit_iteration(smpc_ctx* c, const float* u_dev);
// d's noise pointers at the limited noise of the iteration at hand, in the layout the pass about to
// be launched with d reads; made first (one launch on c->stream) if no pass of the iteration read
// that layout yet.  Limits off: nothing.
int use_limited_noise(smpc_ctx* c, SmpcDev& d, bool group_major);
// ---- moving obstacles ----
// d (behind use_limited_noise: its noise pointers are the iteration's) starts its costs from the
// moving-obstacle term: SD_COST_SEED in d.flags — set here, behind the choice of the instance, which
// never sees the bit — and, if no pass of the iteration was seeded yet, one smpc_moving_cost launch on
// c->stream into d.costs_prev, reading the layout the pass reads.  Off, or fail_flag_in: nothing.
int use_moving_seed(smpc_ctx* c, SmpcDev& d, bool group_major);
// The same for a member that rides a group's batched launch: use_moving_seed's bookkeeping, and in
// place of its launch the member's arguments into *mm for the group's ONE smpc_moving_cost_*_many
// launch per form, which goes out behind the hand-over (u is read from the member's tick block on the
// device).  *filled: *mm was written and is of form *form.
int fill_moving_member(smpc_ctx* c, SmpcDev& d, bool group_major, SmpcMovingMember* mm, SmpcMovingForm* form, bool* filled);
// smpc_set_moving_obstacles in its parts, shared with smpc_group_set_moving_obstacles: the checks of a
// table with n > 0 (the message to c's last error), the floats the packed table takes, the table
// packed into `stage` (its three regions, each 16-byte aligned), and the per-member capacity
int check_moving_table(smpc_ctx* c, const smpc_moving_obstacles_params* p, const float* xy, const float* radius, uint32_t n);
size_t moving_table_floats(uint32_t T, uint32_t n);
size_t moving_table_capacity(uint32_t T);
void pack_moving_table(float* stage, uint32_t T, const smpc_moving_obstacles_params* p, const float* xy, const float* radius, uint32_t n);
// the term off: K = 0, nothing scored; the views back at the ctx's own allocation
void moving_off(smpc_ctx* c);
// the table went up on the stream the ctx had then: the one it has now waits for it (once)
int wait_table_upload(smpc_ctx* c);
// {Obstacles,Cost}Critic::findCircumscribedCost: the possibly-inscribed cost of the footprint; -1 without an inflation layer
float circumscribed_cost(const HostCostmap& map, double fp_circumscribed_radius, double fp_layer_scale);
// the same for a first-iteration pass on the [B,T] noise that keeps costs of its own (the critic
// breakdown): m into a buffer of the ctx's (allocated at the first call), which becomes
// d.costs_prev; the tick's own m and hits (smpc_get_moving_obstacle_costs) are left alone
int seed_own_costs(smpc_ctx* c, SmpcDev& d);
int update_time_major(smpc_ctx* c);
int ensure_row_major(smpc_ctx* c);
int draw_noise(smpc_ctx* c);
int redraw_async(smpc_ctx* c);
int cancel_redraw(smpc_ctx* c);
int absorb_redraw(smpc_ctx* c);

}  // namespace smpc_impl

#pragma GCC visibility pop

#endif  // SMPC_CTX_H_
