// smpc_stats.cpp — smpc_critic_breakdown (include/smpc.h): per-critic costs and effective samples
// of the tick smpc_optimize would run next.
//
// The tick is prepared exactly as smpc_optimize prepares it (prepare_tick: the same gates, tables
// and upload), scored by smpc_pass_stats — the general wave pass keeping every critic's term
// (smpc_wave_stats.hip) — into buffers of the breakdown's own, and reduced there.  What a tick
// carries over to the next one (the furthest-point predictor, the launch plan the prune table
// looks at, the counters) is put back before the call returns; costs, u and the result block are
// never written.
//
// smpc_group_critic_breakdown is the same for the members of an smpc_group in launches whose number
// does not depend on the group's size (smpc_wave_stats_many.hip), each member carried likewise.

#include "smpc_ctx.h"
#include "smpc_group.h"
#include "../../include/smpc_debug.h"   // smpc_debug_stats_ms

namespace smpc_impl {

static const char* const kCriticNames[SMPC_STATS_ROWS] = {
  "ConstraintCritic", "CostCritic", "ObstaclesCritic", "PathAlignCritic", "PathAlignLegacyCritic", "PathFollowCritic",
  "GoalAngleCritic", "PreferForwardCritic", "GoalCritic", "PathAngleCritic", "TwirlingCritic", "VelocityDeadbandCritic",
  "ControlCost"};

// What prepare_tick and the furthest-point pre-pass change and a later tick would see: the predictor
// as a whole (the breakdown runs predict_hint — the hint, the last prediction, the nominal endpoint of
// the tick at hand — and never remember_furthest, so the anchor and the drift come back as they
// were: a field added to the predictor is carried without being named here), the launch plan
// (plan_launch; the next tick's prune_table_for_tick reads it), the last kernel's name (the
// pre-pass and the stats pass write it) and the pass counters.
struct Carried {
  FurthestPredictor pred;
  PassPlan plan;
  uint32_t passes, last_pass_kind;
  char last_kernel[sizeof(smpc_last_pass_kernel)];
};
static Carried save_carried(const smpc_ctx* c)
{
  Carried s{c->pred, c->plan, c->passes, c->last_pass_kind, {}};
  memcpy(s.last_kernel, smpc_last_pass_kernel, sizeof(s.last_kernel));
  return s;
}
static void restore_carried(smpc_ctx* c, Carried& s)
{
  c->pred = std::move(s.pred);
  c->plan = s.plan;
  c->passes = s.passes;
  c->last_pass_kind = s.last_pass_kind;
  memcpy(smpc_last_pass_kernel, s.last_kernel, sizeof(s.last_kernel));
}

// the float regions of d_stats, in floats from its start (each a multiple of four: 16-byte aligned)
struct StatsLayout {
  size_t rows, costs, partials, furthest, out, total;
};
static StatsLayout stats_layout(uint32_t ld, uint32_t T)
{
  StatsLayout l{};
  l.rows = 0;
  l.costs = static_cast<size_t>(SMPC_STATS_ROWS) * ld;
  l.partials = l.costs + ld;
  l.furthest = l.partials + align_up(kMaxGrid * (SMPC_TUPLE_HEADER + 3u * T) + 16u, 4);   // (+ the canary's slot, as d_partials)
  l.out = l.furthest + 4;
  l.total = l.out + align_up(static_cast<uint32_t>(sizeof(SmpcStatsOut) / sizeof(float)), 4);
  return l;
}

// where one breakdown's pass and reduction work: the regions above in the ctx's own d_stats, or a
// member's regions of its group's arena (GroupStatsArena).  costs follows rows: one memset clears both.
struct StatsBufs {
  float* rows = nullptr;       // [SMPC_STATS_ROWS][ld]
  float* costs = nullptr;      // [ld]
  float* partials = nullptr;
  float* furthest = nullptr;
  SmpcStatsOut* out = nullptr;
  double* part = nullptr;      // the reduction's (SMPC_STATS_ROWS + 1) x slices x 4 doubles
  uint32_t ld = 0;
};
static StatsBufs own_bufs(const smpc_ctx* c)
{
  const StatsLayout l = stats_layout(c->stats.ld, c->cfg.time_steps);
  float* base = c->stats.d_stats.get();
  return StatsBufs{base + l.rows, base + l.costs, base + l.partials, base + l.furthest,
                   reinterpret_cast<SmpcStatsOut*>(base + l.out), c->stats.d_part.get(), c->stats.ld};
}

static int ensure_buffers(smpc_ctx* c)
{
  if (c->stats.d_stats) return SMPC_OK;
  const uint32_t B = c->cfg.batch_size, T = c->cfg.time_steps;
  const uint32_t ld = align_up(B, 4);
  const StatsLayout l = stats_layout(ld, T);
  uint32_t slice = 0;
  const uint32_t S = stats_reduce_slices(B, &slice);
  HIPCK(c, stats_set_lds_limit(static_cast<int>(kLdsPerCu)));
  // (d_stats last: it marks the set complete — a call that failed half way picks up where it stopped)
  HIPCK(c, c->stats.d_part.ensure(static_cast<size_t>(SMPC_STATS_ROWS + 1) * S * 4));
  for (Event& e : c->stats.ev) HIPCK(c, e.ensure());
  c->stats.ld = ld;
  HIPCK(c, c->stats.d_stats.ensure(l.total));
  return SMPC_OK;
}

// which rows the pass scored with these flags at furthest point S (the per-S gates it reads from
// the tick block, here from the block's host copy)
static uint32_t scored_rows(const smpc_ctx* c, uint32_t flags, uint32_t S)
{
  const uint32_t P = c->P;
  const TickLayout tl = tick_layout(c->cfg.time_steps, std::max(P, 1u));
  const uint8_t* h = c->tick.h_tick;
  if (S >= P) S = P ? P - 1 : 0;
  uint32_t m = 1u << SMPC_STATS_CONTROL;
  auto row = [&](bool on, uint32_t k) {if (on) m |= 1u << k;};
  row(flags & SD_CONSTRAINT, SMPC_CRITIC_CONSTRAINT);
  row(flags & SD_COST, SMPC_CRITIC_COST);
  row(flags & SD_OBSTACLES, SMPC_CRITIC_OBSTACLES);
  row((flags & SD_PATH_ALIGN) && P > 0 && S > 0 && h[tl.pa_active + S], SMPC_CRITIC_PATH_ALIGN);
  row((flags & SD_PATH_ALIGN_LEGACY) && P > 1 && h[tl.pal_active + S], SMPC_CRITIC_PATH_ALIGN_LEGACY);
  row((flags & SD_PATH_FOLLOW) && P > 0, SMPC_CRITIC_PATH_FOLLOW);
  row(flags & SD_GOAL_ANGLE, SMPC_CRITIC_GOAL_ANGLE);
  row(flags & SD_PREFER_FORWARD, SMPC_CRITIC_PREFER_FORWARD);
  row(flags & SD_GOAL, SMPC_CRITIC_GOAL);
  row((flags & SD_PATH_ANGLE) && P > 0 && h[tl.pang_active + S], SMPC_CRITIC_PATH_ANGLE);
  row(flags & SD_TWIRLING, SMPC_CRITIC_TWIRLING);
  row(flags & SD_DEADBAND, SMPC_CRITIC_VELOCITY_DEADBAND);
  return m;
}

// one stats pass + reduction with `flags`; the result on the host in *o
static int score_rows(smpc_ctx* c, const StatsBufs& sb, uint32_t flags, const float* d_furthest, SmpcStatsOut* o)
{
  const uint32_t T = c->cfg.time_steps, ld = sb.ld;
  const bool prof = (c->cfg.flags & SMPC_FLAG_PROFILE) != 0 && c->stats.ev[0].get();   // (events: ensure_buffers, a ctx's own breakdown)
  // rows the pass does not score hold zeros
  HIPCK(c, hipMemsetAsync(sb.rows, 0, static_cast<size_t>(SMPC_STATS_ROWS + 1) * ld * sizeof(float), c->stream));
  SmpcDev d = c->dev;
  d.flags = flags;
  d.d_furthest = d_furthest;
  d.furthest_hint = 0;
  d.costs = sb.costs;
  d.costs_prev = nullptr;          // (never SD_ACCUMULATE: the first iteration)
  d.partials = sb.partials;
  d.tail = 0;
  const StatsInst* k = stats_select(c->R, T);
  if (!k) return fail(c, SMPC_ERR_UNSUPPORTED, "no instance of the stats pass for this horizon");
  const PassGeom& g = c->plan.wave;   // planned for every tick, whatever pass the tick itself takes
  {
    int rc = ensure_row_major(c);
    if (rc != SMPC_OK) return rc;
    // acceleration limits: the [B,T] limited noise (a lane context has it only because of this call)
    rc = use_limited_noise(c, d, false);
    if (rc != SMPC_OK) return rc;
    // moving obstacles: the costs start from m, as the tick's do — no row carries the term, so the
    // rows add up to the cost minus m
    rc = seed_own_costs(c, d);
    if (rc != SMPC_OK) return rc;
  }
  c->launched = true;
  if (prof) HIPCK(c, hipEventRecord(c->stats.ev[0].get(), c->stream));
  HIPCK(c, stats_launch(k, d, g.lds, sb.rows, ld, g.grid, g.block, c->stream));
  if (prof) {
    HIPCK(c, hipEventRecord(c->stats.ev[1].get(), c->stream));
    HIPCK(c, hipEventRecord(c->stats.ev[2].get(), c->stream));
  }
  HIPCK(c, stats_launch_reduce(sb.rows, ld, sb.costs, d.B, d.k2, sb.part, sb.partials, g.grid, T, sb.out, c->stream));
  if (prof) HIPCK(c, hipEventRecord(c->stats.ev[3].get(), c->stream));
  HIPCK(c, hipMemcpyAsync(o, sb.out, sizeof(*o), hipMemcpyDeviceToHost, c->stream));
  HIPCK(c, hipStreamSynchronize(c->stream));
  c->launched = false;
  if (prof) {
    (void)hipEventElapsedTime(&c->stats.pass_ms, c->stats.ev[0].get(), c->stats.ev[1].get());
    (void)hipEventElapsedTime(&c->stats.reduce_ms, c->stats.ev[2].get(), c->stats.ev[3].get());
  }
  return SMPC_OK;
}

static const char* const kTwoCollFp =
  "critic breakdown: consider_footprint=true with both ObstaclesCritic and CostCritic in the list";

// the struct of one breakdown: what was scored (flags at furthest point S) and what the reduction left
static void fill_stats(const smpc_ctx* c, uint32_t flags, uint32_t S, bool fail_flag, const SmpcStatsOut& o, smpc_critic_stats* stats)
{
  memset(stats, 0, sizeof(*stats));
  stats->scored_mask = scored_rows(c, flags, S);
  stats->fail_flag = fail_flag ? 1u : 0u;
  stats->batch = c->cfg.batch_size;
  stats->best_rollout = o.best_rollout;
  stats->best_cost = o.best_cost;
  stats->effective_samples = o.effective_samples;
  static_assert(sizeof(o.sum) == sizeof(stats->sum), "the device result's rows are the struct's");
  memcpy(stats->sum, o.sum, sizeof(o.sum));
  memcpy(stats->min, o.min, sizeof(o.min));
  memcpy(stats->max, o.max, sizeof(o.max));
  memcpy(stats->weighted, o.weighted, sizeof(o.weighted));
  memcpy(stats->at_best, o.at_best, sizeof(o.at_best));
}

static int fetch_rows(smpc_ctx* c, const StatsBufs& sb, float* per_rollout)
{
  const size_t row = c->cfg.batch_size * sizeof(float);
  HIPCK(c, hipMemcpy2D(per_rollout, row, sb.rows, sb.ld * sizeof(float), row, SMPC_STATS_ROWS, hipMemcpyDeviceToHost));
  return SMPC_OK;
}

static int breakdown(smpc_ctx* c, const smpc_tick_in* in, const float* u_in, smpc_critic_stats* stats, float* per_rollout)
{
  int rc = prepare_tick(c, in, u_in);
  if (rc != SMPC_OK) return rc;
  if (c->two_coll_fp) return fail(c, SMPC_ERR_UNSUPPORTED, kTwoCollFp);
  rc = ensure_buffers(c);
  if (rc != SMPC_OK) return rc;
  const StatsBufs sb = own_bufs(c);
  // the first iteration's flags (smpc_optimize), without the trajectory write-out: its tensors are the tick's
  uint32_t flags = scoring_flags(c, c->fail_in) & ~SD_STORE_TRAJ;
  bool fail_flag = c->fail_in;
  float* dF = nullptr;
  if (flags & SD_NEED_FURTHEST) {
    dF = sb.furthest;
    rc = launch_furthest(c, dF);
    if (rc != SMPC_OK) return rc;
  }
  SmpcStatsOut o{};
  rc = score_rows(c, sb, flags, dF, &o);
  if (rc != SMPC_OK) return rc;
  uint32_t S = 0;
  if (dF) {
    float F = 0.f;
    HIPCK(c, hipMemcpy(&F, dF, sizeof(F), hipMemcpyDeviceToHost));
    S = smpc_furthest_index(F);
  }
  // every rollout collides: the critics behind the collision critic were not scored in the
  // reference (critic_manager.cpp:70-73) — the rows are those of the tick's re-score
  if (!c->fail_in && (flags & (SD_OBSTACLES | SD_COST)) && o.non_colliding == 0.0f) {
    fail_flag = true;
    flags = fail_only_flags(c) & ~SD_STORE_TRAJ;
    S = 0;
    rc = score_rows(c, sb, flags, nullptr, &o);
    if (rc != SMPC_OK) return rc;
  }
  fill_stats(c, flags, S, fail_flag, o, stats);
  if (per_rollout) return fetch_rows(c, sb, per_rollout);
  return SMPC_OK;
}

// a breakdown that leaves the ctx as it found it, whatever it returns
static int breakdown_carried(smpc_ctx* c, const smpc_tick_in* in, const float* u_in, smpc_critic_stats* stats, float* per_rollout)
{
  Carried carried = save_carried(c);
  const int rc = breakdown(c, in, u_in, stats, per_rollout);
  if (rc != SMPC_OK && c->launched) {
    (void)hipStreamSynchronize(c->stream);   // nothing of an abandoned breakdown may run into the next tick
    c->launched = false;
  }
  restore_carried(c, carried);
  return rc;
}

// ---- smpc_group_critic_breakdown: the members' float regions in one allocation of the group's ----
// In floats from the arena's start, for the m members that ride (in their order):
//   [rows + costs of member 0] .. [rows + costs of member m-1] [furthest-point words, four floats each]
//       — what ONE memset clears (rows the pass does not score hold zeros; the pre-pass raises its word from 0)
//   [SmpcStatsOut of member 0 ..]   — with the furthest-point words in front of it what ONE copy brings back
//   [the pass's partials of member 0 ..]
struct GroupStatsArena {
  std::vector<size_t> rows;   // per member
  std::vector<uint32_t> ld;
  size_t furthest = 0, out = 0, partials = 0, total = 0;
  size_t out_floats = 0, partial_floats = 0;   // per member
  std::vector<size_t> part;   // per member, in doubles from d_stats_part
  size_t part_total = 0;
  uint32_t slices_max = 0;
};
static GroupStatsArena group_arena(const smpc_group* g, const std::vector<uint32_t>& order)
{
  GroupStatsArena a;
  const uint32_t T = g->ctxs[order[0]]->cfg.time_steps;
  size_t at = 0;
  for (uint32_t i : order) {
    const uint32_t B = g->ctxs[i]->cfg.batch_size, ld = align_up(B, 4);
    a.rows.push_back(at);
    a.ld.push_back(ld);
    at += static_cast<size_t>(SMPC_STATS_ROWS + 1) * ld;
    const uint32_t S = stats_reduce_slices(B, nullptr);
    a.part.push_back(a.part_total);
    a.part_total += static_cast<size_t>(SMPC_STATS_ROWS + 1) * S * 4;
    a.slices_max = std::max(a.slices_max, S);
  }
  const size_t m = order.size();
  a.furthest = at;
  a.out = a.furthest + 4 * m;
  a.out_floats = align_up(static_cast<uint32_t>(sizeof(SmpcStatsOut) / sizeof(float)), 4);
  a.partials = a.out + a.out_floats * m;
  a.partial_floats = align_up(kMaxGrid * (SMPC_TUPLE_HEADER + 3u * T) + 16u, 4);   // (as stats_layout)
  a.total = a.partials + a.partial_floats * m;
  return a;
}

}  // namespace smpc_impl

using namespace smpc_impl;

extern "C" {

const char* smpc_critic_name(uint32_t id) {return id < SMPC_STATS_ROWS ? kCriticNames[id] : nullptr;}

int smpc_critic_breakdown(smpc_ctx* c, const smpc_tick_in* in, const float* u_in, smpc_critic_stats* stats, float* per_rollout)
{
  if (!c || !in || !u_in || !stats) return fail(c, SMPC_ERR_INVALID, "null argument");
  if (c->in_group || c->defer_upload)
    return fail(c, SMPC_ERR_STATE, "critic breakdown: the ctx is a member of a group (its tick block is the group's)");
  HIPCK(c, hipSetDevice(c->device));
  return breakdown_carried(c, in, u_in, stats, per_rollout);
}

int smpc_group_breakdown_counts(const smpc_group* g, uint64_t* batched_members, uint64_t* single_members)
{
  if (!g) return SMPC_ERR_INVALID;
  if (batched_members) *batched_members = g->breakdown_batched;
  if (single_members) *single_members = g->breakdown_single;
  return SMPC_OK;
}

// The breakdown of every member taken, the group staying a group.  Each member's tick is prepared as
// a round prepares it (prepare_tick into its slot of the group's blocks, nothing uploaded yet); then
// ONE memset, ONE upload, the pre-pass of the members that need a furthest point, the stats pass and
// the two reduction launches for all of them, ONE copy back and ONE wait.  In front of the pass, on
// the same stream: what prepare_tick itself enqueues per member (lookup tables that changed), the
// [B,T] copy of a lane member's noise, and the limiter of a member with acceleration limits — as in
// a round.  Behind it: the re-score of a member whose rollouts all collide, one by one (score_rows:
// the single call's launches into the member's regions of the arena), and the rows of the members
// that asked for them.  Every member is put back as it was found (Carried).
int smpc_group_critic_breakdown(smpc_group* g, const smpc_tick_in* ins, const float* const* u_ins, const uint8_t* take,
                                smpc_critic_stats* stats, float* const* per_rollout, int32_t* status)
{
  if (!g || !ins || !u_ins || !stats || !status) return fail(nullptr, SMPC_ERR_INVALID, "null argument");
  const uint32_t n = static_cast<uint32_t>(g->ctxs.size());
  auto taken = [&](uint32_t i) {return !take || take[i] != 0;};
  uint32_t first = 0;
  while (first < n && !taken(first)) ++first;
  if (first == n) return fail(nullptr, SMPC_ERR_INVALID, "critic breakdown: no member of the group is taken");
  smpc_ctx* c0 = g->ctxs[first];    // (errors of the call as a whole are reported on the first member taken)
  HIPCK(c0, hipSetDevice(c0->device));
  if (g->launched) {
    // the round before was abandoned between its launch and its last fetch_out (smpc_group_optimize_some)
    HIPCK(c0, hipStreamSynchronize(g->stream));
    g->launched = false;
  }
  const uint32_t T = c0->cfg.time_steps;
  const StatsManyInst* k = stats_many_select(c0->R, T);
  if (!k) {
    // T > 64: no grouped instance (as smpc_pass_many) — one by one, each with its own upload into
    // its slot of the group's blocks, as a round ticks a member alone
    for (uint32_t i = 0; i < n; ++i) {
      if (!taken(i)) continue;
      smpc_ctx* c = g->ctxs[i];
      c->defer_upload = false;
      status[i] = u_ins[i] ? breakdown_carried(c, &ins[i], u_ins[i], &stats[i], per_rollout ? per_rollout[i] : nullptr)
                           : fail(c, SMPC_ERR_INVALID, "null control sequence");
      c->defer_upload = true;
      g->breakdown_single++;
      if (status[i] == SMPC_ERR_DEVICE) return status[i];
    }
    return SMPC_OK;
  }
  // ---- prepare every member taken -------------------------------------------------------------
  std::vector<Carried> carried(n);
  std::vector<bool> saved(n, false);
  // what every way out of here does: nothing of this call runs on, every member as it was found
  auto put_back = [&](bool wait) {
    if (wait) (void)hipStreamSynchronize(g->stream);
    for (uint32_t i = n; i-- > 0;) {   // (in reverse: the kernel name the first one saved is the one that stays)
      if (!saved[i]) continue;
      if (wait) g->ctxs[i]->launched = false;
      restore_carried(g->ctxs[i], carried[i]);
    }
    if (wait) g->launched = false;
  };
  std::vector<uint32_t> order, flags(n, 0u);
  for (uint32_t i = 0; i < n; ++i) {
    if (!taken(i)) continue;
    smpc_ctx* c = g->ctxs[i];
    carried[i] = save_carried(c);
    saved[i] = true;
    int rc = u_ins[i] ? prepare_tick(c, &ins[i], u_ins[i]) : fail(c, SMPC_ERR_INVALID, "null control sequence");
    if (rc == SMPC_OK && c->two_coll_fp) rc = fail(c, SMPC_ERR_UNSUPPORTED, kTwoCollFp);
    if (rc == SMPC_OK) rc = ensure_row_major(c);   // the wave-per-rollout pass reads the [B,T] tensors
    status[i] = rc;
    if (rc == SMPC_ERR_DEVICE) {
      put_back(true);
      return rc;
    }
    if (rc != SMPC_OK) continue;   // this member's own refusal: the others go on
    // the first iteration's flags (smpc_optimize), without the trajectory write-out
    flags[i] = scoring_flags(c, c->fail_in) & ~SD_STORE_TRAJ;
    order.push_back(i);
  }
  if (order.empty()) {
    put_back(true);
    return SMPC_OK;
  }
  const uint32_t m = static_cast<uint32_t>(order.size());
  auto give_up = [&](int rc) {
    put_back(true);
    return rc;
  };
#define GHIPCK(call)                                                                                           \
  do {                                                                                                         \
    hipError_t e__ = (call);                                                                                   \
    if (e__ != hipSuccess) return give_up(fail(c0, SMPC_ERR_DEVICE, std::string(#call) + ": " + hipGetErrorString(e__))); \
  } while (0)
  // ---- the arena ---------------------------------------------------------------------------------
  const GroupStatsArena a = group_arena(g, order);
  const size_t back_floats = a.partials - a.furthest;   // the furthest-point words and the results: one copy
  if (!g->stats_lds_set) {
    GHIPCK(stats_many_set_lds_limit(static_cast<int>(kLdsPerCu)));
    GHIPCK(stats_set_lds_limit(static_cast<int>(kLdsPerCu)));   // (the re-score of a member that collides everywhere)
    g->stats_lds_set = true;
  }
  // (grown where the members taken ask for more; nothing of an earlier call still runs: every call ends with a wait)
  GHIPCK(g->d_stats.ensure(a.total));
  GHIPCK(g->d_stats_part.ensure(a.part_total));
  GHIPCK(g->h_stats_out.ensure(back_floats));
  // ---- the argument arrays -----------------------------------------------------------------------
  SmpcDev* hd = reinterpret_cast<SmpcDev*>(g->h_all.get() + g->off_dev);
  SmpcWaveGeom* hg = reinterpret_cast<SmpcWaveGeom*>(g->h_all.get() + g->off_geo);
  SmpcDev* hfd = reinterpret_cast<SmpcDev*>(g->h_all.get() + g->off_fdev);
  SmpcWaveGeom* hfg = reinterpret_cast<SmpcWaveGeom*>(g->h_all.get() + g->off_fgeo);
  SmpcStatsDst* hdst = reinterpret_cast<SmpcStatsDst*>(g->h_all.get() + g->off_sdst);
  SmpcStatsReduceArgs* hred = reinterpret_cast<SmpcStatsReduceArgs*>(g->h_all.get() + g->off_sred);
  std::vector<StatsBufs> bufs(m);
  uint32_t nf = 0, grid_max = 0, lds_max = 0, fgrid_max = 0, flds_max = 0;
  const uint32_t block = pass_block(c0->R);
  for (uint32_t j = 0; j < m; ++j) {
    smpc_ctx* c = g->ctxs[order[j]];
    StatsBufs& sb = bufs[j];
    sb.ld = a.ld[j];
    sb.rows = g->d_stats.get() + a.rows[j];
    sb.costs = sb.rows + static_cast<size_t>(SMPC_STATS_ROWS) * sb.ld;
    sb.furthest = g->d_stats.get() + a.furthest + 4 * j;
    sb.out = reinterpret_cast<SmpcStatsOut*>(g->d_stats.get() + a.out + a.out_floats * j);
    sb.partials = g->d_stats.get() + a.partials + a.partial_floats * j;
    sb.part = g->d_stats_part.get() + a.part[j];
    const PassGeom& pg = c->plan.wave;   // planned for every tick, whatever pass the tick itself takes
    const bool need_f = (flags[order[j]] & SD_NEED_FURTHEST) != 0;
    if (need_f) {
      // (launch_furthest's parameter block and carve-up, its word this member's own)
      SmpcDev& d = hfd[nf];
      d = c->dev;
      const int rc = use_limited_noise(c, d, false);
      if (rc != SMPC_OK) return give_up(rc);
      d.flags = c->gate_flags & SD_NEED_FURTHEST;
      d.furthest_out = reinterpret_cast<uint32_t*>(sb.furthest);
      hfg[nf].lds = make_lds(0, c->P, T, block / 64, false);
      hfg[nf].grid = pg.grid;
      fgrid_max = std::max(fgrid_max, pg.grid);
      flds_max = std::max(flds_max, hfg[nf].lds.total);
      nf++;
    }
    // (score_rows' parameter block)
    SmpcDev& d = hd[j];
    d = c->dev;
    d.flags = flags[order[j]];
    d.d_furthest = need_f ? sb.furthest : nullptr;
    d.furthest_hint = 0;
    d.costs = sb.costs;
    d.costs_prev = nullptr;
    d.partials = sb.partials;
    d.tail = 0;
    {
      int rc = use_limited_noise(c, d, false);
      if (rc != SMPC_OK) return give_up(rc);
      rc = seed_own_costs(c, d);   // (a member with moving obstacles: its seed kernel on the group's stream, as in a round)
      if (rc != SMPC_OK) return give_up(rc);
    }
    hg[j].lds = pg.lds;
    hg[j].grid = pg.grid;
    grid_max = std::max(grid_max, pg.grid);
    lds_max = std::max(lds_max, pg.lds.total);
    hdst[j].stats = sb.rows;
    hdst[j].ld = sb.ld;
    SmpcStatsReduceArgs& r = hred[j];
    r.stats = sb.rows;
    r.costs = sb.costs;
    r.part = sb.part;
    r.pass_partials = sb.partials;
    r.out = sb.out;
    r.ld = sb.ld;
    r.B = d.B;
    r.S = stats_reduce_slices(d.B, &r.slice);
    r.nblk = pg.grid;
    r.TL = 4u + 3u * T;
    r.k2 = d.k2;
  }
  // ---- one memset, one upload, the launches, one copy back, one wait -------------------------------
  GHIPCK(hipMemsetAsync(g->d_stats.get(), 0, a.out * sizeof(float), g->stream));
  if (c0->tick.bar_tick) {
    // (every member's last tick or breakdown was waited for: nothing reads the blocks)
    for (uint32_t i : order) bar_copy(g->d_all.get() + g->slot * i, g->h_all.get() + g->slot * i, g->ctxs[i]->tick.used);
    bar_copy(g->d_all.get() + g->off_dev, g->h_all.get() + g->off_dev, g->total_stats - g->off_dev);
    bar_flush(c0);
  }
  else GHIPCK(hipMemcpyAsync(g->d_all.get(), g->h_all.get(), g->total_stats, hipMemcpyHostToDevice, g->stream));
  g->launched = true;
  if (nf)
    GHIPCK(stats_launch_furthest_many(k, reinterpret_cast<const SmpcDev*>(g->d_all.get() + g->off_fdev),
                                      reinterpret_cast<const SmpcWaveGeom*>(g->d_all.get() + g->off_fgeo), nf, fgrid_max, flds_max, block,
                                      g->stream));
  GHIPCK(stats_launch_many(k, reinterpret_cast<const SmpcDev*>(g->d_all.get() + g->off_dev),
                           reinterpret_cast<const SmpcWaveGeom*>(g->d_all.get() + g->off_geo),
                           reinterpret_cast<const SmpcStatsDst*>(g->d_all.get() + g->off_sdst), m, grid_max, lds_max, block, g->stream));
  GHIPCK(stats_launch_reduce_many(reinterpret_cast<const SmpcStatsReduceArgs*>(g->d_all.get() + g->off_sred), m, a.slices_max, g->stream));
  GHIPCK(hipMemcpyAsync(g->h_stats_out.get(), g->d_stats.get() + a.furthest, back_floats * sizeof(float), hipMemcpyDeviceToHost, g->stream));
  GHIPCK(hipStreamSynchronize(g->stream));
  g->launched = false;
  for (uint32_t i : order) g->ctxs[i]->launched = false;
  g->breakdown_batched += m;
  // ---- per member: the struct, the re-score of one that collides everywhere, the rows ------------
  for (uint32_t j = 0; j < m; ++j) {
    const uint32_t i = order[j];
    smpc_ctx* c = g->ctxs[i];
    SmpcStatsOut o;
    memcpy(&o, g->h_stats_out.get() + (a.out - a.furthest) + a.out_floats * j, sizeof(o));
    uint32_t fl = flags[i], S = 0;
    bool fail_flag = c->fail_in;
    if (fl & SD_NEED_FURTHEST) S = smpc_furthest_index(g->h_stats_out.get()[4 * j]);
    int rc = SMPC_OK;
    if (!c->fail_in && (fl & (SD_OBSTACLES | SD_COST)) && o.non_colliding == 0.0f) {
      // (critic_manager.cpp:70-73, as the single call: the rows are those of the tick's re-score)
      fail_flag = true;
      fl = fail_only_flags(c) & ~SD_STORE_TRAJ;
      S = 0;
      rc = score_rows(c, bufs[j], fl, nullptr, &o);
    }
    if (rc == SMPC_OK) {
      fill_stats(c, fl, S, fail_flag, o, &stats[i]);
      if (per_rollout && per_rollout[i]) rc = fetch_rows(c, bufs[j], per_rollout[i]);
    }
    status[i] = rc;
    if (rc == SMPC_ERR_DEVICE) return give_up(rc);
  }
#undef GHIPCK
  put_back(false);
  return SMPC_OK;
}

// developer aid (SMPC_FLAG_PROFILE): GPU time of the last breakdown's scoring pass and of its
// reduction (both launches), by HIP events; of the re-score when every rollout collided
int smpc_debug_stats_ms(const smpc_ctx* c, float* pass_ms, float* reduce_ms)
{
  if (!c || !pass_ms || !reduce_ms) return SMPC_ERR_INVALID;
  *pass_ms = c->stats.pass_ms;
  *reduce_ms = c->stats.reduce_ms;
  return SMPC_OK;
}

}  // extern "C"
