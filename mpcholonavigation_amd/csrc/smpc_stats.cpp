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
  std::vector<size_t> part;   // per member, in doubles from the group's d_part (GroupStatsBufs)
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

// ---- smpc_group_critic_breakdown in its stages ------------------------------------------------------
namespace {

// What every way out of a grouped breakdown does: when it goes, every member saved is put back as it
// was found, in reverse (the kernel name the first one saved is the one that stays).  Unless told
// wait = false — the success path alone, which has waited — it first waits for the group's stream and
// clears the launched flags: nothing of an abandoned call runs on.
struct MembersPutBack {
  smpc_group* g = nullptr;   // null: not armed, nothing to do
  std::vector<Carried> carried;
  std::vector<bool> saved;
  bool wait = true;
  MembersPutBack() = default;
  MembersPutBack(const MembersPutBack&) = delete;
  MembersPutBack& operator=(const MembersPutBack&) = delete;
  void arm(smpc_group* group)
  {
    g = group;
    carried.resize(g->ctxs.size());
    saved.assign(g->ctxs.size(), false);
  }
  void save(uint32_t i)
  {
    carried[i] = save_carried(g->ctxs[i]);
    saved[i] = true;
  }
  ~MembersPutBack()
  {
    if (!g) return;
    if (wait) (void)hipStreamSynchronize(g->stream);
    for (uint32_t i = static_cast<uint32_t>(saved.size()); i-- > 0;) {
      if (!saved[i]) continue;
      if (wait) g->ctxs[i]->launched = false;
      restore_carried(g->ctxs[i], carried[i]);
    }
    if (wait) g->launched = false;
  }
};

// the state the stages hand on
struct GroupBreakdown {
  // the caller's arrays
  const smpc_tick_in* ins;
  const float* const* u_ins;
  const uint8_t* take;
  smpc_critic_stats* stats;
  float* const* per_rollout;
  int32_t* status;
  smpc_ctx* c0 = nullptr;   // the first member taken
  uint32_t n = 0, T = 0;
  const StatsManyInst* k = nullptr;   // the grouped instance (null: none for this horizon)
  MembersPutBack put_back;
  std::vector<uint32_t> order, flags;   // the members that ride, by member index; per member: its scoring flags
  GroupStatsArena a;
  std::vector<StatsBufs> bufs;          // per rider: its regions of the arena
  uint32_t nf = 0;                      // riders that need a furthest point: the pre-pass's members
  uint32_t grid_max = 0, lds_max = 0, fgrid_max = 0, flds_max = 0, block = 0;
  size_t back_floats() const {return a.partials - a.furthest;}   // the furthest-point words and the results: one copy
};

// T > 64: no grouped instance (as smpc_pass_many) — one by one, each with its own upload into its
// slot of the group's blocks, as a round ticks a member alone
static int breakdown_one_by_one(smpc_group* g, GroupBreakdown& b)
{
  for (uint32_t i = 0; i < b.n; ++i) {
    if (!group_takes(b.take, i)) continue;
    smpc_ctx* c = g->ctxs[i];
    c->defer_upload = false;
    b.status[i] = b.u_ins[i] ? breakdown_carried(c, &b.ins[i], b.u_ins[i], &b.stats[i], b.per_rollout ? b.per_rollout[i] : nullptr)
                             : fail(c, SMPC_ERR_INVALID, "null control sequence");
    c->defer_upload = true;
    g->count.breakdown_single++;
    if (b.status[i] == SMPC_ERR_DEVICE) return b.status[i];
  }
  return SMPC_OK;
}

// prepare every member taken, each saved first; a member's own refusal lets the others go on
static int breakdown_prepare(smpc_group* g, GroupBreakdown& b)
{
  b.put_back.arm(g);
  b.flags.assign(b.n, 0u);
  for (uint32_t i = 0; i < b.n; ++i) {
    if (!group_takes(b.take, i)) continue;
    smpc_ctx* c = g->ctxs[i];
    b.put_back.save(i);
    int rc = b.u_ins[i] ? prepare_tick(c, &b.ins[i], b.u_ins[i]) : fail(c, SMPC_ERR_INVALID, "null control sequence");
    if (rc == SMPC_OK && c->two_coll_fp) rc = fail(c, SMPC_ERR_UNSUPPORTED, kTwoCollFp);
    if (rc == SMPC_OK) rc = ensure_row_major(c);   // the wave-per-rollout pass reads the [B,T] tensors
    b.status[i] = rc;
    if (rc == SMPC_ERR_DEVICE) return rc;
    if (rc != SMPC_OK) continue;
    // the first iteration's flags (smpc_optimize), without the trajectory write-out
    b.flags[i] = scoring_flags(c, c->fail_in) & ~SD_STORE_TRAJ;
    b.order.push_back(i);
  }
  return SMPC_OK;
}

// the arena for the riders and the group's buffers behind it
static int breakdown_buffers(smpc_group* g, GroupBreakdown& b)
{
  b.a = group_arena(g, b.order);
  GroupStatsBufs& s = g->stats;
  if (!s.lds_set) {
    HIPCK(b.c0, stats_many_set_lds_limit(static_cast<int>(kLdsPerCu)));
    HIPCK(b.c0, stats_set_lds_limit(static_cast<int>(kLdsPerCu)));   // (the re-score of a member that collides everywhere)
    s.lds_set = true;
  }
  // (grown where the members taken ask for more; nothing of an earlier call still runs: every call ends with a wait)
  HIPCK(b.c0, s.d_stats.ensure(b.a.total));
  HIPCK(b.c0, s.d_part.ensure(b.a.part_total));
  HIPCK(b.c0, s.h_out.ensure(b.back_floats()));
  return SMPC_OK;
}

// the argument arrays: per rider the stats pass's parameter block, geometry, rows and reduction
// arguments; per rider that needs a furthest point the pre-pass's parameter block and geometry
static int breakdown_fill(smpc_group* g, GroupBreakdown& b)
{
  const GroupStatsArena& a = b.a;
  const uint32_t m = static_cast<uint32_t>(b.order.size()), T = b.T;
  SmpcDev* hd = g->arr.h_dev();
  SmpcWaveGeom* hg = g->arr.h_geo();
  SmpcDev* hfd = g->arr.h_fdev();
  SmpcWaveGeom* hfg = g->arr.h_fgeo();
  SmpcStatsDst* hdst = g->arr.h_sdst();
  SmpcStatsReduceArgs* hred = g->arr.h_sred();
  float* d_stats = g->stats.d_stats.get();
  b.bufs.assign(m, StatsBufs{});
  b.block = pass_block(b.c0->R);
  for (uint32_t j = 0; j < m; ++j) {
    smpc_ctx* c = g->ctxs[b.order[j]];
    StatsBufs& sb = b.bufs[j];
    sb.ld = a.ld[j];
    sb.rows = d_stats + a.rows[j];
    sb.costs = sb.rows + static_cast<size_t>(SMPC_STATS_ROWS) * sb.ld;
    sb.furthest = d_stats + a.furthest + 4 * j;
    sb.out = reinterpret_cast<SmpcStatsOut*>(d_stats + a.out + a.out_floats * j);
    sb.partials = d_stats + a.partials + a.partial_floats * j;
    sb.part = g->stats.d_part.get() + a.part[j];
    const PassGeom& pg = c->plan.wave;   // planned for every tick, whatever pass the tick itself takes
    const bool need_f = (b.flags[b.order[j]] & SD_NEED_FURTHEST) != 0;
    if (need_f) {
      // (launch_furthest's parameter block and carve-up, its word this member's own)
      SmpcDev& d = hfd[b.nf];
      d = c->dev;
      const int rc = use_limited_noise(c, d, false);
      if (rc != SMPC_OK) return rc;
      d.flags = c->gate_flags & SD_NEED_FURTHEST;
      d.furthest_out = reinterpret_cast<uint32_t*>(sb.furthest);
      hfg[b.nf].lds = make_lds(0, c->P, T, b.block / 64, false);
      hfg[b.nf].grid = pg.grid;
      b.fgrid_max = std::max(b.fgrid_max, pg.grid);
      b.flds_max = std::max(b.flds_max, hfg[b.nf].lds.total);
      b.nf++;
    }
    // (score_rows' parameter block)
    SmpcDev& d = hd[j];
    d = c->dev;
    d.flags = b.flags[b.order[j]];
    d.d_furthest = need_f ? sb.furthest : nullptr;
    d.furthest_hint = 0;
    d.costs = sb.costs;
    d.costs_prev = nullptr;
    d.partials = sb.partials;
    d.tail = 0;
    {
      int rc = use_limited_noise(c, d, false);
      if (rc != SMPC_OK) return rc;
      rc = seed_own_costs(c, d);   // (a member with moving obstacles: its seed kernel on the group's stream, as in a round)
      if (rc != SMPC_OK) return rc;
    }
    hg[j].lds = pg.lds;
    hg[j].grid = pg.grid;
    b.grid_max = std::max(b.grid_max, pg.grid);
    b.lds_max = std::max(b.lds_max, pg.lds.total);
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
  return SMPC_OK;
}

// one memset, one hand-over, the launches, one copy back, one wait
static int breakdown_run(smpc_group* g, GroupBreakdown& b)
{
  smpc_ctx* c0 = b.c0;
  const GroupStatsArena& a = b.a;
  const uint32_t m = static_cast<uint32_t>(b.order.size());
  float* d_stats = g->stats.d_stats.get();
  HIPCK(c0, hipMemsetAsync(d_stats, 0, a.out * sizeof(float), g->stream));
  // (every member's last tick or breakdown was waited for: nothing reads the blocks)
  const int rc = group_hand_over(g, c0, b.order, g->arr.at.breakdown);
  if (rc != SMPC_OK) return rc;
  g->launched = true;
  if (b.nf)
    HIPCK(c0, stats_launch_furthest_many(b.k, g->arr.d_fdev(), g->arr.d_fgeo(), b.nf, b.fgrid_max, b.flds_max, b.block, g->stream));
  HIPCK(c0, stats_launch_many(b.k, g->arr.d_dev(), g->arr.d_geo(), g->arr.d_sdst(), m, b.grid_max, b.lds_max, b.block, g->stream));
  HIPCK(c0, stats_launch_reduce_many(g->arr.d_sred(), m, a.slices_max, g->stream));
  HIPCK(c0, hipMemcpyAsync(g->stats.h_out.get(), d_stats + a.furthest, b.back_floats() * sizeof(float), hipMemcpyDeviceToHost, g->stream));
  HIPCK(c0, hipStreamSynchronize(g->stream));
  g->launched = false;
  for (uint32_t i : b.order) g->ctxs[i]->launched = false;
  g->count.breakdown_batched += m;
  return SMPC_OK;
}

// per rider: the struct, the re-score of one that collides everywhere, the rows
static int breakdown_collect(smpc_group* g, GroupBreakdown& b)
{
  const GroupStatsArena& a = b.a;
  const float* h_out = g->stats.h_out.get();
  for (uint32_t j = 0; j < b.order.size(); ++j) {
    const uint32_t i = b.order[j];
    smpc_ctx* c = g->ctxs[i];
    SmpcStatsOut o;
    memcpy(&o, h_out + (a.out - a.furthest) + a.out_floats * j, sizeof(o));
    uint32_t fl = b.flags[i], S = 0;
    bool fail_flag = c->fail_in;
    if (fl & SD_NEED_FURTHEST) S = smpc_furthest_index(h_out[4 * j]);
    int rc = SMPC_OK;
    if (!c->fail_in && (fl & (SD_OBSTACLES | SD_COST)) && o.non_colliding == 0.0f) {
      // (critic_manager.cpp:70-73, as the single call: the rows are those of the tick's re-score)
      fail_flag = true;
      fl = fail_only_flags(c) & ~SD_STORE_TRAJ;
      S = 0;
      rc = score_rows(c, b.bufs[j], fl, nullptr, &o);
    }
    if (rc == SMPC_OK) {
      fill_stats(c, fl, S, fail_flag, o, &b.stats[i]);
      if (b.per_rollout && b.per_rollout[i]) rc = fetch_rows(c, b.bufs[j], b.per_rollout[i]);
    }
    b.status[i] = rc;
    if (rc == SMPC_ERR_DEVICE) return rc;
  }
  return SMPC_OK;
}

}  // namespace

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
  if (batched_members) *batched_members = g->count.breakdown_batched;
  if (single_members) *single_members = g->count.breakdown_single;
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
// that asked for them.  Every member is put back as it was found (Carried, MembersPutBack): on every
// way out behind breakdown_prepare, b's destructor does it.
int smpc_group_critic_breakdown(smpc_group* g, const smpc_tick_in* ins, const float* const* u_ins, const uint8_t* take,
                                smpc_critic_stats* stats, float* const* per_rollout, int32_t* status)
{
  if (!g || !ins || !u_ins || !stats || !status) return fail(nullptr, SMPC_ERR_INVALID, "null argument");
  GroupBreakdown b{ins, u_ins, take, stats, per_rollout, status};
  int rc = group_enter(g, take, &b.c0);
  if (rc != SMPC_OK) return rc;
  if (!b.c0) return fail(nullptr, SMPC_ERR_INVALID, "critic breakdown: no member of the group is taken");
  b.n = static_cast<uint32_t>(g->ctxs.size());
  b.T = b.c0->cfg.time_steps;
  b.k = stats_many_select(b.c0->R, b.T);
  if (!b.k) return breakdown_one_by_one(g, b);
  rc = breakdown_prepare(g, b);
  if (rc != SMPC_OK || b.order.empty()) return rc;
  rc = breakdown_buffers(g, b);
  if (rc == SMPC_OK) rc = breakdown_fill(g, b);
  if (rc == SMPC_OK) rc = breakdown_run(g, b);
  if (rc == SMPC_OK) rc = breakdown_collect(g, b);
  if (rc != SMPC_OK) return rc;
  b.put_back.wait = false;   // (the success path: the call has waited, in breakdown_run)
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
