// smpc_stats.cpp — smpc_critic_breakdown (include/smpc.h): per-critic costs and effective samples
// of the tick smpc_optimize would run next.
//
// The tick is prepared exactly as smpc_optimize prepares it (prepare_tick: the same gates, tables
// and upload), scored by smpc_pass_stats — the general wave pass keeping every critic's term
// (smpc_wave_stats.hip) — into buffers of the breakdown's own, and reduced there.  What a tick
// carries over to the next one (the furthest-point predictor, the launch plan the prune table
// looks at, the counters) is put back before the call returns; costs, u and the result block are
// never written.

#include "smpc_ctx.h"

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

static int ensure_buffers(smpc_ctx* c)
{
  if (c->d_stats) return SMPC_OK;
  const uint32_t B = c->cfg.batch_size, T = c->cfg.time_steps;
  const uint32_t ld = align_up(B, 4);
  const StatsLayout l = stats_layout(ld, T);
  uint32_t slice = 0;
  const uint32_t S = stats_reduce_slices(B, &slice);
  HIPCK(c, stats_set_lds_limit(static_cast<int>(kLdsPerCu)));
  // (d_stats last: it marks the set complete — a call that failed half way picks up where it stopped)
  if (!c->d_stats_part)
    HIPCK(c, hipMalloc(&c->d_stats_part, static_cast<size_t>(SMPC_STATS_ROWS + 1) * S * 4 * sizeof(double)));
  for (hipEvent_t& e : c->ev_stats)
    if (!e) HIPCK(c, hipEventCreate(&e));
  c->stats_ld = ld;
  HIPCK(c, hipMalloc(&c->d_stats, l.total * sizeof(float)));
  return SMPC_OK;
}

// which rows the pass scored with these flags at furthest point S (the per-S gates it reads from
// the tick block, here from the block's host copy)
static uint32_t scored_rows(const smpc_ctx* c, uint32_t flags, uint32_t S)
{
  const uint32_t P = c->P;
  const TickLayout tl = tick_layout(c->cfg.time_steps, std::max(P, 1u));
  const uint8_t* h = c->h_tick;
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
static int score_rows(smpc_ctx* c, uint32_t flags, const float* d_furthest, SmpcStatsOut* o)
{
  const uint32_t T = c->cfg.time_steps, ld = c->stats_ld;
  const StatsLayout l = stats_layout(ld, T);
  float* base = c->d_stats;
  const bool prof = (c->cfg.flags & SMPC_FLAG_PROFILE) != 0;
  // rows the pass does not score hold zeros
  HIPCK(c, hipMemsetAsync(base, 0, l.partials * sizeof(float), c->stream));
  SmpcDev d = c->dev;
  d.flags = flags;
  d.d_furthest = d_furthest;
  d.furthest_hint = 0;
  d.costs = base + l.costs;
  d.costs_prev = nullptr;          // (never SD_ACCUMULATE: the first iteration)
  d.partials = base + l.partials;
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
  }
  c->launched = true;
  if (prof) HIPCK(c, hipEventRecord(c->ev_stats[0], c->stream));
  HIPCK(c, stats_launch(k, d, g.lds, base + l.rows, ld, g.grid, g.block, c->stream));
  if (prof) {
    HIPCK(c, hipEventRecord(c->ev_stats[1], c->stream));
    HIPCK(c, hipEventRecord(c->ev_stats[2], c->stream));
  }
  HIPCK(c, stats_launch_reduce(base + l.rows, ld, base + l.costs, d.B, d.k2, c->d_stats_part, base + l.partials, g.grid, T,
                               reinterpret_cast<SmpcStatsOut*>(base + l.out), c->stream));
  if (prof) HIPCK(c, hipEventRecord(c->ev_stats[3], c->stream));
  HIPCK(c, hipMemcpyAsync(o, base + l.out, sizeof(*o), hipMemcpyDeviceToHost, c->stream));
  HIPCK(c, hipStreamSynchronize(c->stream));
  c->launched = false;
  if (prof) {
    (void)hipEventElapsedTime(&c->stats_pass_ms, c->ev_stats[0], c->ev_stats[1]);
    (void)hipEventElapsedTime(&c->stats_reduce_ms, c->ev_stats[2], c->ev_stats[3]);
  }
  return SMPC_OK;
}

static int breakdown(smpc_ctx* c, const smpc_tick_in* in, const float* u_in, smpc_critic_stats* stats, float* per_rollout)
{
  int rc = prepare_tick(c, in, u_in);
  if (rc != SMPC_OK) return rc;
  if (c->two_coll_fp)
    return fail(c, SMPC_ERR_UNSUPPORTED,
                "critic breakdown: consider_footprint=true with both ObstaclesCritic and CostCritic in the list");
  rc = ensure_buffers(c);
  if (rc != SMPC_OK) return rc;
  const uint32_t B = c->cfg.batch_size, T = c->cfg.time_steps, ld = c->stats_ld;
  const StatsLayout l = stats_layout(ld, T);
  // the first iteration's flags (smpc_optimize), without the trajectory write-out: its tensors are the tick's
  uint32_t flags = scoring_flags(c, c->fail_in) & ~SD_STORE_TRAJ;
  bool fail_flag = c->fail_in;
  float* dF = nullptr;
  if (flags & SD_NEED_FURTHEST) {
    dF = c->d_stats + l.furthest;
    rc = launch_furthest(c, dF);
    if (rc != SMPC_OK) return rc;
  }
  SmpcStatsOut o{};
  rc = score_rows(c, flags, dF, &o);
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
    rc = score_rows(c, flags, nullptr, &o);
    if (rc != SMPC_OK) return rc;
  }
  memset(stats, 0, sizeof(*stats));
  stats->scored_mask = scored_rows(c, flags, S);
  stats->fail_flag = fail_flag ? 1u : 0u;
  stats->batch = B;
  stats->best_rollout = o.best_rollout;
  stats->best_cost = o.best_cost;
  stats->effective_samples = o.effective_samples;
  static_assert(sizeof(o.sum) == sizeof(stats->sum), "the device result's rows are the struct's");
  memcpy(stats->sum, o.sum, sizeof(o.sum));
  memcpy(stats->min, o.min, sizeof(o.min));
  memcpy(stats->max, o.max, sizeof(o.max));
  memcpy(stats->weighted, o.weighted, sizeof(o.weighted));
  memcpy(stats->at_best, o.at_best, sizeof(o.at_best));
  if (per_rollout)
    HIPCK(c, hipMemcpy2D(per_rollout, B * sizeof(float), c->d_stats + l.rows, ld * sizeof(float), B * sizeof(float),
                         SMPC_STATS_ROWS, hipMemcpyDeviceToHost));
  return SMPC_OK;
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
  Carried carried = save_carried(c);
  const int rc = breakdown(c, in, u_in, stats, per_rollout);
  if (rc != SMPC_OK && c->launched) {
    (void)hipStreamSynchronize(c->stream);   // nothing of an abandoned breakdown may run into the next tick
    c->launched = false;
  }
  restore_carried(c, carried);
  return rc;
}

// developer aid (SMPC_FLAG_PROFILE): GPU time of the last breakdown's scoring pass and of its
// reduction (both launches), by HIP events; of the re-score when every rollout collided
int smpc_debug_stats_ms(const smpc_ctx* c, float* pass_ms, float* reduce_ms)
{
  if (!c || !pass_ms || !reduce_ms) return SMPC_ERR_INVALID;
  *pass_ms = c->stats_pass_ms;
  *reduce_ms = c->stats_reduce_ms;
  return SMPC_OK;
}

}  // extern "C"
