// smpc_group.cpp — several planning instances per launch (include/smpc.h smpc_group_*;
// BASELINE configs[4]: multi-robot fleets): one upload, one scoring launch, one reduction for a
// set of contexts.
#include "smpc_ctx.h"
#include "smpc_group.h"
#include "../../include/smpc_debug.h"   // smpc_debug_group_moving_launches

using namespace smpc_impl;

extern "C" {

int smpc_group_create(smpc_ctx* const* ctxs, uint32_t n, smpc_group** out)
{
  if (!ctxs || !n || !out) return fail(nullptr, SMPC_ERR_INVALID, "null argument");
  *out = nullptr;
  for (uint32_t i = 0; i < n; ++i) {
    if (!ctxs[i]) return fail(nullptr, SMPC_ERR_INVALID, "null ctx");
    if (ctxs[i]->device != ctxs[0]->device || ctxs[i]->cfg.time_steps != ctxs[0]->cfg.time_steps)
      return fail(nullptr, SMPC_ERR_INVALID, "a group's contexts share the device and time_steps");
    if (ctxs[i]->defer_upload) return fail(nullptr, SMPC_ERR_STATE, "ctx already in a group");
  }
  smpc_group* g = new (std::nothrow) smpc_group();
  if (!g) return fail(nullptr, SMPC_ERR_NOMEM, "out of memory");
  smpc_ctx* c0 = ctxs[0];
  if (hipSetDevice(c0->device) != hipSuccess) {
    delete g;
    return fail(nullptr, SMPC_ERR_DEVICE, "hipSetDevice");
  }
  GroupArrays& a = g->arr;
  a.at = group_layout(c0->tick.cap, n, GroupElemSizes{sizeof(SmpcDev), sizeof(SmpcReduceArgs), sizeof(SmpcWaveGeom),
                                                      sizeof(SmpcMovingMember), sizeof(SmpcStatsDst), sizeof(SmpcStatsReduceArgs)});
  if (a.h_all.ensure(a.at.breakdown) != hipSuccess || a.d_all.ensure(a.at.breakdown) != hipSuccess) {
    delete g;
    return fail(nullptr, SMPC_ERR_NOMEM, "group buffers");
  }
  g->stream = c0->own_stream.get();
  for (uint32_t i = 0; i < n; ++i) {
    smpc_ctx* c = ctxs[i];
    (void)hipStreamSynchronize(c->stream);
    g->ctxs.push_back(c);
    g->saved_stream.push_back(c->stream);
    c->stream = g->stream;
    c->tick.h_tick = a.h_slot(i);
    c->tick.d_tick = a.d_slot(i);
    c->defer_upload = true;
    c->in_group = true;
    c->lut_valid = false;
  }
  *out = g;
  return SMPC_OK;
}

void smpc_group_destroy(smpc_group* g)
{
  if (!g) return;
  (void)hipStreamSynchronize(g->stream);
  for (size_t i = 0; i < g->ctxs.size(); ++i) {
    smpc_ctx* c = g->ctxs[i];
    c->stream = g->saved_stream[i];
    c->tick.view_own();
    if (c->mov.group_table) moving_off(c);   // the table was the group's and goes with it
    c->defer_upload = false;
    c->in_group = false;
  }
  delete g;   // its buffers: their holders' destructors (smpc_own.h)
}

int smpc_group_stats(const smpc_group* g, uint64_t* batched_launches, uint64_t* single_ticks)
{
  if (!g) return SMPC_ERR_INVALID;
  if (batched_launches) *batched_launches = g->count.batched_launches;
  if (single_ticks) *single_ticks = g->count.single_ticks;
  return SMPC_OK;
}

}  // extern "C"

namespace smpc_impl {

int group_enter(smpc_group* g, const uint8_t* take, smpc_ctx** c0)
{
  const uint32_t n = static_cast<uint32_t>(g->ctxs.size());
  uint32_t first = 0;
  while (first < n && !group_takes(take, first)) ++first;
  *c0 = first < n ? g->ctxs[first] : nullptr;
  if (!*c0) return SMPC_OK;
  HIPCK(*c0, hipSetDevice((*c0)->device));
  if (g->launched) {
    // the round before was abandoned between its launch and its last fetch_out: its kernels may
    // still read the tick blocks and the argument arrays this call is about to write
    HIPCK(*c0, hipStreamSynchronize(g->stream));
    g->launched = false;
  }
  return SMPC_OK;
}

int group_hand_over(smpc_group* g, smpc_ctx* c0, const std::vector<uint32_t>& order, size_t extent)
{
  const GroupArrays& a = g->arr;
  if (c0->tick.bar_tick) {
    for (uint32_t i : order) bar_copy(a.d_slot(i), a.h_slot(i), g->ctxs[i]->tick.used);
    bar_copy(a.d_all.get() + a.at.dev, a.h_all.get() + a.at.dev, extent - a.at.dev);
    bar_flush(c0);
  }
  else HIPCK(c0, hipMemcpyAsync(a.d_all.get(), a.h_all.get(), extent, hipMemcpyHostToDevice, g->stream));
  return SMPC_OK;
}

namespace {

// ---- a round (smpc_group_optimize_some) in its stages: the state they hand on -------------------
struct Round {
  // the caller's arrays
  const smpc_tick_in* ins;
  float* const* u_inout;
  smpc_tick_out* outs;
  const uint8_t* take;
  smpc_ctx* c0 = nullptr;   // the first member taken
  uint32_t n = 0, T = 0;
  std::vector<GroupMemberPlan> mem;   // per member: what the partition is made from (round_prepare)
  std::vector<uint32_t> flags;        // per member: its scoring flags
  GroupPartition part;                // who rides which launch (group_partition)
  // the riding members with moving obstacles, by the form of smpc_moving_cost their pass's layout asks for (round_fill)
  std::vector<SmpcMovingMember> mov[SMPC_MOVING_FORMS];
  bool taken(uint32_t i) const {return group_takes(take, i);}
};

uint32_t lane_lds_total(uint32_t window_bytes, uint32_t Pmax, uint32_t T) {return lane_lds(window_bytes, Pmax, T).total;}

// member i on its own, with smpc_optimize
int tick_alone(smpc_group* g, Round& r, uint32_t i)
{
  smpc_ctx* c = g->ctxs[i];
  c->defer_upload = false;   // its own upload, into its slot of the group's buffers
  const int rc = smpc_optimize(c, &r.ins[i], r.u_inout[i], r.outs ? &r.outs[i] : nullptr);
  c->defer_upload = true;
  g->count.single_ticks++;
  return rc;
}

// prepare every member taken; note which launch, if any, its own plan lets it ride
int round_prepare(smpc_group* g, Round& r)
{
  r.mem.assign(r.n, GroupMemberPlan{});
  r.flags.assign(r.n, 0u);
  for (uint32_t i = 0; i < r.n; ++i) {
    if (!r.taken(i)) continue;
    smpc_ctx* c = g->ctxs[i];
    GroupMemberPlan& m = r.mem[i];
    m.taken = true;
    if (!r.u_inout[i]) return fail(c, SMPC_ERR_INVALID, "null control sequence");
    int rc = begin_tick(c, &r.ins[i], r.u_inout[i]);
    if (rc != SMPC_OK) return rc;
    r.flags[i] = scoring_flags(c, c->fail_in);
    const bool need_f = (r.flags[i] & SD_NEED_FURTHEST) != 0;
    if (need_f) r.flags[i] |= SD_LOCAL_FURTHEST;
    // what every batched launch asks of a member: one iteration scored once with a predicted
    // furthest point, the completion polled, no Ackermann launch behind the reduction, one
    // non-colliding count
    m.eligible = c->cfg.iteration_count == 1 && !c->fail_in &&
      !(c->cfg.flags & (SMPC_FLAG_NO_SPECULATION | SMPC_FLAG_PROFILE)) && (!need_f || c->pred.hint_valid) &&
      c->knobs.poll && c->acker_r < 0.f && !c->two_coll_fp;
    if (!m.eligible) continue;
    // (a near-goal member scores GoalAngle: instances of the lane pass the batched launch does not
    // have; members with the deployed critic list — Constraint / Cost / Twirling — have theirs, and
    // a member without those critics runs them unchanged; a member that scores with cost powers
    // has no batched instance either and is ticked on its own)
    const LaneInst* k = c->plan.kind == PassPlan::kLane && !c->plan.rr && !c->plan.pow
      ? lane_select(r.flags[i], r.T, false, true, c->acker_r, false) : nullptr;
    if (k) {
      m.lane = true;
      m.inst = k;
      m.grid = c->plan.lane.grid;
      m.window_bytes = c->plan.window_bytes;
      m.block = c->plan.lane.block;
      m.P = c->P;
      m.obst = k->obst;
      m.dep = k->dep;
      continue;
    }
    // its own plan chose the wave pass: the grouped row of the same <R, MODE, FULL> (R = 1 and the
    // lean modes only: wave_select has no other grouped row).  The in-launch reduction experiment
    // waits for the grid's other blocks; smpc_pass_many never does.
    if (c->plan.kind == PassPlan::kWave && c->R == 1 && !c->knobs.fused_reduce) {
      m.inst = wave_select(c->R, c->score_mode, r.T, true);
      m.grid = c->plan.wave.grid;
      m.lds = c->plan.wave.lds.total;
    }
  }
  return SMPC_OK;
}

// everybody taken who does not ride is ticked alone, first
int round_tick_others(smpc_group* g, Round& r)
{
  std::vector<bool> rides(r.n, false);
  for (uint32_t i : r.part.order) rides[i] = true;
  for (uint32_t i = 0; i < r.n; ++i) {
    if (rides[i] || !r.taken(i)) continue;
    const int rc = tick_alone(g, r, i);
    if (rc != SMPC_OK) return rc;
  }
  return SMPC_OK;
}

// the riders' parameter blocks, reduction arguments and wave geometry at their rider positions; the
// moving-obstacle members form by form
int round_fill(smpc_group* g, Round& r)
{
  SmpcDev* hd = g->arr.h_dev();
  SmpcReduceArgs* hr = g->arr.h_red();
  SmpcWaveGeom* hg = g->arr.h_geo();
  for (const GroupLaunch& l : r.part.launches) {
    for (uint32_t j = l.first; j < l.first + l.count; ++j) {
      const uint32_t i = r.part.order[j];
      smpc_ctx* c = g->ctxs[i];
      if (!l.lane) {
        const int rc = ensure_row_major(c);   // the wave-per-rollout pass reads the [B,T] tensors
        if (rc != SMPC_OK) return rc;
      }
      SmpcFinal fin;
      fill_score_args(c, r.flags[i], nullptr, nullptr, c->pred.hint, true, nullptr, hd[j], fin);
      {
        // a member with acceleration limits: its limiter goes out here, on the group's stream (c->stream
        // while grouped) ahead of the grouped pass, and its parameter block points at the limited noise
        int rc = use_limited_noise(c, hd[j], l.lane);
        if (rc != SMPC_OK) return rc;
        // a member with moving obstacles keeps riding the batched launch (SD_COST_SEED is set behind
        // the choice of the instance); its seed comes from the group's ONE smpc_moving_cost_*_many
        // launch per form, behind the hand-over: here only its arguments
        SmpcMovingMember mm;
        SmpcMovingForm form;
        bool filled = false;
        rc = g->mov.per_member ? use_moving_seed(c, hd[j], l.lane)
                               : fill_moving_member(c, hd[j], l.lane, &mm, &form, &filled);
        if (rc != SMPC_OK) return rc;
        if (filled) r.mov[form].push_back(mm);
      }
      hr[j].partials = c->d_partials.get();
      hr[j].tuple = c->d_tuple.get();
      // (a wave member: its own grid — the blocks beyond it wrote nothing; the lane launch: every
      // member's blocks write a partial)
      hr[j].nblk = l.lane ? r.part.lane.grid : c->plan.wave.grid;
      hr[j].host_out = fin.u_host;
      hr[j].seq = fin.seq;
      hr[j].neg_inv_temp = c->dev.neg_inv_temp;   // (its own: the members share the horizon, nothing else)
      fin.u_host = nullptr;          // one publishing block for the whole group instead
      fin.done_counter = nullptr;
      hr[j].fin = fin;
      hg[j].lds = c->plan.wave.lds;
      hg[j].grid = c->plan.wave.grid;
      c->passes++;
      c->last_pass_kind = l.lane ? PassPlan::kLane : PassPlan::kWave;
    }
  }
  // the moving-obstacle arguments form by form, one run per launch
  SmpcMovingMember* hm = g->arr.h_mov();
  uint32_t at = 0;
  for (const auto& v : r.mov) {
    if (!v.empty()) memcpy(hm + at, v.data(), v.size() * sizeof(SmpcMovingMember));
    at += static_cast<uint32_t>(v.size());
  }
  return SMPC_OK;
}

// behind the hand-over: the moving-obstacle term, one scoring launch per instance, ONE reduction
int round_launch(smpc_group* g, Round& r)
{
  smpc_ctx* c0 = r.c0;
  // the moving-obstacle term of every riding member that has one: behind the hand-over (u is read
  // from the tick blocks it delivered), in front of the scoring launches (they start from the seed);
  // at most one launch per form, however many members
  uint32_t at = 0;
  for (int f = 0; f < SMPC_MOVING_FORMS; ++f) {
    const uint32_t count = static_cast<uint32_t>(r.mov[f].size());
    if (!count) continue;
    uint32_t grid = 0;
    for (const SmpcMovingMember& mm : r.mov[f]) grid = std::max(grid, mm.grid);
    HIPCK(c0, smpc_launch_moving_cost_many(g->arr.d_mov(at), count, grid, static_cast<SmpcMovingForm>(f), r.T, g->stream));
    g->launched = true;
    g->count.moving_launches++;
    at += count;
  }
  // (the footprint tables of a MODE 4 member and the collision table of any member went out in
  // prepare_tick on c->stream, which is this stream while the context is grouped: in front of these)
  const GroupLaneCommon& lane = r.part.lane;
  for (const GroupLaunch& l : r.part.launches) {
    if (l.lane) {
      HIPCK(c0, lane_launch(static_cast<const LaneInst*>(l.inst), c0->dev, g->arr.d_dev(l.first), l.count,
                            lane_lds(lane.window_bytes, lane.Pmax, r.T), l.grid, lane.block, g->stream));
    } else {
      HIPCK(c0, wave_launch_many(static_cast<const WaveInst*>(l.inst), g->arr.d_dev(l.first), g->arr.d_geo(l.first), l.count, l.grid,
                                 l.lds, pass_block(1), g->stream));
    }
    g->launched = true;
    if (l.count >= 2) g->count.batched_launches++;
  }
  HIPCK(c0, smpc_launch_reduce_many(g->arr.d_red(), static_cast<uint32_t>(r.part.order.size()), r.T, g->stream));
  g->count.batched_ticks++;
  return SMPC_OK;
}

// per rider: wait, verify the speculation and the collision count; a miss or a member that collides
// everywhere is ticked again, alone
int round_collect(smpc_group* g, Round& r)
{
  for (uint32_t i : r.part.order) {
    smpc_ctx* c = g->ctxs[i];
    int rc = fetch_out(c);
    if (rc != SMPC_OK) return rc;
    const bool need_f = (r.flags[i] & SD_NEED_FURTHEST) != 0;
    const TickResult res = tick_result(c);
    const float F_true = res.F_local();
    const uint32_t S_true = smpc_furthest_index(F_true);
    const bool miss = need_f && S_true != c->pred.hint;
    const bool all_collide = (r.flags[i] & (SD_OBSTACLES | SD_COST)) && res.non_colliding() == 0.0f;
    if (miss || all_collide) {
      if (miss) {
        c->spec_misses++;
        remember_furthest(c, &r.ins[i], F_true);   // smpc_optimize speculates with the true value now: one pass
        c->pred.hint_F = F_true;                      // (not the smoothed estimate a fresh-noise tick leaves)
        c->pred.hint_is_this_ticks = true;
      }
      rc = tick_alone(g, r, i);
      if (rc != SMPC_OK) return rc;
      if (r.outs) r.outs[i].passes++;    // the batched scoring this member took part in counts
      continue;
    }
    if (need_f) remember_furthest(c, &r.ins[i], F_true);   // as smpc_optimize does: the predictor's state advances every tick
    store_control_sequence(c, r.u_inout[i]);
    // (no fail flag: such a member was ticked alone; score_pass_ms 0: a profiling member never rides)
    rc = fill_tick_out(c, r.outs ? &r.outs[i] : nullptr, false, need_f, need_f ? S_true : 0u);
    if (rc != SMPC_OK) return rc;
  }
  g->launched = false;   // every riding member's fetch_out has returned
  return SMPC_OK;
}

}  // namespace

}  // namespace smpc_impl

extern "C" {

// One tick of every member taken (take == null: of every member).  The members that can take a batched launch with a speculated furthest
// point (the steady state) are partitioned by the scoring instance their own plan chose (group_partition,
// smpc_group_layout.h):
//   * the members on the lane-per-rollout pass ride ONE launch of a grouped lane instance, as they
//     always did (they must agree on the window, the block and on whether a costmap lookup is scored;
//     if they do not, each is ticked on its own);
//   * the members on the wave-per-rollout pass in MODE 0, 3 or 4 (T <= 64: the deployed critic list
//     with or without consider_footprint, near-goal ticks, contexts created without the lane flag)
//     ride one launch of smpc_pass_many per distinct instance, each with the grid, the LDS carve-up
//     and so the rollout-to-wave assignment and flush group of its own smpc_pass launch; an instance
//     that only one member chose is not worth a launch of its own kind: that member is ticked alone.
// The group then issues ONE upload, those scoring launches and ONE reduction + publish launch for all
// of them.  A member that misses its speculation, collides everywhere, or is not eligible is ticked
// on its own with smpc_optimize — results are those of smpc_optimize in every case.
// A member that is not taken is not looked at: no prepare, no upload, no launch, no fetch; the
// partition above is the partition of the members taken.
int smpc_group_optimize_some(smpc_group* g, const smpc_tick_in* ins, float* const* u_inout,
                             smpc_tick_out* outs, const uint8_t* take)
{
  if (!g || !ins || !u_inout) return fail(nullptr, SMPC_ERR_INVALID, "null argument");
  Round r{ins, u_inout, outs, take};
  int rc = group_enter(g, take, &r.c0);
  if (rc != SMPC_OK || !r.c0) return rc;   // (nobody taken: nothing to do)
  r.n = static_cast<uint32_t>(g->ctxs.size());
  r.T = r.c0->cfg.time_steps;
  static const bool timing = getenv("SMPC_GROUP_TIMING") != nullptr;
  auto now = [] {return std::chrono::steady_clock::now();};
  auto us_between = [](auto a, auto b) {return std::chrono::duration<double, std::micro>(b - a).count();};
  const auto t_start = now();
  rc = round_prepare(g, r);
  if (rc != SMPC_OK) return rc;
  r.part = group_partition(r.mem.data(), r.n, r.T, lane_lds_total, kLdsPerCu);
  rc = round_tick_others(g, r);
  if (rc != SMPC_OK || r.part.order.empty()) return rc;
  const auto t_prep = now();
  rc = round_fill(g, r);
  if (rc == SMPC_OK) rc = group_hand_over(g, r.c0, r.part.order, g->arr.at.round);
  if (rc == SMPC_OK) rc = round_launch(g, r);
  if (rc != SMPC_OK) return rc;
  const auto t_launch = now();
  rc = round_collect(g, r);
  if (rc != SMPC_OK) return rc;
  if (timing && (g->count.batched_ticks % 64) == 0)
    fprintf(stderr, "[smpc_group] prepare %.1f us, fill+launch %.1f us, wait+collect %.1f us; batched %llu single %llu\n",
            us_between(t_start, t_prep), us_between(t_prep, t_launch), us_between(t_launch, now()),
            (unsigned long long)g->count.batched_ticks, (unsigned long long)g->count.single_ticks);
  return SMPC_OK;
}

int smpc_group_optimize(smpc_group* g, const smpc_tick_in* ins, float* const* u_inout,
                        smpc_tick_out* outs)
{
  return smpc_group_optimize_some(g, ins, u_inout, outs, nullptr);
}

// smpc_set_moving_obstacles for every member taken, with ONE staging fill, ONE upload and ONE event
// for all of them.  Every member is checked before anything is written.
int smpc_group_set_moving_obstacles(smpc_group* g, const smpc_moving_obstacles_params* params, const float* const* xy,
                                    const float* const* radius, const uint32_t* n_discs, const uint8_t* take)
{
  if (!g) return SMPC_ERR_INVALID;
  if (!n_discs) return fail(nullptr, SMPC_ERR_INVALID, "null argument");
  const uint32_t n = static_cast<uint32_t>(g->ctxs.size());
  // (not group_enter: errors of this call are reported on member 0, taken or not, and it writes
  // neither the tick blocks nor the argument arrays an abandoned round may still read)
  auto taken = [&](uint32_t i) {return group_takes(take, i);};
  bool any = false;
  for (uint32_t i = 0; i < n; ++i) {
    if (!taken(i) || n_discs[i] == 0) continue;
    smpc_ctx* c = g->ctxs[i];
    const int rc = (!params || !xy || !radius) ? fail(c, SMPC_ERR_INVALID, "null argument")
                                               : check_moving_table(c, &params[i], xy[i], radius[i], n_discs[i]);
    if (rc != SMPC_OK) {
      (void)fail(nullptr, rc, "smpc_group_set_moving_obstacles: member " + std::to_string(i) + ": " + c->err);
      return rc;
    }
    any = true;
  }
  smpc_ctx* c0 = g->ctxs[0];
  const uint32_t T = c0->cfg.time_steps;
  if (!any) {
    // nothing to upload: the members taken switch their term off, the others keep their tables
    for (uint32_t i = 0; i < n; ++i)
      if (taken(i)) moving_off(g->ctxs[i]);
    return SMPC_OK;
  }
  // buffers first: a call that fails here has changed no member either
  HIPCK(c0, hipSetDevice(c0->device));
  const size_t cap = moving_table_capacity(T) * n;
  HIPCK(c0, g->mov.tab.ensure(cap));
  for (auto& st : g->mov.stage) HIPCK(c0, st.ensure(cap));
  HIPCK(c0, g->mov.ev_up.ensure(hipEventDisableTiming));
  g->mov.at.resize(n, 0);
  g->mov.used.resize(n, 0);
  for (uint32_t i = 0; i < n; ++i) {
    if (!taken(i) || n_discs[i] == 0) continue;
    smpc_ctx* c = g->ctxs[i];
    HIPCK(c, c->mov.hit.ensure(c->cfg.batch_size));
    HIPCK(c, c->mov.m.ensure(c->cfg.batch_size));
  }
  // the upload before this one may still be reading its staging buffer (and the one before that is
  // older still: the buffer written now)
  if (g->mov.up_recorded) HIPCK(c0, hipEventSynchronize(g->mov.ev_up.get()));
  // The tables back to back in member order, each region 16-byte aligned, in the staging buffer the
  // last upload did not read: a member taken gets its new table, a member not taken whose table
  // lives in the group's buffer keeps it — its packed bytes move over from the other staging buffer
  // and travel again, so that the whole is ONE run.
  const float* src = g->mov.stage[g->mov.cur].get();
  float* dst = g->mov.stage[g->mov.cur ^ 1].get();
  size_t at = 0;
  for (uint32_t i = 0; i < n; ++i) {
    smpc_ctx* c = g->ctxs[i];
    float* tk = g->mov.tab.get() + at;
    if (taken(i)) {
      if (n_discs[i] == 0) {
        moving_off(c);
        continue;
      }
      pack_moving_table(dst + at, T, &params[i], xy[i], radius[i], n_discs[i]);
      g->mov.used[i] = moving_table_floats(T, n_discs[i]);
      const size_t n_tk = static_cast<size_t>(T) * n_discs[i] * 4;
      const size_t n_kt = (static_cast<size_t>(n_discs[i]) * T * 2 + 3) & ~static_cast<size_t>(3);
      c->mov.tk = tk;
      c->mov.tab_kt = tk + n_tk;
      c->mov.disc = c->mov.tab_kt + n_kt;
      c->mov.group_table = true;
      c->mov.par = params[i];
      c->mov.K = n_discs[i];
      c->mov.iter = 0;
      c->mov.scored = false;
    } else if (c->mov.group_table) {
      memcpy(dst + at, src + g->mov.at[i], g->mov.used[i] * sizeof(float));
      c->mov.tab_kt = tk + (c->mov.tab_kt - c->mov.tk);
      c->mov.disc = tk + (c->mov.disc - c->mov.tk);
      c->mov.tk = tk;
    } else {
      continue;
    }
    g->mov.at[i] = at;
    at += g->mov.used[i];
  }
  g->mov.cur ^= 1;
  HIPCK(c0, hipMemcpyAsync(g->mov.tab.get(), dst, at * sizeof(float), hipMemcpyHostToDevice, g->stream));
  HIPCK(c0, hipEventRecord(g->mov.ev_up.get(), g->stream));
  g->mov.up_recorded = true;
  g->count.moving_uploads++;
  return SMPC_OK;
}

int smpc_debug_group_moving_per_member(smpc_group* g, int on)
{
  if (!g) return SMPC_ERR_INVALID;
  g->mov.per_member = on != 0;
  return SMPC_OK;
}

int smpc_debug_group_moving_launches(const smpc_group* g, uint64_t* grouped_launches, uint64_t* table_uploads)
{
  if (!g) return SMPC_ERR_INVALID;
  if (grouped_launches) *grouped_launches = g->count.moving_launches;
  if (table_uploads) *table_uploads = g->count.moving_uploads;
  return SMPC_OK;
}

}  // extern "C"
