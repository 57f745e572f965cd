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
  g->slot = align_up(static_cast<uint32_t>(c0->tick.cap), 256);
  g->off_dev = g->slot * n;
  g->off_red = g->off_dev + align_up(static_cast<uint32_t>(sizeof(SmpcDev)) * n, 256);
  g->off_geo = g->off_red + align_up(static_cast<uint32_t>(sizeof(SmpcReduceArgs)) * n, 256);
  g->off_mov = g->off_geo + align_up(static_cast<uint32_t>(sizeof(SmpcWaveGeom)) * n, 256);
  g->total = g->off_mov + align_up(static_cast<uint32_t>(sizeof(SmpcMovingMember)) * n, 256);
  // behind what a round hands over: the further argument arrays of smpc_group_critic_breakdown
  g->off_fdev = g->total;
  g->off_fgeo = g->off_fdev + align_up(static_cast<uint32_t>(sizeof(SmpcDev)) * n, 256);
  g->off_sdst = g->off_fgeo + align_up(static_cast<uint32_t>(sizeof(SmpcWaveGeom)) * n, 256);
  g->off_sred = g->off_sdst + align_up(static_cast<uint32_t>(sizeof(SmpcStatsDst)) * n, 256);
  g->total_stats = g->off_sred + align_up(static_cast<uint32_t>(sizeof(SmpcStatsReduceArgs)) * n, 256);
  if (g->h_all.ensure(g->total_stats) != hipSuccess || g->d_all.ensure(g->total_stats) != hipSuccess) {
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
    c->tick.h_tick = g->h_all.get() + g->slot * i;
    c->tick.d_tick = g->d_all.get() + g->slot * i;
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
  if (batched_launches) *batched_launches = g->batched_launches;
  if (single_ticks) *single_ticks = g->single_ticks;
  return SMPC_OK;
}

// One tick of every member taken (take == null: of every member).  The members that can take a batched launch with a speculated furthest
// point (the steady state) are partitioned by the scoring instance their own plan chose:
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
  const uint32_t n = static_cast<uint32_t>(g->ctxs.size());
  auto taken = [&](uint32_t i) {return !take || take[i] != 0;};
  uint32_t first = 0;
  while (first < n && !taken(first)) ++first;
  if (first == n) return SMPC_OK;   // nobody taken: nothing to do
  smpc_ctx* c0 = g->ctxs[first];    // (errors of the round as a whole are reported on the first member taken)
  HIPCK(c0, hipSetDevice(c0->device));
  if (g->launched) {
    // the round before was abandoned between its launch and its last fetch_out: its kernels may
    // still read the tick blocks and the argument arrays this round is about to write
    HIPCK(c0, hipStreamSynchronize(g->stream));
    g->launched = false;
  }
  auto single = [&](uint32_t i) -> int {
    smpc_ctx* c = g->ctxs[i];
    c->defer_upload = false;   // its own upload, into its slot of the group's buffers
    const int rc = smpc_optimize(c, &ins[i], u_inout[i], outs ? &outs[i] : nullptr);
    c->defer_upload = true;
    g->single_ticks++;
    return rc;
  };
  static const bool timing = getenv("SMPC_GROUP_TIMING") != nullptr;
  auto now = [] {return std::chrono::steady_clock::now();};
  auto us_between = [](auto a, auto b) {return std::chrono::duration<double, std::micro>(b - a).count();};
  const auto t_start = now();
  const uint32_t T = c0->cfg.time_steps;
  // ---- prepare every member; decide which launch, if any, it rides ------------------------
  // part[i]: null — ticked alone; the grouped lane instance's address for every lane member; the
  // member's row of smpc_pass_many for a wave member
  std::vector<const void*> part(n, nullptr);
  std::vector<uint32_t> flags(n);
  bool lane_ok = true;
  uint32_t lane_first = n, Pmax = 0, window_bytes = 0, gridx = 0;
  const LaneInst* inst = nullptr;   // the grouped lane instance: one for all lane members
  static const char kLaneTag = 0;   // (stands for "the lane launch" until the instance is known)
  for (uint32_t i = 0; i < n; ++i) {
    if (!taken(i)) continue;
    smpc_ctx* c = g->ctxs[i];
    if (!u_inout[i]) return fail(c, SMPC_ERR_INVALID, "null control sequence");
    int rc = begin_tick(c, &ins[i], u_inout[i]);
    if (rc != SMPC_OK) return rc;
    flags[i] = scoring_flags(c, c->fail_in);
    const bool need_f = (flags[i] & SD_NEED_FURTHEST) != 0;
    if (need_f) flags[i] |= SD_LOCAL_FURTHEST;
    // what every batched launch asks of a member: one iteration scored once with a predicted
    // furthest point, the completion polled, no Ackermann launch behind the reduction, one
    // non-colliding count
    const bool ok = c->cfg.iteration_count == 1 && !c->fail_in &&
      !(c->cfg.flags & (SMPC_FLAG_NO_SPECULATION | SMPC_FLAG_PROFILE)) && (!need_f || c->pred.hint_valid) &&
      c->knobs.poll && c->acker_r < 0.f && !c->two_coll_fp;
    if (!ok) continue;
    // (a near-goal member scores GoalAngle: instances of the lane pass the batched launch does not
    // have; members with the deployed critic list — Constraint / Cost / Twirling — have theirs, and
    // a member without those critics runs them unchanged; a member that scores with cost powers
    // has no batched instance either and is ticked on its own)
    const LaneInst* k = c->plan.kind == PassPlan::kLane && !c->plan.rr && !c->plan.pow
      ? lane_select(flags[i], T, false, true, c->acker_r, false) : nullptr;
    if (k) {
      part[i] = &kLaneTag;
      if (lane_first == n) {
        lane_first = i;
        window_bytes = c->plan.window_bytes;
      }
      // the lane members agree on the window, the block and on whether a costmap lookup is scored
      else if (c->plan.window_bytes != window_bytes || (inst && k->obst != inst->obst) ||
               c->plan.lane.block != g->ctxs[lane_first]->plan.lane.block)
        lane_ok = false;
      if (!inst || k->dep) inst = k;
      Pmax = std::max(Pmax, c->P);
      gridx = std::max(gridx, c->plan.lane.grid);
      continue;
    }
    // its own plan chose the wave pass: the grouped row of the same <R, MODE, FULL> (R = 1 and the
    // lean modes only: wave_select has no other grouped row).  The in-launch reduction experiment
    // waits for the grid's other blocks; smpc_pass_many never does.
    if (c->plan.kind == PassPlan::kWave && c->R == 1 && !c->knobs.fused_reduce)
      part[i] = wave_select(c->R, c->score_mode, T, true);
  }
  SmpcLds L{};
  if (lane_first != n) {
    L = lane_lds(window_bytes, Pmax, T);
    if (L.total > kLdsPerCu) lane_ok = false;
  }
  // batched members in launch order: the lane members, then the wave members instance by instance
  struct Launch { const WaveInst* wave; uint32_t first, count, grid, lds; };   // wave == null: the lane launch
  std::vector<uint32_t> order;
  std::vector<Launch> launches;
  if (lane_first != n && lane_ok) {
    launches.push_back({nullptr, 0, 0, gridx, L.total});
    for (uint32_t i = 0; i < n; ++i)
      if (part[i] == &kLaneTag) order.push_back(i);
    launches.back().count = static_cast<uint32_t>(order.size());
  }
  for (uint32_t i = 0; i < n; ++i) {
    if (!part[i] || part[i] == &kLaneTag) continue;
    bool seen = false;
    for (const Launch& l : launches) seen = seen || l.wave == part[i];
    if (seen) continue;
    Launch l{static_cast<const WaveInst*>(part[i]), static_cast<uint32_t>(order.size()), 0, 0, 0};
    for (uint32_t j = i; j < n; ++j) {
      if (part[j] != part[i]) continue;
      order.push_back(j);
      l.count++;
      l.grid = std::max(l.grid, g->ctxs[j]->plan.wave.grid);
      l.lds = std::max(l.lds, g->ctxs[j]->plan.wave.lds.total);
    }
    if (l.count >= 2) launches.push_back(l);
    else order.pop_back();   // alone on its instance: ticked alone
  }
  // ---- everybody else is ticked alone, first ------------------------------------------------
  {
    std::vector<bool> rides(n, false);
    for (uint32_t i : order) rides[i] = true;
    for (uint32_t i = 0; i < n; ++i) {
      if (rides[i] || !taken(i)) continue;
      const int rc = single(i);
      if (rc != SMPC_OK) return rc;
    }
  }
  if (order.empty()) return SMPC_OK;
  const uint32_t m = static_cast<uint32_t>(order.size());
  const auto t_prep = now();
  // ---- one upload, one scoring launch per instance, one reduction launch ---------------------
  SmpcDev* hd = reinterpret_cast<SmpcDev*>(g->h_all.get() + g->off_dev);
  SmpcReduceArgs* hr = reinterpret_cast<SmpcReduceArgs*>(g->h_all.get() + g->off_red);
  SmpcWaveGeom* hg = reinterpret_cast<SmpcWaveGeom*>(g->h_all.get() + g->off_geo);
  // the riding members with moving obstacles, by the form of smpc_moving_cost their pass's layout asks for
  std::vector<SmpcMovingMember> mov[SMPC_MOVING_FORMS];
  for (const Launch& l : launches) {
    for (uint32_t j = l.first; j < l.first + l.count; ++j) {
      const uint32_t i = order[j];
      smpc_ctx* c = g->ctxs[i];
      if (l.wave) {
        const int rc = ensure_row_major(c);   // the wave-per-rollout pass reads the [B,T] tensors
        if (rc != SMPC_OK) return rc;
      }
      SmpcFinal fin;
      fill_score_args(c, flags[i], nullptr, nullptr, c->pred.hint, true, nullptr, hd[j], fin);
      {
        // a member with acceleration limits: its limiter goes out here, on the group's stream (c->stream
        // while grouped) ahead of the grouped pass, and its parameter block points at the limited noise
        int rc = use_limited_noise(c, hd[j], !l.wave);
        if (rc != SMPC_OK) return rc;
        // a member with moving obstacles keeps riding the batched launch (SD_COST_SEED is set behind
        // the choice of the instance); its seed comes from the group's ONE smpc_moving_cost_*_many
        // launch per form, behind the hand-over: here only its arguments
        SmpcMovingMember mm;
        SmpcMovingForm form;
        bool filled = false;
        rc = g->moving_per_member ? use_moving_seed(c, hd[j], !l.wave)
                                  : fill_moving_member(c, hd[j], !l.wave, &mm, &form, &filled);
        if (rc != SMPC_OK) return rc;
        if (filled) mov[form].push_back(mm);
      }
      hr[j].partials = c->d_partials.get();
      hr[j].tuple = c->d_tuple.get();
      // (a wave member: its own grid — the blocks beyond it wrote nothing; the lane launch: every
      // member's blocks write a partial)
      hr[j].nblk = l.wave ? c->plan.wave.grid : gridx;
      hr[j].host_out = fin.u_host;
      hr[j].seq = fin.seq;
      hr[j].neg_inv_temp = c->dev.neg_inv_temp;   // (its own: the members share the horizon, nothing else)
      fin.u_host = nullptr;          // one publishing block for the whole group instead
      fin.done_counter = nullptr;
      hr[j].fin = fin;
      hg[j].lds = c->plan.wave.lds;
      hg[j].grid = c->plan.wave.grid;
      c->passes++;
      c->last_pass_kind = l.wave ? PassPlan::kWave : PassPlan::kLane;
    }
  }
  // the moving-obstacle arguments form by form, one run per launch
  SmpcMovingMember* hm = reinterpret_cast<SmpcMovingMember*>(g->h_all.get() + g->off_mov);
  {
    uint32_t at = 0;
    for (const auto& v : mov) {
      if (!v.empty()) memcpy(hm + at, v.data(), v.size() * sizeof(SmpcMovingMember));
      at += static_cast<uint32_t>(v.size());
    }
  }
  // one hand-over for every riding member's tick block and parameter block: CPU stores through the
  // BAR (every member's last tick was fetched: nothing reads the buffer), else a copy on the stream
  if (c0->tick.bar_tick) {
    // (only what this tick wrote: a slot is sized for the longest path, 25 KB, a tick fills ~4)
    for (uint32_t i : order) bar_copy(g->d_all.get() + g->slot * i, g->h_all.get() + g->slot * i, g->ctxs[i]->tick.used);
    bar_copy(g->d_all.get() + g->off_dev, g->h_all.get() + g->off_dev, g->total - g->off_dev);
    bar_flush(c0);
  }
  else HIPCK(c0, hipMemcpyAsync(g->d_all.get(), g->h_all.get(), g->total, hipMemcpyHostToDevice, g->stream));
  // the moving-obstacle term of every riding member that has one: behind the hand-over (u is read
  // from the tick blocks it delivered), in front of the scoring launches (they start from the seed);
  // at most one launch per form, however many members
  {
    const SmpcMovingMember* d_mov = reinterpret_cast<const SmpcMovingMember*>(g->d_all.get() + g->off_mov);
    uint32_t at = 0;
    for (int f = 0; f < SMPC_MOVING_FORMS; ++f) {
      const uint32_t count = static_cast<uint32_t>(mov[f].size());
      if (!count) continue;
      uint32_t grid = 0;
      for (const SmpcMovingMember& mm : mov[f]) grid = std::max(grid, mm.grid);
      HIPCK(c0, smpc_launch_moving_cost_many(d_mov + at, count, grid, static_cast<SmpcMovingForm>(f), T, g->stream));
      g->launched = true;
      g->moving_launches++;
      at += count;
    }
  }
  // (the footprint tables of a MODE 4 member and the collision table of any member went out in
  // prepare_tick on c->stream, which is this stream while the context is grouped: in front of these)
  for (const Launch& l : launches) {
    const SmpcDev* d_dev = reinterpret_cast<const SmpcDev*>(g->d_all.get() + g->off_dev) + l.first;
    if (l.wave) {
      HIPCK(c0, wave_launch_many(l.wave, d_dev, reinterpret_cast<const SmpcWaveGeom*>(g->d_all.get() + g->off_geo) + l.first,
                                 l.count, l.grid, l.lds, pass_block(1), g->stream));
    } else {
      HIPCK(c0, lane_launch(inst, c0->dev, d_dev, l.count, L, l.grid, g->ctxs[lane_first]->plan.lane.block, g->stream));
    }
    g->launched = true;
    if (l.count >= 2) g->batched_launches++;
  }
  HIPCK(c0, smpc_launch_reduce_many(reinterpret_cast<const SmpcReduceArgs*>(g->d_all.get() + g->off_red), m,
                                    T, g->stream));
  g->batched_ticks++;
  const auto t_launch = now();
  // ---- per member: wait, verify the speculation and the collision count --------------------
  for (uint32_t i : order) {
    smpc_ctx* c = g->ctxs[i];
    int rc = fetch_out(c);
    if (rc != SMPC_OK) return rc;
    const bool need_f = (flags[i] & SD_NEED_FURTHEST) != 0;
    const TickResult res = tick_result(c);
    const float F_true = res.F_local();
    const uint32_t S_true = smpc_furthest_index(F_true);
    const bool miss = need_f && S_true != c->pred.hint;
    const bool all_collide = (flags[i] & (SD_OBSTACLES | SD_COST)) && res.non_colliding() == 0.0f;
    if (miss || all_collide) {
      if (miss) {
        c->spec_misses++;
        remember_furthest(c, &ins[i], F_true);   // smpc_optimize speculates with the true value now: one pass
        c->pred.hint_F = F_true;                      // (not the smoothed estimate a fresh-noise tick leaves)
        c->pred.hint_is_this_ticks = true;
      }
      rc = single(i);
      if (rc != SMPC_OK) return rc;
      if (outs) outs[i].passes++;    // the batched scoring this member took part in counts
      continue;
    }
    if (need_f) remember_furthest(c, &ins[i], F_true);   // as smpc_optimize does: the predictor's state advances every tick
    store_control_sequence(c, u_inout[i]);
    // (no fail flag: such a member was ticked alone; score_pass_ms 0: a profiling member never rides)
    rc = fill_tick_out(c, outs ? &outs[i] : nullptr, false, need_f, need_f ? S_true : 0u);
    if (rc != SMPC_OK) return rc;
  }
  g->launched = false;   // every riding member's fetch_out has returned
  if (timing && (g->batched_ticks % 64) == 0)
    fprintf(stderr, "[smpc_group] prepare %.1f us, fill+launch %.1f us, wait+collect %.1f us; batched %llu single %llu\n",
            us_between(t_start, t_prep), us_between(t_prep, t_launch), us_between(t_launch, now()),
            (unsigned long long)g->batched_ticks, (unsigned long long)g->single_ticks);
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
  auto taken = [&](uint32_t i) {return !take || take[i] != 0;};
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
  HIPCK(c0, g->mov_tab.ensure(cap));
  for (auto& st : g->mov_stage) HIPCK(c0, st.ensure(cap));
  HIPCK(c0, g->mov_ev_up.ensure(hipEventDisableTiming));
  g->mov_at.resize(n, 0);
  g->mov_used.resize(n, 0);
  for (uint32_t i = 0; i < n; ++i) {
    if (!taken(i) || n_discs[i] == 0) continue;
    smpc_ctx* c = g->ctxs[i];
    HIPCK(c, c->mov.hit.ensure(c->cfg.batch_size));
    HIPCK(c, c->mov.m.ensure(c->cfg.batch_size));
  }
  // the upload before this one may still be reading its staging buffer (and the one before that is
  // older still: the buffer written now)
  if (g->mov_up_recorded) HIPCK(c0, hipEventSynchronize(g->mov_ev_up.get()));
  // The tables back to back in member order, each region 16-byte aligned, in the staging buffer the
  // last upload did not read: a member taken gets its new table, a member not taken whose table
  // lives in the group's buffer keeps it — its packed bytes move over from the other staging buffer
  // and travel again, so that the whole is ONE run.
  const float* src = g->mov_stage[g->mov_cur].get();
  float* dst = g->mov_stage[g->mov_cur ^ 1].get();
  size_t at = 0;
  for (uint32_t i = 0; i < n; ++i) {
    smpc_ctx* c = g->ctxs[i];
    float* tk = g->mov_tab.get() + at;
    if (taken(i)) {
      if (n_discs[i] == 0) {
        moving_off(c);
        continue;
      }
      pack_moving_table(dst + at, T, &params[i], xy[i], radius[i], n_discs[i]);
      g->mov_used[i] = moving_table_floats(T, n_discs[i]);
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
      memcpy(dst + at, src + g->mov_at[i], g->mov_used[i] * sizeof(float));
      c->mov.tab_kt = tk + (c->mov.tab_kt - c->mov.tk);
      c->mov.disc = tk + (c->mov.disc - c->mov.tk);
      c->mov.tk = tk;
    } else {
      continue;
    }
    g->mov_at[i] = at;
    at += g->mov_used[i];
  }
  g->mov_cur ^= 1;
  HIPCK(c0, hipMemcpyAsync(g->mov_tab.get(), dst, at * sizeof(float), hipMemcpyHostToDevice, g->stream));
  HIPCK(c0, hipEventRecord(g->mov_ev_up.get(), g->stream));
  g->mov_up_recorded = true;
  g->moving_uploads++;
  return SMPC_OK;
}

int smpc_debug_group_moving_per_member(smpc_group* g, int on)
{
  if (!g) return SMPC_ERR_INVALID;
  g->moving_per_member = on != 0;
  return SMPC_OK;
}

int smpc_debug_group_moving_launches(const smpc_group* g, uint64_t* grouped_launches, uint64_t* table_uploads)
{
  if (!g) return SMPC_ERR_INVALID;
  if (grouped_launches) *grouped_launches = g->moving_launches;
  if (table_uploads) *table_uploads = g->moving_uploads;
  return SMPC_OK;
}

}  // extern "C"
