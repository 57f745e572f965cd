// smpc_moving_host.cpp — host side of the moving obstacles (smpc_ctx.h: MovingObstacles; the kernel:
// smpc_moving.hip): the table's two forms and its upload (smpc_set_moving_obstacles), the seed
// kernel's launch in front of an iteration's first pass (use_moving_seed, seed_own_costs), the same
// for a group's riding member as arguments of the grouped launch (fill_moving_member), and the last
// tick's m and hits handed out.  The table's checks and layout are functions of their own, shared with
// smpc_group_set_moving_obstacles (smpc_group.cpp).

#include "smpc_ctx.h"
#include "../../include/smpc_debug.h"   // smpc_debug_moving_ms

namespace smpc_impl {

// The moving-obstacle kernel's launch for the pass about to go out with d: the noise d points at, in
// the layout that pass reads; m into `seed` (added to its content when d accumulates).
// the table went up on the stream the ctx had then: the one it has now waits for it (once).  (A
// group's table went up on the group's stream, which is the member's for as long as the table holds.)
int wait_table_upload(smpc_ctx* c)
{
  if (!c->mov.group_table && c->mov.up_recorded && c->mov.up_stream != c->stream) {
    HIPCK(c, hipStreamWaitEvent(c->stream, c->mov.ev_up.get(), 0));
    c->mov.up_stream = c->stream;
  }
  return SMPC_OK;
}

static int moving_cost(smpc_ctx* c, const SmpcDev& d, bool group_major, float* seed, float* m_out, uint8_t* hit_out)
{
  const uint32_t T = c->cfg.time_steps;
  SmpcMovingArgs a{};
  if (group_major) {
    a.n[0] = d.tvx; a.n[1] = c->holonomic ? d.tvy : nullptr; a.n[2] = d.twz;
    a.tab = c->mov.tk;
  } else {
    const int rc = ensure_row_major(c);
    if (rc != SMPC_OK) return rc;
    a.n[0] = d.nvx; a.n[1] = c->holonomic ? d.nvy : nullptr; a.n[2] = d.nwz;
    a.tab = c->mov.tab_kt;
  }
  {
    const int rc = wait_table_upload(c);
    if (rc != SMPC_OK) return rc;
  }
  a.disc = c->mov.disc;
  a.seed = seed; a.m_out = m_out; a.hit_out = hit_out;
  a.B = c->cfg.batch_size; a.T = T; a.K = c->mov.K;
  a.add = (d.flags & SD_ACCUMULATE) ? 1u : 0u;
  a.u_dev = c->lim.u_dev;   // the iteration's u: as the limiter takes it
  if (!a.u_dev) {
    const TickLayout tl = tick_layout(T, std::max(c->P, 1u));
    memcpy(a.u_arg, c->tick.h_tick + tl.u, 3 * T * sizeof(float));
  }
  a.x0 = d.x0; a.y0 = d.y0; a.yaw0 = d.yaw0; a.cos0 = d.cos0; a.sin0 = d.sin0; a.dt = d.dt;
  a.v0[0] = d.svx; a.v0[1] = d.svy; a.v0[2] = d.swz;
  a.collision_cost = c->mov.par.collision_cost;
  a.repulsion_weight = c->mov.par.repulsion_weight;
  a.margin = c->mov.par.margin;
  const bool prof = (c->cfg.flags & SMPC_FLAG_PROFILE) != 0;
  if (prof) {
    for (Event& e : c->mov.ev) HIPCK(c, e.ensure());
    HIPCK(c, hipEventRecord(c->mov.ev[0].get(), c->stream));
  }
  c->launched = true;
  HIPCK(c, smpc_launch_moving_cost(a, group_major, c->stream));
  if (prof) HIPCK(c, hipEventRecord(c->mov.ev[1].get(), c->stream));
  return SMPC_OK;
}

int use_moving_seed(smpc_ctx* c, SmpcDev& d, bool group_major)
{
  if (c->mov.K == 0) return SMPC_OK;
  if (c->fail_in) {
    c->mov.scored = false;   // this tick scores nothing: there is no "last tick's m" behind it
    return SMPC_OK;
  }
  if (c->lim.iter == 0) begin_limit_iteration(c, nullptr);
  if (c->mov.iter != c->lim.iter) {
    const int rc = moving_cost(c, d, group_major, const_cast<float*>(d.costs_prev), c->mov.m.get(), c->mov.hit.get());
    if (rc != SMPC_OK) return rc;
    c->mov.iter = c->lim.iter;
    c->mov.scored = true;
  }
  d.flags |= SD_COST_SEED;
  return SMPC_OK;
}

int fill_moving_member(smpc_ctx* c, SmpcDev& d, bool group_major, SmpcMovingMember* mm, SmpcMovingForm* form, bool* filled)
{
  *filled = false;
  if (c->mov.K == 0) return SMPC_OK;
  if (c->fail_in) {
    c->mov.scored = false;
    return SMPC_OK;
  }
  if (c->lim.iter == 0) begin_limit_iteration(c, nullptr);
  if (c->mov.iter != c->lim.iter) {
    const uint32_t B = c->cfg.batch_size, T = c->cfg.time_steps;
    SmpcMovingMember a{};
    if (group_major) {
      a.n[0] = d.tvx; a.n[1] = c->holonomic ? d.tvy : nullptr; a.n[2] = d.twz;
      a.tab = c->mov.tk;
      a.grid = ((B + 63u) / 64u + 3u) / 4u;
      *form = c->holonomic ? SMPC_MOVING_GM_VY : SMPC_MOVING_GM;
    } else {
      const int rc = ensure_row_major(c);
      if (rc != SMPC_OK) return rc;
      a.n[0] = d.nvx; a.n[1] = c->holonomic ? d.nvy : nullptr; a.n[2] = d.nwz;
      a.tab = c->mov.tab_kt;
      a.grid = (B + 3u) / 4u;
      *form = SMPC_MOVING_RM;
    }
    {
      const int rc = wait_table_upload(c);
      if (rc != SMPC_OK) return rc;
    }
    a.disc = c->mov.disc;
    a.seed = const_cast<float*>(d.costs_prev); a.m_out = c->mov.m.get(); a.hit_out = c->mov.hit.get();
    a.B = B; a.T = T; a.K = c->mov.K;
    a.add = (d.flags & SD_ACCUMULATE) ? 1u : 0u;
    // the iteration's u where the launch finds it: what the limiter was given, or the member's tick
    // block on the device — the floats moving_cost copies into u_arg, delivered by the hand-over
    a.u_dev = c->lim.u_dev;
    if (!a.u_dev) a.u_dev = reinterpret_cast<const float*>(c->tick.d_tick + tick_layout(T, std::max(c->P, 1u)).u);
    a.x0 = d.x0; a.y0 = d.y0; a.yaw0 = d.yaw0; a.cos0 = d.cos0; a.sin0 = d.sin0; a.dt = d.dt;
    a.v0[0] = d.svx; a.v0[1] = d.svy; a.v0[2] = d.swz;
    a.collision_cost = c->mov.par.collision_cost;
    a.repulsion_weight = c->mov.par.repulsion_weight;
    a.margin = c->mov.par.margin;
    *mm = a;
    *filled = true;
    c->launched = true;
    c->mov.iter = c->lim.iter;
    c->mov.scored = true;
  }
  d.flags |= SD_COST_SEED;
  return SMPC_OK;
}

int seed_own_costs(smpc_ctx* c, SmpcDev& d)
{
  if (c->mov.K == 0 || c->fail_in) return SMPC_OK;
  HIPCK(c, c->mov.stats_seed.ensure(c->cfg.batch_size));
  const int rc = moving_cost(c, d, false, c->mov.stats_seed.get(), nullptr, nullptr);
  if (rc != SMPC_OK) return rc;
  d.costs_prev = c->mov.stats_seed.get();
  d.flags |= SD_COST_SEED;
  return SMPC_OK;
}

void moving_off(smpc_ctx* c)
{
  c->mov.K = 0;
  c->mov.iter = 0;
  c->mov.scored = false;
  if (c->mov.group_table) {
    // the table was a group's: nothing of it is kept
    c->mov.group_table = false;
    c->mov.tk = c->mov.tab_kt = c->mov.disc = nullptr;
  }
}

int check_moving_table(smpc_ctx* c, const smpc_moving_obstacles_params* p, const float* xy, const float* radius, uint32_t n)
{
  if (n > SMPC_MAX_MOVING_OBSTACLES) return fail(c, SMPC_ERR_UNSUPPORTED, "more than SMPC_MAX_MOVING_OBSTACLES moving obstacles");
  if (!p || !xy || !radius) return fail(c, SMPC_ERR_INVALID, "null argument");
  if (!std::isfinite(p->collision_cost) || !std::isfinite(p->repulsion_weight) || !std::isfinite(p->margin) ||
      !(p->collision_cost >= 0.f) || !(p->repulsion_weight >= 0.f) || !(p->margin > 0.f))
    return fail(c, SMPC_ERR_INVALID, "moving obstacles: collision_cost >= 0, repulsion_weight >= 0, margin > 0, all finite");
  const uint32_t T = c->cfg.time_steps;
  if (T > SMPC_MOVING_MAX_T) return fail(c, SMPC_ERR_UNSUPPORTED, "moving obstacles: more than 256 time steps");
  for (uint32_t k = 0; k < n; ++k)
    if (!std::isfinite(radius[k]) || !(radius[k] > 0.f)) return fail(c, SMPC_ERR_INVALID, "moving obstacles: every radius must be finite and > 0");
  for (size_t i = 0; i < static_cast<size_t>(n) * T * 2; ++i)
    if (!std::isfinite(xy[i])) return fail(c, SMPC_ERR_INVALID, "moving obstacles: every centre must be finite");
  return SMPC_OK;
}

size_t moving_table_floats(uint32_t T, uint32_t n)
{
  const size_t n_tk = static_cast<size_t>(T) * n * 4, n_kt = (static_cast<size_t>(n) * T * 2 + 3) & ~static_cast<size_t>(3);
  return n_tk + n_kt + 4 * static_cast<size_t>(n);
}

size_t moving_table_capacity(uint32_t T)
{
  return static_cast<size_t>(SMPC_MAX_MOVING_OBSTACLES) * T * 6 + SMPC_MAX_MOVING_OBSTACLES * 4;
}

void pack_moving_table(float* tk, uint32_t T, const smpc_moving_obstacles_params* p, const float* xy, const float* radius, uint32_t n)
{
  const size_t n_tk = static_cast<size_t>(T) * n * 4, n_kt = (static_cast<size_t>(n) * T * 2 + 3) & ~static_cast<size_t>(3);
  float* kt = tk + n_tk;
  float* disc = kt + n_kt;
  for (uint32_t k = 0; k < n; ++k) {
    const float reach = radius[k] + p->margin;
    const float reach2 = reach * reach * SMPC_MOVING_REACH_GUARD;
    disc[4 * k + 0] = radius[k]; disc[4 * k + 1] = reach; disc[4 * k + 2] = reach2; disc[4 * k + 3] = 0.f;
    for (uint32_t t = 0; t < T; ++t) {
      const float x = xy[(static_cast<size_t>(k) * T + t) * 2], y = xy[(static_cast<size_t>(k) * T + t) * 2 + 1];
      float* e = tk + (static_cast<size_t>(t) * n + k) * 4;
      e[0] = x; e[1] = y; e[2] = reach2; e[3] = radius[k];
      kt[(static_cast<size_t>(k) * T + t) * 2] = x;
      kt[(static_cast<size_t>(k) * T + t) * 2 + 1] = y;
    }
  }
  for (size_t i = static_cast<size_t>(n) * T * 2; i < n_kt; ++i) kt[i] = 0.f;   // (the pairs' padding up to 16 bytes)
}

}  // namespace smpc_impl

using namespace smpc_impl;

extern "C" {

void smpc_moving_obstacles_params_default(smpc_moving_obstacles_params* p)
{
  if (!p) return;
  p->collision_cost = 10000.0f;
  p->repulsion_weight = 5.0f;
  p->margin = 0.5f;
  p->reserved = 0;
}

int smpc_set_moving_obstacles(smpc_ctx* c, const smpc_moving_obstacles_params* p, const float* xy, const float* radius, uint32_t n)
{
  if (!c) return SMPC_ERR_INVALID;
  if (n == 0) {
    // off: the buffers stay (a controller that clears and sets the table every few ticks), nothing reads them
    moving_off(c);
    return SMPC_OK;
  }
  {
    const int rc = check_moving_table(c, p, xy, radius, n);
    if (rc != SMPC_OK) return rc;
  }
  const uint32_t B = c->cfg.batch_size, T = c->cfg.time_steps;
  // Buffers, each checked on its own (a call that failed half way picks up where it stopped): the
  // table's three regions — [T][K] quads | [K][T] pairs | [K] disc constants — in ONE device
  // allocation sized for the most discs a table can hold, a pinned staging copy of the same size, and
  // the event behind the last upload.
  HIPCK(c, hipSetDevice(c->device));
  const size_t tab_floats = moving_table_capacity(T);
  HIPCK(c, c->mov.tab_tk.ensure(tab_floats));
  HIPCK(c, c->mov.stage.ensure(tab_floats));
  HIPCK(c, c->mov.ev_up.ensure(hipEventDisableTiming));
  HIPCK(c, c->mov.hit.ensure(B));
  HIPCK(c, c->mov.m.ensure(B));
  // the upload before this one may still be reading the staging copy
  if (c->mov.up_recorded) HIPCK(c, hipEventSynchronize(c->mov.ev_up.get()));
  // the table in the two forms the launches read (smpc_moving.h), then the disc constants: written
  // straight into the staging copy — this is the copy the call makes before it returns
  // (packed for THIS table, each region 16-byte aligned: the upload is one run)
  float* tk = c->mov.stage.get();
  pack_moving_table(tk, T, p, xy, radius, n);
  const size_t n_tk = static_cast<size_t>(T) * n * 4, n_kt = (static_cast<size_t>(n) * T * 2 + 3) & ~static_cast<size_t>(3);
  const size_t used = moving_table_floats(T, n);
  // ONE upload on the ctx's stream, behind whatever of the last tick still reads the table, nothing
  // waited for (a fleet's 15 neighbours at T = 56: 20 KB).  The next tick's kernel follows on the same
  // stream, or waits for the event where the ctx has changed streams since (a group formed or
  // dropped): moving_cost.
  HIPCK(c, hipMemcpyAsync(c->mov.tab_tk.get(), tk, used * sizeof(float), hipMemcpyHostToDevice, c->stream));
  c->mov.tk = c->mov.tab_tk.get();
  c->mov.tab_kt = c->mov.tk + n_tk;
  c->mov.disc = c->mov.tab_kt + n_kt;
  c->mov.group_table = false;   // (a group's table of this member: overridden — the last call wins)
  HIPCK(c, hipEventRecord(c->mov.ev_up.get(), c->stream));
  c->mov.up_recorded = true;
  c->mov.up_stream = c->stream;
  c->mov.par = *p;
  c->mov.K = n;
  c->mov.iter = 0;
  c->mov.scored = false;
  return SMPC_OK;
}

int smpc_get_moving_obstacle_costs(smpc_ctx* c, float* m, uint8_t* hit)
{
  if (!c || !m) return fail(c, SMPC_ERR_INVALID, "null argument");
  if (c->mov.K == 0) return fail(c, SMPC_ERR_STATE, "no moving-obstacle costs: the term is off");
  if (!c->mov.scored) return fail(c, SMPC_ERR_STATE, "no moving-obstacle costs: no tick has scored this table");
  HIPCK(c, hipSetDevice(c->device));
  HIPCK(c, hipStreamSynchronize(c->stream));
  HIPCK(c, hipMemcpy(m, c->mov.m.get(), c->cfg.batch_size * sizeof(float), hipMemcpyDeviceToHost));
  if (hit) HIPCK(c, hipMemcpy(hit, c->mov.hit.get(), c->cfg.batch_size, hipMemcpyDeviceToHost));
  return SMPC_OK;
}

// developer aid (SMPC_FLAG_PROFILE): GPU time of the last smpc_moving_cost launch, by HIP events
int smpc_debug_moving_ms(smpc_ctx* c, float* ms)
{
  if (!c || !ms || !c->mov.ev[0] || !c->mov.ev[1]) return SMPC_ERR_INVALID;
  HIPCK(c, hipSetDevice(c->device));
  HIPCK(c, hipEventSynchronize(c->mov.ev[1].get()));
  HIPCK(c, hipEventElapsedTime(ms, c->mov.ev[0].get(), c->mov.ev[1].get()));
  return SMPC_OK;
}

}  // extern "C"
