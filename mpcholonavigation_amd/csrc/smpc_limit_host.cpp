// smpc_limit_host.cpp — host side of the acceleration limits (smpc_ctx.h: Limiter; the kernel:
// smpc_limit.hip): the setters, the limiter's launch in front of the first pass of an iteration that
// reads a layout (use_limited_noise), and the limited noise handed out.

#include "smpc_ctx.h"
#include "../../include/smpc_debug.h"   // smpc_debug_limit_ms

namespace smpc_impl {

void begin_limit_iteration(smpc_ctx* c, const float* u_dev)
{
  c->lim.u_dev = u_dev;
  if (++c->lim.iter == 0) ++c->lim.iter;
}

// The limiter's launch for one layout.  The buffers of that layout are allocated here, at the
// first tick that reads it.
static int limit_noise(smpc_ctx* c, bool group_major)
{
  const uint32_t B = c->cfg.batch_size, T = c->cfg.time_steps;
  SmpcLimitArgs a{};
  if (group_major) {
    const size_t ngm = SMPC_GM_ELEMS(B, T);
    if (!c->lim.l_gm) {
      HIPCK(c, c->lim.l_gm.ensure(3 * ngm));
      HIPCK(c, hipMemsetAsync(c->lim.l_gm.get(), 0, 3 * ngm * sizeof(float), c->stream));   // (vy of a non-holonomic model stays zero)
    }
    a.src[0] = c->noise.cur.tvx.get(); a.src[1] = c->holonomic ? c->noise.cur.tvy : nullptr; a.src[2] = c->noise.cur.twz;
    a.dst[0] = c->lim.l_gm.get(); a.dst[1] = c->holonomic ? c->lim.l_gm.get() + ngm : nullptr; a.dst[2] = c->lim.l_gm.get() + 2 * ngm;
  } else {
    const int rc = ensure_row_major(c);
    if (rc != SMPC_OK) return rc;
    for (int k = 0; k < 3; ++k)
      if (k != 1 || c->holonomic) HIPCK(c, c->lim.l_rm[k].ensure(static_cast<size_t>(B) * T));
    a.src[0] = c->noise.cur.nvx.get(); a.src[1] = c->holonomic ? c->noise.cur.nvy.get() : nullptr; a.src[2] = c->noise.cur.nwz.get();
    for (int k = 0; k < 3; ++k) a.dst[k] = c->lim.l_rm[k].get();
  }
  a.B = B; a.T = T;
  a.u_dev = c->lim.u_dev;
  if (!a.u_dev) {
    // iteration 0: the control sequence as prepare_tick put it into the tick block's host copy
    // (vy row zeroed for a non-holonomic model), whichever way the block itself travels
    const TickLayout tl = tick_layout(T, std::max(c->P, 1u));
    memcpy(a.u_arg, c->tick.h_tick + tl.u, 3 * T * sizeof(float));
  }
  a.v0[0] = c->dev.svx; a.v0[1] = c->dev.svy; a.v0[2] = c->dev.swz;
  const float dt = c->cfg.model_dt;
  a.dhi[0] = dt * c->lim.lim[0]; a.dhi[1] = dt * c->lim.lim[2]; a.dhi[2] = dt * c->lim.lim[3];
  a.dlo[0] = dt * c->lim.lim[1]; a.dlo[1] = -a.dhi[1]; a.dlo[2] = -a.dhi[2];
  const bool prof = (c->cfg.flags & SMPC_FLAG_PROFILE) != 0;
  if (prof) {
    for (Event& e : c->lim.ev) HIPCK(c, e.ensure());
    HIPCK(c, hipEventRecord(c->lim.ev[0].get(), c->stream));
  }
  c->launched = true;
  HIPCK(c, smpc_launch_limit_noise(a, group_major, c->stream));
  if (prof) HIPCK(c, hipEventRecord(c->lim.ev[1].get(), c->stream));
  return SMPC_OK;
}

int use_limited_noise(smpc_ctx* c, SmpcDev& d, bool group_major)
{
  if (!c->lim.on) return SMPC_OK;
  uint32_t& have = group_major ? c->lim.gm_iter : c->lim.rm_iter;
  if (have != c->lim.iter || c->lim.iter == 0) {
    if (c->lim.iter == 0) begin_limit_iteration(c, nullptr);
    const int rc = limit_noise(c, group_major);
    if (rc != SMPC_OK) return rc;
    have = c->lim.iter;
  }
  if (group_major) {
    const size_t ngm = SMPC_GM_ELEMS(c->cfg.batch_size, c->cfg.time_steps);
    d.tvx = c->lim.l_gm.get(); d.tvy = c->lim.l_gm.get() + ngm; d.twz = c->lim.l_gm.get() + 2 * ngm;
  } else {
    d.nvx = c->lim.l_rm[0].get(); d.nwz = c->lim.l_rm[2].get();
    if (c->holonomic) d.nvy = c->lim.l_rm[1].get();   // (else: the stored zeros, untouched)
  }
  return SMPC_OK;
}

}  // namespace smpc_impl

using namespace smpc_impl;

extern "C" {

int smpc_set_acceleration_limits(smpc_ctx* c, float ax_max, float ax_min, float ay_max, float az_max)
{
  if (!c) return SMPC_ERR_INVALID;
  const bool off = ax_max == 0.f && ax_min == 0.f && ay_max == 0.f && az_max == 0.f;
  if (!off) {
    if (!std::isfinite(ax_max) || !std::isfinite(ax_min) || !std::isfinite(ay_max) || !std::isfinite(az_max))
      return fail(c, SMPC_ERR_INVALID, "acceleration limits must be finite");
    if (!(ax_max > 0.f) || !(ax_min < 0.f) || !(ay_max > 0.f) || !(az_max > 0.f))
      return fail(c, SMPC_ERR_INVALID, "acceleration limits: ax_max > 0, ax_min < 0, ay_max > 0, az_max > 0 (all four 0: off)");
  }
  c->lim.on = !off;
  c->lim.lim[0] = ax_max; c->lim.lim[1] = ax_min; c->lim.lim[2] = ay_max; c->lim.lim[3] = az_max;
  // what the buffers hold was made with the limits as they were: nothing to hand out until a tick ran
  c->lim.rm_iter = c->lim.gm_iter = 0;
  return SMPC_OK;
}

int smpc_get_acceleration_limits(const smpc_ctx* c, float out[4])
{
  if (!c || !out) return SMPC_ERR_INVALID;
  memcpy(out, c->lim.lim, sizeof(c->lim.lim));
  return SMPC_OK;
}

int smpc_get_limited_noise(smpc_ctx* c, float* nvx, float* nvy, float* nwz)
{
  if (!c) return SMPC_ERR_INVALID;
  if (!c->lim.on) return fail(c, SMPC_ERR_STATE, "no limited noise: the acceleration limits are off");
  const bool rm = c->lim.iter != 0 && c->lim.rm_iter == c->lim.iter;
  const bool gm = c->lim.iter != 0 && c->lim.gm_iter == c->lim.iter;
  if (!rm && !gm) return fail(c, SMPC_ERR_STATE, "no limited noise: no tick has run with these acceleration limits");
  HIPCK(c, hipSetDevice(c->device));
  const uint32_t B = c->cfg.batch_size, T = c->cfg.time_steps;
  const size_t n = static_cast<size_t>(B) * T * sizeof(float);
  if (!rm) {
    // the last iteration's passes read the group-major layout only: the [B,T] form is made from it
    const size_t ngm = SMPC_GM_ELEMS(B, T);
    for (int k = 0; k < 3; ++k) {
      if (k == 1 && !c->holonomic) continue;
      HIPCK(c, c->lim.l_rm[k].ensure(n / sizeof(float)));
      HIPCK(c, smpc_launch_relayout(c->lim.l_gm.get() + k * ngm, c->lim.l_rm[k].get(), B, T, false, c->stream));
    }
    c->lim.rm_iter = c->lim.iter;
  }
  HIPCK(c, hipStreamSynchronize(c->stream));
  if (nvx) HIPCK(c, hipMemcpy(nvx, c->lim.l_rm[0].get(), n, hipMemcpyDeviceToHost));
  if (nvy) {
    if (c->holonomic) HIPCK(c, hipMemcpy(nvy, c->lim.l_rm[1].get(), n, hipMemcpyDeviceToHost));
    else memset(nvy, 0, n);
  }
  if (nwz) HIPCK(c, hipMemcpy(nwz, c->lim.l_rm[2].get(), n, hipMemcpyDeviceToHost));
  return SMPC_OK;
}

// developer aid (SMPC_FLAG_PROFILE): GPU time of the last smpc_limit_noise launch, by HIP events
int smpc_debug_limit_ms(smpc_ctx* c, float* ms)
{
  if (!c || !ms || !c->lim.ev[0] || !c->lim.ev[1]) return SMPC_ERR_INVALID;
  HIPCK(c, hipSetDevice(c->device));
  HIPCK(c, hipEventSynchronize(c->lim.ev[1].get()));
  HIPCK(c, hipEventElapsedTime(ms, c->lim.ev[0].get(), c->lim.ev[1].get()));
  return SMPC_OK;
}

}  // extern "C"
