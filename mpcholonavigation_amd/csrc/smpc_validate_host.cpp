// smpc_validate_host.cpp — host side of the trajectory validator (include/smpc.h:
// smpc_validate_trajectory, smpc_group_validate_trajectories; the kernel: smpc_validate.hip).
//
// A call is ONE upload (every member's arguments and control sequence, back to back in one pinned
// buffer), ONE launch (a block per member) and ONE wait; the kernel writes the verdicts and the
// poses into host memory mapped into the device, so nothing is copied back.  The single call runs
// the same three steps with one member, out of buffers of the context's own; the group call out of
// buffers of the group's, on the group's stream.  Both go out on the stream the member's costmap
// uploads and ticks use: a pending costmap upload is in front of the launch.
//
// Nothing a tick depends on is read-modified here: the call prepares no tick, touches neither the
// tick block nor the predictor, the costs, the noise or the counters.  It reads the costmap's device
// copy, the footprint and the moving-obstacle table where they live.

#include "smpc_ctx.h"
#include "smpc_group.h"

namespace smpc_impl {

namespace {

// the upload: SmpcValidateArgs[count], then the members' control sequences [count][3T]
size_t u_offset(uint32_t count) {return align_up(static_cast<uint32_t>(sizeof(SmpcValidateArgs)) * count, 16);}
size_t in_bytes(uint32_t count, uint32_t T) {return u_offset(count) + static_cast<size_t>(count) * 3u * T * sizeof(float);}
size_t out_stride(uint32_t T) {return align_up(static_cast<uint32_t>(sizeof(smpc_validation)), 16) + align_up(3u * T * 4u, 16);}

int ensure_bufs(smpc_ctx* c, ValidateBufs& b, uint32_t count, uint32_t T)
{
  if (b.cap >= count) return SMPC_OK;
  // (nothing of an earlier call still runs: every call ends with a wait)
  b.cap = 0;
  HIPCK(c, b.h_in.ensure(in_bytes(count, T)));
  HIPCK(c, b.d_in.ensure(in_bytes(count, T)));
  b.h_out.reset();
  HIPCK(c, b.h_out.ensure(out_stride(T) * count, hipHostMallocMapped));
  HIPCK(c, hipHostGetDevicePointer(reinterpret_cast<void**>(&b.h_out_dev), b.h_out.get(), 0));
  b.cap = count;
  return SMPC_OK;
}

// what the call refuses of one member, before anything is written
int check_member(smpc_ctx* c, const smpc_validation_params* p, const float* u)
{
  if (!p || !u) return fail(c, SMPC_ERR_INVALID, "null argument");
  if (!std::isfinite(p->collision_lookahead_time) || !(p->collision_lookahead_time > 0.f))
    return fail(c, SMPC_ERR_INVALID, "trajectory validation: collision_lookahead_time must be > 0 and finite");
  if (c->cfg.time_steps > SMPC_VALIDATE_MAX_T) return fail(c, SMPC_ERR_UNSUPPORTED, "trajectory validation: more than 256 time steps");
  if (!c->map.set) return fail(c, SMPC_ERR_STATE, "trajectory validation: smpc_set_costmap first");
  if (p->consider_footprint && c->fp_x.empty())
    return fail(c, SMPC_ERR_STATE, "trajectory validation: consider_footprint needs smpc_set_footprint");
  return SMPC_OK;
}

// member c at position j of a launch of `count`: its arguments and control sequence into the pinned buffer
int fill_member(smpc_ctx* c, const smpc_validation_params* p, double x, double y, float yaw, const float* u,
                ValidateBufs& b, uint32_t j, uint32_t count)
{
  const uint32_t T = c->cfg.time_steps;
  SmpcValidateArgs a{};
  a.map = c->d_map.get();
  a.W = c->map.W; a.H = c->map.H;
  a.ox = c->map.ox; a.oy = c->map.oy; a.res = c->map.res;
  a.track_unknown = c->map.track_unknown ? 1u : 0u;
  a.consider_footprint = p->consider_footprint ? 1u : 0u;
  if (a.consider_footprint) {
    a.fp_n = static_cast<uint32_t>(c->fp_x.size());
    for (uint32_t i = 0; i < a.fp_n; ++i) {
      a.fp_x[i] = c->fp_x[i];
      a.fp_y[i] = c->fp_y[i];
    }
    a.fp_pic = circumscribed_cost(c->map, c->fp_circumscribed_radius, c->fp_layer_scale);
  }
  const size_t u_at = u_offset(count) + static_cast<size_t>(j) * 3u * T * sizeof(float);
  a.u = reinterpret_cast<const float*>(b.d_in.get() + u_at);
  a.x0 = x; a.y0 = y; a.yaw0 = yaw;
  a.dt = c->cfg.model_dt;
  a.T = T;
  // upstream divides in float: 2.0f / 0.05f is 40
  const float steps = floorf(p->collision_lookahead_time / c->cfg.model_dt);
  a.n_check = steps >= static_cast<float>(T) ? T : (steps > 0.f ? static_cast<uint32_t>(steps) : 0u);
  a.holonomic = c->holonomic ? 1u : 0u;
  if (p->moving_obstacles && c->mov.K > 0) {
    const int rc = wait_table_upload(c);   // (a table that went up on a stream the ctx has left since)
    if (rc != SMPC_OK) return rc;
    a.K = c->mov.K;
    a.tab_kt = c->mov.tab_kt;
    a.disc = c->mov.disc;
  }
  uint8_t* out_dev = b.h_out_dev + out_stride(T) * j;
  a.out = reinterpret_cast<smpc_validation*>(out_dev);
  a.xyyaw = reinterpret_cast<float*>(out_dev + align_up(static_cast<uint32_t>(sizeof(smpc_validation)), 16));
  memcpy(b.h_in.get() + sizeof(a) * j, &a, sizeof(a));
  memcpy(b.h_in.get() + u_at, u, 3u * T * sizeof(float));
  return SMPC_OK;
}

// one upload, one launch, one wait
int run(smpc_ctx* c0, ValidateBufs& b, uint32_t count, hipStream_t st)
{
  const uint32_t T = c0->cfg.time_steps;
  HIPCK(c0, hipMemcpyAsync(b.d_in.get(), b.h_in.get(), in_bytes(count, T), hipMemcpyHostToDevice, st));
  const hipError_t e = smpc_launch_validate(reinterpret_cast<const SmpcValidateArgs*>(b.d_in.get()), count, st);
  const hipError_t w = hipStreamSynchronize(st);   // (also behind a launch that failed: the upload reads the pinned buffer)
  HIPCK(c0, e);
  HIPCK(c0, w);
  return SMPC_OK;
}

void take_member(const ValidateBufs& b, uint32_t j, uint32_t T, smpc_validation* out, float* xyyaw)
{
  const uint8_t* h = b.h_out.get() + out_stride(T) * j;
  memcpy(out, h, sizeof(*out));
  if (xyyaw) memcpy(xyyaw, h + align_up(static_cast<uint32_t>(sizeof(smpc_validation)), 16), 3u * T * sizeof(float));
}

}  // namespace

}  // namespace smpc_impl

using namespace smpc_impl;

extern "C" {

void smpc_validation_params_default(smpc_validation_params* p)
{
  if (!p) return;
  p->collision_lookahead_time = 2.0f;
  p->consider_footprint = 0;
  p->moving_obstacles = 1;
  p->reserved = 0;
}

int smpc_validate_trajectory(smpc_ctx* c, const smpc_validation_params* p, double pose_x, double pose_y, float pose_yaw,
                             const float* u, smpc_validation* out, float* xyyaw)
{
  if (!c || !out) return fail(c, SMPC_ERR_INVALID, "null argument");
  int rc = check_member(c, p, u);
  if (rc != SMPC_OK) return rc;
  if (c->in_group || c->defer_upload)
    return fail(c, SMPC_ERR_STATE, "trajectory validation: the ctx is a member of a group (smpc_group_validate_trajectories)");
  HIPCK(c, hipSetDevice(c->device));
  rc = ensure_bufs(c, c->val, 1, c->cfg.time_steps);
  if (rc == SMPC_OK) rc = fill_member(c, p, pose_x, pose_y, pose_yaw, u, c->val, 0, 1);
  if (rc == SMPC_OK) rc = run(c, c->val, 1, c->stream);
  if (rc != SMPC_OK) return rc;
  take_member(c->val, 0, c->cfg.time_steps, out, xyyaw);
  return SMPC_OK;
}

// The members taken, each checked on its own (a refusal is that member's status and lets the others
// go on), then the three steps for those that passed, in member order.
int smpc_group_validate_trajectories(smpc_group* g, const smpc_validation_params* params, const double* poses,
                                     const float* const* u, const uint8_t* take, smpc_validation* out,
                                     float* const* xyyaw, int32_t* status)
{
  if (!g || !params || !poses || !u || !out || !status) return fail(nullptr, SMPC_ERR_INVALID, "null argument");
  smpc_ctx* c0 = nullptr;
  int rc = group_enter(g, take, &c0);
  if (rc != SMPC_OK) return rc;
  if (!c0) return fail(nullptr, SMPC_ERR_INVALID, "trajectory validation: no member of the group is taken");
  const uint32_t n = static_cast<uint32_t>(g->ctxs.size()), T = c0->cfg.time_steps;
  std::vector<uint32_t> order;
  for (uint32_t i = 0; i < n; ++i) {
    if (!group_takes(take, i)) continue;
    status[i] = check_member(g->ctxs[i], &params[i], u[i]);
    if (status[i] == SMPC_OK) order.push_back(i);
  }
  if (order.empty()) return SMPC_OK;
  rc = ensure_bufs(c0, g->val, n, T);
  for (uint32_t j = 0; rc == SMPC_OK && j < order.size(); ++j) {
    const uint32_t i = order[j];
    rc = fill_member(g->ctxs[i], &params[i], poses[3 * i], poses[3 * i + 1], static_cast<float>(poses[3 * i + 2]), u[i], g->val, j,
                     static_cast<uint32_t>(order.size()));
    if (rc != SMPC_OK) status[i] = rc;
  }
  if (rc == SMPC_OK) rc = run(c0, g->val, static_cast<uint32_t>(order.size()), g->stream);
  if (rc != SMPC_OK) return rc;
  g->count.validate_launches++;
  g->count.validate_members += order.size();
  for (uint32_t j = 0; j < order.size(); ++j) {
    const uint32_t i = order[j];
    take_member(g->val, j, T, &out[i], xyyaw ? xyyaw[i] : nullptr);
  }
  return SMPC_OK;
}

int smpc_group_validation_counts(const smpc_group* g, uint64_t* launches, uint64_t* members)
{
  if (!g) return SMPC_ERR_INVALID;
  if (launches) *launches = g->count.validate_launches;
  if (members) *members = g->count.validate_members;
  return SMPC_OK;
}

}  // extern "C"
