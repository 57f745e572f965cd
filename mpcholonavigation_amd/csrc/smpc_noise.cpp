// smpc_noise.cpp — the stored noise (smpc_ctx.h: NoiseStore): the caller's tensors (smpc_set_noise),
// the device RNG's draws (smpc_seed, smpc_redraw_noise), the background draw into the second set
// (smpc_redraw_noise_async) that the next tick absorbs, and the two layouts kept in step.

#include "smpc_ctx.h"

namespace smpc_impl {

// keep the group-major copies (smpc_dev.h: SMPC_GM_INDEX) in step with the [B,T] tensors
int update_time_major(smpc_ctx* c)
{
  if (!c->noise.use_tpr) return SMPC_OK;
  const uint32_t B = c->cfg.batch_size, T = c->cfg.time_steps;
  HIPCK(c, smpc_launch_relayout(c->noise.cur.nvx.get(), c->noise.cur.tvx.get(), B, T, true, c->stream));
  HIPCK(c, smpc_launch_relayout(c->noise.cur.nvy.get(), c->noise.cur.tvy, B, T, true, c->stream));
  HIPCK(c, smpc_launch_relayout(c->noise.cur.nwz.get(), c->noise.cur.twz, B, T, true, c->stream));
  return SMPC_OK;
}

// the [B,T] tensors (wave-per-rollout pass, smpc_get_noise) from the group-major copy, when a
// device-RNG draw filled only that one
int ensure_row_major(smpc_ctx* c)
{
  if (c->noise.rm_valid) return SMPC_OK;
  const uint32_t B = c->cfg.batch_size, T = c->cfg.time_steps;
  HIPCK(c, smpc_launch_relayout(c->noise.cur.tvx.get(), c->noise.cur.nvx.get(), B, T, false, c->stream));
  if (c->holonomic) HIPCK(c, smpc_launch_relayout(c->noise.cur.tvy, c->noise.cur.nvy.get(), B, T, false, c->stream));
  HIPCK(c, smpc_launch_relayout(c->noise.cur.twz, c->noise.cur.nwz.get(), B, T, false, c->stream));
  c->noise.rm_valid = true;
  return SMPC_OK;
}

// One epoch of the device RNG into the given set of tensors, on stream st (no wait).
// rm_valid_out: whether the [B,T] tensors of the set hold the draw (else only the group-major ones)
static int launch_draw(smpc_ctx* c, const NoiseSet& set, hipStream_t st, bool* rm_valid_out)
{
  float* const nvx = set.nvx.get();
  float* const nvy = set.nvy.get();
  float* const nwz = set.nwz.get();
  float* const tvx = set.tvx.get();
  float* const tvy = set.tvy;
  float* const twz = set.twz;
  const uint64_t n = static_cast<uint64_t>(c->cfg.batch_size) * c->cfg.time_steps;
  const uint64_t base = c->cfg.shard_offset * c->cfg.time_steps;
  const uint32_t B = c->cfg.batch_size, T = c->cfg.time_steps;
  if (c->noise.use_tpr && (T & 3u) == 0 && !getenv("SMPC_NO_FUSED_FILL")) {
    // lane-per-rollout contexts: draw straight into the group-major layout that pass reads —
    // one write of the noise instead of a write, a read and a second write (fill + transpose);
    // the [B,T] copy is made only if something asks for it (ensure_row_major)
    HIPCK(c, smpc_launch_fill_noise_tm(tvx, B, T, base, c->noise.seed, 0, c->noise.epoch, c->cfg.vx_std, st));
    HIPCK(c, smpc_launch_fill_noise_tm(twz, B, T, base, c->noise.seed, 1, c->noise.epoch, c->cfg.wz_std, st));
    if (c->holonomic)
      HIPCK(c, smpc_launch_fill_noise_tm(tvy, B, T, base, c->noise.seed, 2, c->noise.epoch, c->cfg.vy_std, st));
    else
      HIPCK(c, hipMemsetAsync(tvy, 0, SMPC_GM_ELEMS(B, T) * sizeof(float), st));
    *rm_valid_out = false;
    return SMPC_OK;
  }
  // draw order vx, wz, vy (noise_generator.cpp:107-122)
  HIPCK(c, smpc_launch_fill_noise(nvx, n, base, c->noise.seed, 0, c->noise.epoch, c->cfg.vx_std, st));
  HIPCK(c, smpc_launch_fill_noise(nwz, n, base, c->noise.seed, 1, c->noise.epoch, c->cfg.wz_std, st));
  // noises_vy_ keeps its zeros for a non-holonomic model (noise_generator.cpp:117-121)
  if (c->holonomic) HIPCK(c, smpc_launch_fill_noise(nvy, n, base, c->noise.seed, 2, c->noise.epoch, c->cfg.vy_std, st));
  if (c->noise.use_tpr) {
    HIPCK(c, smpc_launch_relayout(nvx, tvx, B, T, true, st));
    HIPCK(c, smpc_launch_relayout(nvy, tvy, B, T, true, st));
    HIPCK(c, smpc_launch_relayout(nwz, twz, B, T, true, st));
  }
  *rm_valid_out = true;
  return SMPC_OK;
}

// a draw requested with smpc_redraw_noise_async that no tick has taken yet is dropped (whoever
// calls this is about to overwrite the noise anyway)
int cancel_redraw(smpc_ctx* c)
{
  if (!c->noise.redraw_pending) return SMPC_OK;
  HIPCK(c, hipEventSynchronize(c->noise.ev_fill.get()));
  c->noise.redraw_pending = false;
  return SMPC_OK;
}

// The tick about to be prepared takes the noise drawn in the background, if there is any: its
// stream waits for the draw ON THE DEVICE and the two sets of tensors change places.
int absorb_redraw(smpc_ctx* c)
{
  if (!c->noise.redraw_pending) return SMPC_OK;
  HIPCK(c, hipStreamWaitEvent(c->stream, c->noise.ev_fill.get(), 0));
  std::swap(c->noise.cur, c->noise.next);
  c->noise.rm_valid = c->noise.redraw_rm_valid;
  c->noise.redraw_pending = false;
  c->noise.noise_gen++;
  return SMPC_OK;
}

int draw_noise(smpc_ctx* c)
{
  int rc = cancel_redraw(c);
  if (rc != SMPC_OK) return rc;
  bool rm = true;
  rc = launch_draw(c, c->noise.cur, c->stream, &rm);
  if (rc != SMPC_OK) return rc;
  HIPCK(c, hipStreamSynchronize(c->stream));
  c->noise.have_noise = true;
  c->noise.rm_valid = rm;
  c->noise.noise_gen++;
  return SMPC_OK;
}

// NoiseGenerator::generateNextNoises as the reference runs it (noise_generator.cpp:54-63,97-105:
// a thread draws the next tensors while the optimizer goes on): the next epoch goes into the
// OTHER set of tensors on a stream of its own, and the call returns at once.
int redraw_async(smpc_ctx* c)
{
  if (c->noise.redraw_pending) return SMPC_OK;   // (the reference's signal is not counted either)
  const size_t n = static_cast<size_t>(c->cfg.batch_size) * c->cfg.time_steps;
  HIPCK(c, c->noise.fill_stream.ensure(hipStreamNonBlocking));
  HIPCK(c, c->noise.ev_fill.ensure(hipEventDisableTiming));
  NoiseSet& next = c->noise.next;
  if (c->noise.use_tpr && !next.tvx) {
    const size_t ngm = SMPC_GM_ELEMS(c->cfg.batch_size, c->cfg.time_steps);
    HIPCK(c, next.tvx.ensure(3 * ngm));
    HIPCK(c, hipMemset(next.tvx.get(), 0, 3 * ngm * sizeof(float)));   // (the padding steps of a ragged horizon: zeros)
    next.tvy = next.tvx.get() + ngm;
    next.twz = next.tvy + ngm;
  }
  HIPCK(c, next.nvx.ensure(n));
  HIPCK(c, next.nwz.ensure(n));
  if (!next.nvy) {
    HIPCK(c, next.nvy.ensure(n));
    if (!c->holonomic) HIPCK(c, hipMemset(next.nvy.get(), 0, n * sizeof(float)));
  }
  c->noise.epoch++;
  bool rm = true;
  const int rc = launch_draw(c, next, c->noise.fill_stream.get(), &rm);
  if (rc != SMPC_OK) return rc;
  HIPCK(c, hipEventRecord(c->noise.ev_fill.get(), c->noise.fill_stream.get()));
  c->noise.redraw_rm_valid = rm;
  c->noise.redraw_pending = true;
  return SMPC_OK;
}

}  // namespace smpc_impl

using namespace smpc_impl;

extern "C" {

int smpc_set_noise(smpc_ctx* c, const float* nvx, const float* nvy, const float* nwz)
{
  if (!c || !nvx || !nvy || !nwz) return SMPC_ERR_INVALID;
  HIPCK(c, hipSetDevice(c->device));
  const size_t n = static_cast<size_t>(c->cfg.batch_size) * c->cfg.time_steps * sizeof(float);
  {
    const int rc = cancel_redraw(c);
    if (rc != SMPC_OK) return rc;
  }
  HIPCK(c, hipMemcpyAsync(c->noise.cur.nvx.get(), nvx, n, hipMemcpyHostToDevice, c->stream));
  if (c->holonomic) HIPCK(c, hipMemcpyAsync(c->noise.cur.nvy.get(), nvy, n, hipMemcpyHostToDevice, c->stream));
  HIPCK(c, hipMemcpyAsync(c->noise.cur.nwz.get(), nwz, n, hipMemcpyHostToDevice, c->stream));
  {
    int rc = update_time_major(c);
    if (rc != SMPC_OK) return rc;
  }
  HIPCK(c, hipStreamSynchronize(c->stream));
  c->noise.have_noise = true;
  c->noise.rm_valid = true;
  c->noise.rng_mode = false;
  c->noise.noise_gen++;
  return SMPC_OK;
}

int smpc_seed(smpc_ctx* c, uint64_t seed)
{
  if (!c) return SMPC_ERR_INVALID;
  HIPCK(c, hipSetDevice(c->device));
  c->noise.seed = seed;
  c->noise.epoch = 0;
  c->noise.rng_mode = true;
  return draw_noise(c);
}

int smpc_redraw_noise(smpc_ctx* c)
{
  if (!c) return SMPC_ERR_INVALID;
  if (!c->noise.rng_mode) return fail(c, SMPC_ERR_STATE, "smpc_redraw_noise needs device-RNG mode (smpc_seed)");
  HIPCK(c, hipSetDevice(c->device));
  c->noise.epoch++;
  return draw_noise(c);
}

int smpc_redraw_noise_async(smpc_ctx* c)
{
  if (!c) return SMPC_ERR_INVALID;
  if (!c->noise.rng_mode) return fail(c, SMPC_ERR_STATE, "smpc_redraw_noise_async needs device-RNG mode (smpc_seed)");
  HIPCK(c, hipSetDevice(c->device));
  return redraw_async(c);
}

int smpc_get_noise(smpc_ctx* c, float* nvx, float* nvy, float* nwz)
{
  if (!c) return SMPC_ERR_INVALID;
  if (!c->noise.have_noise) return fail(c, SMPC_ERR_STATE, "no noise yet");
  HIPCK(c, hipSetDevice(c->device));
  const size_t n = static_cast<size_t>(c->cfg.batch_size) * c->cfg.time_steps * sizeof(float);
  {
    const int rc = ensure_row_major(c);
    if (rc != SMPC_OK) return rc;
  }
  HIPCK(c, hipStreamSynchronize(c->stream));
  if (nvx) HIPCK(c, hipMemcpy(nvx, c->noise.cur.nvx.get(), n, hipMemcpyDeviceToHost));
  if (nvy) HIPCK(c, hipMemcpy(nvy, c->noise.cur.nvy.get(), n, hipMemcpyDeviceToHost));
  if (nwz) HIPCK(c, hipMemcpy(nwz, c->noise.cur.nwz.get(), n, hipMemcpyDeviceToHost));
  return SMPC_OK;
}

}  // extern "C"
