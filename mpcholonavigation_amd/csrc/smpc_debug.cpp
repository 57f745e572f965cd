// smpc_debug.cpp — the developer entry points of include/smpc_debug.h that are not part of a
// feature's own file: the device selftests (one kernel each, on buffers of their own) and the
// views into a context's state that tests and tools read.

#include "smpc_ctx.h"
#include "../../include/smpc_debug.h"

using namespace smpc_impl;

extern "C" {

int smpc_selftest_sincos(smpc_ctx* c, const float* x, uint32_t n, float* sin_out, float* cos_out)
{
  if (!c || !x || !sin_out || !cos_out || n == 0) return fail(c, SMPC_ERR_INVALID, "null argument");
  HIPCK(c, hipSetDevice(c->device));
  DevBuf<float> dx, ds, dc;
  HIPCK(c, dx.ensure(n));
  HIPCK(c, ds.ensure(n));
  HIPCK(c, dc.ensure(n));
  HIPCK(c, hipMemcpyAsync(dx.get(), x, n * sizeof(float), hipMemcpyHostToDevice, c->stream));
  HIPCK(c, smpc_launch_sincos(dx.get(), n, ds.get(), dc.get(), c->stream));
  HIPCK(c, hipMemcpyAsync(sin_out, ds.get(), n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  HIPCK(c, hipMemcpyAsync(cos_out, dc.get(), n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  HIPCK(c, hipStreamSynchronize(c->stream));
  return SMPC_OK;
}

int smpc_selftest_philox(smpc_ctx* c, const uint32_t* ctr, const uint32_t* key, uint32_t n, uint32_t* out)
{
  if (!c || !ctr || !key || !out || n == 0 || n > (1u << 26)) return fail(c, SMPC_ERR_INVALID, "bad argument");
  HIPCK(c, hipSetDevice(c->device));
  const size_t words = static_cast<size_t>(n) * 4, bytes = words * sizeof(uint32_t);
  DevBuf<uint32_t> dc, dout;
  HIPCK(c, dc.ensure(words));
  HIPCK(c, dout.ensure(words));
  HIPCK(c, hipMemcpyAsync(dc.get(), ctr, bytes, hipMemcpyHostToDevice, c->stream));
  HIPCK(c, smpc_launch_philox(dc.get(), key[0], key[1], n, dout.get(), c->stream));
  HIPCK(c, hipMemcpyAsync(out, dout.get(), bytes, hipMemcpyDeviceToHost, c->stream));
  HIPCK(c, hipStreamSynchronize(c->stream));
  return SMPC_OK;
}

int smpc_selftest_box_muller(smpc_ctx* c, const uint32_t* r0, const uint32_t* r1, uint32_t n, float* z0, float* z1)
{
  if (!c || !r0 || !r1 || !z0 || !z1 || n == 0 || n > (1u << 26)) return fail(c, SMPC_ERR_INVALID, "bad argument");
  HIPCK(c, hipSetDevice(c->device));
  const size_t bytes = static_cast<size_t>(n) * sizeof(uint32_t);
  DevBuf<uint32_t> d0, d1;
  DevBuf<float> dz0, dz1;
  HIPCK(c, d0.ensure(n));
  HIPCK(c, d1.ensure(n));
  HIPCK(c, dz0.ensure(n));
  HIPCK(c, dz1.ensure(n));
  HIPCK(c, hipMemcpyAsync(d0.get(), r0, bytes, hipMemcpyHostToDevice, c->stream));
  HIPCK(c, hipMemcpyAsync(d1.get(), r1, bytes, hipMemcpyHostToDevice, c->stream));
  HIPCK(c, smpc_launch_box_muller(d0.get(), d1.get(), n, dz0.get(), dz1.get(), c->stream));
  HIPCK(c, hipMemcpyAsync(z0, dz0.get(), bytes, hipMemcpyDeviceToHost, c->stream));
  HIPCK(c, hipMemcpyAsync(z1, dz1.get(), bytes, hipMemcpyDeviceToHost, c->stream));
  HIPCK(c, hipStreamSynchronize(c->stream));
  return SMPC_OK;
}

int smpc_selftest_lane_reduce(smpc_ctx* c, const float* v, const float* w, float* out)
{
  if (!c || !v || !w || !out) return fail(c, SMPC_ERR_INVALID, "null argument");
  HIPCK(c, hipSetDevice(c->device));
  DevBuf<float> dv, dw, dout;
  HIPCK(c, dv.ensure(64 * 64));
  HIPCK(c, dw.ensure(64));
  HIPCK(c, dout.ensure(64));
  HIPCK(c, hipMemcpyAsync(dv.get(), v, 64 * 64 * sizeof(float), hipMemcpyHostToDevice, c->stream));
  HIPCK(c, hipMemcpyAsync(dw.get(), w, 64 * sizeof(float), hipMemcpyHostToDevice, c->stream));
  HIPCK(c, smpc_launch_lane_reduce(dv.get(), dw.get(), dout.get(), c->stream));
  HIPCK(c, hipMemcpyAsync(out, dout.get(), 64 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  HIPCK(c, hipStreamSynchronize(c->stream));
  return SMPC_OK;
}

int smpc_selftest_row_reduce(smpc_ctx* c, const float* v, uint32_t n, float* out)
{
  if (!c || !v || !out || (n != 16 && n != 32)) return fail(c, SMPC_ERR_INVALID, "bad argument");
  HIPCK(c, hipSetDevice(c->device));
  DevBuf<float> dv, dout;
  HIPCK(c, dv.ensure(64 * n));
  HIPCK(c, dout.ensure(64));
  HIPCK(c, hipMemcpyAsync(dv.get(), v, 64 * n * sizeof(float), hipMemcpyHostToDevice, c->stream));
  HIPCK(c, smpc_launch_row_reduce(dv.get(), dout.get(), n, c->stream));
  HIPCK(c, hipMemcpyAsync(out, dout.get(), 64 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  HIPCK(c, hipStreamSynchronize(c->stream));
  return SMPC_OK;
}

// developer aid: smpc_grid_tail's stamps of the last launch, [8 reducers][16] in s_memrealtime ticks (10 ns)
int smpc_debug_tail_timeline(smpc_ctx* c, unsigned long long* out)
{
  if (!c || !out || !c->d_timeline) return SMPC_ERR_INVALID;
  HIPCK(c, hipSetDevice(c->device));
  HIPCK(c, hipStreamSynchronize(c->stream));
  HIPCK(c, hipMemcpy(out, c->d_timeline.get() + SMPC_TAIL_STAMPS_AT, 8 * 16 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  return SMPC_OK;
}

// developer aid: stage durations of the last lane-pass launch, from the stamps of wave 0 of
// every block (shader clocks; stages: entry -> LDS staged -> constants -> group 1 -> group 2
// -> all waves at the final barrier -> partial written); out[7][3] = min, median, max
int smpc_debug_lane_timeline(smpc_ctx* c, double* out, uint32_t* n_blocks)
{
  if (!c || !out || !c->d_timeline) return SMPC_ERR_INVALID;
  HIPCK(c, hipSetDevice(c->device));
  HIPCK(c, hipStreamSynchronize(c->stream));
  const uint32_t nb = c->plan.lane.grid;
  std::vector<unsigned long long> h(static_cast<size_t>(nb) * 8);
  HIPCK(c, hipMemcpy(h.data(), c->d_timeline.get(), h.size() * sizeof(h[0]), hipMemcpyDeviceToHost));
  unsigned long long t0 = ~0ull;
  for (uint32_t b = 0; b < nb; ++b) t0 = std::min(t0, h[b * 8]);
  for (int k = 0; k < 7; ++k) {
    std::vector<double> v;
    for (uint32_t b = 0; b < nb; ++b)
      if (h[b * 8 + k]) v.push_back(static_cast<double>(h[b * 8 + k] - (k ? h[b * 8 + k - 1] : t0)));
    std::sort(v.begin(), v.end());
    out[3 * k] = v.empty() ? 0 : v.front();
    out[3 * k + 1] = v.empty() ? 0 : v[v.size() / 2];
    out[3 * k + 2] = v.empty() ? 0 : v.back();
  }
  // out[21..28]: per wave of the block, median of (end of its groups - stamp 2 of wave 0)
  std::vector<unsigned long long> hw(static_cast<size_t>(nb) * 8);
  HIPCK(c, hipMemcpy(hw.data(), c->d_timeline.get() + 8192, hw.size() * sizeof(hw[0]), hipMemcpyDeviceToHost));
  for (int w = 0; w < 8; ++w) {
    std::vector<double> v;
    for (uint32_t b = 0; b < nb; ++b)
      if (hw[b * 8 + w] && h[b * 8 + 2]) v.push_back(static_cast<double>(hw[b * 8 + w] - h[b * 8 + 2]));
    std::sort(v.begin(), v.end());
    out[21 + w] = v.empty() ? 0 : v[v.size() / 2];
  }
  if (n_blocks) *n_blocks = nb;
  return SMPC_OK;
}

// developer aid (SMPC_LANE_TIMELINE=1): how many groups of the lane pass took the furthest-point scan
// since the last call (the instances with the prune test count; smpc_lane_furthest.inc), and how
// many groups a launch of the current plan has; the counts are cleared
int smpc_debug_lane_scan_count(smpc_ctx* c, unsigned long long* scanned, uint32_t* groups_per_launch)
{
  if (!c || !scanned || !c->d_timeline) return SMPC_ERR_INVALID;
  HIPCK(c, hipSetDevice(c->device));
  HIPCK(c, hipStreamSynchronize(c->stream));
  std::vector<unsigned long long> h(static_cast<size_t>(kMaxGrid) * 8);
  HIPCK(c, hipMemcpy(h.data(), c->d_timeline.get() + SMPC_SCAN_COUNT_AT, h.size() * sizeof(h[0]), hipMemcpyDeviceToHost));
  HIPCK(c, hipMemset(c->d_timeline.get() + SMPC_SCAN_COUNT_AT, 0, h.size() * sizeof(h[0])));
  unsigned long long sum = 0;
  for (unsigned long long v : h) sum += v;
  *scanned = sum;
  if (groups_per_launch) *groups_per_launch = (c->cfg.batch_size + 63u) / 64u;
  return SMPC_OK;
}

// developer aid (tests): the float F = index + fraction the last tick's scoring pass reported (the
// tuple's slot 2, smpc_dev.h), as remember_furthest kept it for the next prediction — the value
// itself while the stored noise stays the same from tick to tick
int smpc_debug_furthest_f(const smpc_ctx* c, float* F)
{
  if (!c || !F || !c->pred.hint_valid) return SMPC_ERR_INVALID;
  *F = c->pred.hint_F;
  return SMPC_OK;
}

// developer aid, host only (tests/test_furthest_prune_cpu.py): the prune table prepare_tick would
// write for this plan and first index; out: SMPC_PRUNE_FLOATS floats
int smpc_debug_prune_table(const float* px, const float* py, uint32_t P, uint32_t k0, int on, float* out)
{
  if (!px || !py || !out) return SMPC_ERR_INVALID;
  build_prune_table(px, py, P, k0, on != 0, out);
  return SMPC_OK;
}

// developer aid, host only (tests/test_lds_layout_cpu.py): the LDS carve-up a scoring pass is
// launched with — kind 0: the wave pass (make_lds; arg = PathAlign samples per rollout), 1: the lane
// pass (lane_lds; arg != 0: the re-read form), 2: the split pass (split_lds; arg = segments, 2 or
// 4) — for a costmap window of window_bytes cells (0: no costmap lookup), P path points and T
// steps, with the block sizes plan_launch uses.  out: the 16 words of SmpcLds in declaration order.
int smpc_debug_lds_layout(int kind, uint32_t window_bytes, uint32_t P, uint32_t T, uint32_t arg, uint32_t* out)
{
  if (!out || T == 0) return SMPC_ERR_INVALID;
  SmpcLds L{};
  if (kind == 0) {
    const int R = T <= 64 ? 1 : (T <= 128 ? 2 : 4);   // (smpc_create)
    L = make_lds(window_bytes, P, T, pass_block(R) / 64, window_bytes != 0, arg);
  } else if (kind == 1) {
    L = lane_lds(window_bytes, P, T, arg != 0);
  } else if (kind == 2 && (arg == 2 || arg == 4)) {
    L = split_lds(window_bytes, P, T, arg);
  } else {
    return SMPC_ERR_INVALID;
  }
  static_assert(sizeof(SmpcLds) == 16 * sizeof(uint32_t), "SmpcLds: 16 words");
  memcpy(out, &L, sizeof(L));
  return SMPC_OK;
}

// developer aid (bench.py labels its roofline with it): the scoring-pass instance the calling
// thread launched last, spelled as rocprofv3's kernel trace spells it
const char* smpc_debug_last_pass_kernel(void) {return smpc_last_pass_kernel;}

// developer aid: how this ctx hands its per-tick inputs to the device — 1: CPU stores through the
// PCIe BAR, 0: a copy on the stream (or, for wave-pass contexts, inside the kernel arguments)
int smpc_debug_bar_tick(const smpc_ctx* c) {return c && c->tick.bar_tick ? 1 : 0;}

}  // extern "C"
