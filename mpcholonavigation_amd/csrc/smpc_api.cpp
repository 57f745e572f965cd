// smpc_api.cpp — host side of the C-ABI declared in include/smpc.h: the context's lifecycle
// (smpc_create, free_ctx), the setters, the costmap, the launch helpers the tick drivers share,
// fetch_out and the single-GPU tick (smpc_optimize).  The rest of the host side by topic: smpc_ctx.h
// lists the files.  All [B,T] work is in the .hip files.  There is no CPU fallback: without a HIP
// device smpc_create() fails.

#include "smpc_ctx.h"

#include <emmintrin.h>

namespace smpc_impl {

thread_local std::string g_create_error;

int fail(smpc_ctx* c, int code, const std::string& msg)
{
  if (c) c->err = msg; else g_create_error = msg;
  return code;
}

// A costmap upload is asynchronous (pinned mirror -> device on the ctx's stream).  Kernels of
// the same stream are ordered behind it; this host-side wait covers the rest: a tick
// launched on another stream (grouped ticks, smpc_set_stream) and the next overwrite of
// the mirror.
int wait_map_upload(smpc_ctx* c)
{
  if (!c->map_pending) return SMPC_OK;
  HIPCK(c, hipEventSynchronize(c->ev_map.get()));
  c->map_pending = false;
  return SMPC_OK;
}

void bar_copy(void* dev_dst, const void* host_src, size_t n)
{
  // The BAR mapping is write-combining: 16-byte streaming stores fill whole 64-byte buffers,
  // and the fence drains them before any later store of this thread — the runtime's doorbell
  // write for the launch that reads the block included (PCIe keeps posted writes to one device
  // in order).  The kernel boundary in front of that launch invalidates the GPU's caches.
  const __m128i* src = static_cast<const __m128i*>(host_src);
  __m128i* dst = static_cast<__m128i*>(dev_dst);
  for (size_t i = 0; i < n / 16; ++i) _mm_stream_si128(dst + i, _mm_load_si128(src + i));
  _mm_sfence();
}

void bar_flush(const smpc_ctx* c)
{
  // one posted MMIO write, ordered behind the drained stores and in front of the doorbell
  if (c->tick.hdp_flush) *c->tick.hdp_flush = 1u;
}

// HDP_MEM_FLUSH_CNTL of HIP device `dev` (matched by PCI location), through the HSA runtime the
// HIP runtime already holds; null when it cannot be found
static volatile uint32_t* find_hdp_flush(int dev)
{
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, dev) != hipSuccess) return nullptr;
  void* h = dlopen("libhsa-runtime64.so.1", RTLD_NOW | RTLD_NOLOAD);
  if (!h) h = dlopen("libhsa-runtime64.so.1", RTLD_NOW | RTLD_LOCAL);
  if (!h) return nullptr;
  using agent_t = struct {uint64_t handle;};
  using iterate_fn = int (*)(int (*)(agent_t, void*), void*);
  using info_fn = int (*)(agent_t, int, void*);
  using init_fn = int (*)();
  static init_fn p_init = reinterpret_cast<init_fn>(dlsym(h, "hsa_init"));
  static iterate_fn p_iter = reinterpret_cast<iterate_fn>(dlsym(h, "hsa_iterate_agents"));
  static info_fn p_info = reinterpret_cast<info_fn>(dlsym(h, "hsa_agent_get_info"));
  if (!p_init || !p_iter || !p_info || p_init() != 0) return nullptr;   // (reference-counted; HIP holds it already)
  struct Want {
    uint32_t domain, bdf;
    volatile uint32_t* reg;
  } want{static_cast<uint32_t>(prop.pciDomainID),
         (static_cast<uint32_t>(prop.pciBusID) << 8) | (static_cast<uint32_t>(prop.pciDeviceID) << 3), nullptr};
  auto cb = [](agent_t a, void* data) -> int {
    Want* w = static_cast<Want*>(data);
    int type = 0;   // HSA_AGENT_INFO_DEVICE = 17, HSA_DEVICE_TYPE_GPU = 1
    if (p_info(a, 17, &type) != 0 || type != 1) return 0;
    uint32_t bdf = 0, domain = 0;
    if (p_info(a, 0xA006, &bdf) != 0) return 0;              // HSA_AMD_AGENT_INFO_BDFID
    if (p_info(a, 0xA00F, &domain) != 0) domain = w->domain;   // HSA_AMD_AGENT_INFO_DOMAIN
    if ((bdf & ~7u) != w->bdf || domain != w->domain) return 0;
    struct {uint32_t* mem; uint32_t* reg;} f{nullptr, nullptr};
    if (p_info(a, 0xA00E, &f) == 0) w->reg = f.mem;          // HSA_AMD_AGENT_INFO_HDP_FLUSH
    return 1;   // (HSA_STATUS_INFO_BREAK: stop iterating)
  };
  (void)p_iter(cb, &want);
  return want.reg;
}

void free_ctx(smpc_ctx* c)
{
  if (!c) return;
  (void)hipSetDevice(c->device);
  // what may still be reading or writing the buffers: the ticks' stream (a breakdown or a tick
  // abandoned on an error), the background draw, and the last moving-obstacle upload
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  if (c->noise.fill_stream) (void)hipStreamSynchronize(c->noise.fill_stream.get());
  if (c->mov.up_recorded) (void)hipEventSynchronize(c->mov.ev_up.get());
  // the two links to other processes, which are not plain frees
  for (uint32_t r = 0; r < c->shard.p2p.world; ++r)
    if (r != c->shard.p2p.rank && c->shard.p2p.peer[r]) (void)hipIpcCloseMemHandle(c->shard.p2p.peer[r]);
  if (c->shard.comm && rccl()) (void)rccl()->CommDestroy(c->shard.comm);
  delete c;   // every buffer, event and stream: its holder's destructor (smpc_own.h)
}

int launch_furthest(smpc_ctx* c, float* d_furthest)
{
  {
    const int rc = ensure_row_major(c);   // the wave-per-rollout pass reads the [B,T] tensors
    if (rc != SMPC_OK) return rc;
  }
  HIPCK(c, hipMemsetAsync(d_furthest, 0, sizeof(float), c->stream));
  SmpcDev d = c->dev;
  {
    const int rc = use_limited_noise(c, d, false);
    if (rc != SMPC_OK) return rc;
  }
  d.flags = c->gate_flags & SD_NEED_FURTHEST;
  d.furthest_out = reinterpret_cast<uint32_t*>(d_furthest);
  SmpcLds L = make_lds(0, c->P, d.T, (pass_block(c->R) / 64), false);
  c->launched = true;
  HIPCK(c, wave_launch(wave_select(c->R, 1, d.T), d, L, c->plan.wave.grid, c->plan.wave.block, c->stream));
  return SMPC_OK;
}

int begin_tick(smpc_ctx* c, const smpc_tick_in* in, const float* u_in)
{
  const int rc = prepare_tick(c, in, u_in);   // (touches none of the three; the predictor it advances is c->pred)
  if (rc != SMPC_OK) return rc;
  c->passes = 0;
  c->evp_used = 0;
  c->costs_cur = 0;
  return SMPC_OK;
}

int refuse_sharded(smpc_ctx* c)
{
  if (c->two_coll_fp)
    return fail(c, SMPC_ERR_UNSUPPORTED,
                "sharded tick: consider_footprint=true with both ObstaclesCritic and CostCritic in the list");
  if (c->cfg.iteration_count != 1)   // (one exchange = one iteration; never silently fewer than asked for)
    return fail(c, SMPC_ERR_UNSUPPORTED, "sharded tick: iteration_count must be 1");
  return SMPC_OK;
}

uint32_t next_seq(smpc_ctx* c)
{
  if (++c->seq == 0) ++c->seq;
  c->poll_seq = c->seq;
  return c->seq;
}

// parameter blocks of one scoring pass + reduction of ctx c (no launch)
// finish_furthest: when `finish`, the reduction also produces the new control sequence
// (single-GPU tick) and reports *finish_furthest (or the pass's own value) as the furthest
// point the critics used
void fill_score_args(smpc_ctx* c, uint32_t flags, const float* u_dev, const float* d_furthest,
                     uint32_t furthest_hint, bool finish, const float* finish_furthest, SmpcDev& d,
                     SmpcFinal& fin)
{
  d = c->dev;
  d.flags = flags;
  if (u_dev) {        // a later iteration: the control sequence the previous one left on the device
    d.u = u_dev;
    d.u_inline = 0;
  }
  d.d_furthest = d_furthest;
  d.furthest_hint = furthest_hint;
  d.costs = c->d_costs[c->costs_cur].get();
  d.costs_prev = c->d_costs[c->costs_cur ^ 1].get();
  fin = SmpcFinal{};
  fin.enabled = finish ? 1 : 0;
  fin.vx_max = c->c_vx_max; fin.vx_min = c->c_vx_min; fin.vy_max = c->c_vy; fin.wz_max = c->c_wz;
  fin.u_dev = c->d_out.get(); fin.u_host = c->h_out_dev; fin.furthest_used = finish_furthest;
  if (finish && c->knobs.poll) {
    fin.done_counter = scratch_word(c, SMPC_SCRATCH_REDUCE_COUNTER);
    fin.seq = next_seq(c);
  }
  if (finish && c->acker_r >= 0.f) {   // the Ackermann launch behind the reduction publishes
    c->acker_seq = fin.seq;
    fin.done_counter = nullptr;
    fin.seq = 0;
  }
}

// The pass that scores `flags` this tick: what plan_launch chose, or — for a pass whose flags were
// stripped after the launch was planned: fail_flag_in (the retry after fallback(), which scores
// nothing: critic_manager.cpp:70-73) or the later iterations of an all-collide tick — the next
// family down that has an instance for them.  The split form scores the plain five with
// ObstaclesCritic on: its stripped tick takes the lane pass.  The re-read form has instances with
// ObstaclesCritic scored only, and no lane instance writes trajectories: such a pass takes the
// wave-per-rollout pass (its geometry is planned for every tick).  A parking-form tick without an
// instance is an error, as it always was.  A tick that scores with cost powers (pl.pow) picks among
// the rows of smpc_pass_lane_pow, which include the two without a costmap lookup for its stripped passes.
// A non-holonomic tick on the rows of smpc_pass_lane_nh (pl.nh) runs them for every pass whose flags
// have one — a speculation miss, a later iteration, the all-collide re-score — and the plain row of
// the flags where they have none (no ObstaclesCritic left: the Omni-form row reads the zero vy stream).
struct PassChoice {
  PassPlan::Kind kind;
  const void* inst;        // WaveInst, LaneInst or SplitInst by kind; null: no instance
  const PassGeom* geom;
};
static PassChoice pass_for(const smpc_ctx* c, uint32_t flags)
{
  const PassPlan& pl = c->plan;
  const uint32_t T = c->dev.T;
  if (pl.kind == PassPlan::kSplit)
    if (const SplitInst* k = split_select(flags, T, c->dev.step, pl.split_nseg)) return {PassPlan::kSplit, k, &pl.split};
  if (pl.kind != PassPlan::kWave) {
    const LaneInst* k = lane_select(flags, T, pl.rr, false, c->acker_r, pl.pow, pl.nh);
    if (k || !(pl.rr || (flags & SD_STORE_TRAJ))) return {PassPlan::kLane, k, &pl.lane};
  }
  return {PassPlan::kWave, wave_select(c->R, c->score_mode, T), &pl.wave};
}

// one scoring pass + block reduction -> tuple
int launch_score(smpc_ctx* c, uint32_t flags, const float* u_dev, const float* d_furthest,
                 uint32_t furthest_hint, float* d_tuple, bool finish, const float* finish_furthest)
{
  SmpcDev d;
  SmpcFinal fin;
  fill_score_args(c, flags, u_dev, d_furthest, furthest_hint, finish, finish_furthest, d, fin);
  const PassChoice pass = pass_for(c, flags);
  {
    // acceleration limits: the iteration's limited noise in the layout this pass reads (made here if
    // this is the first pass of the iteration to read it), in front of the pass's profile events
    int rc = use_limited_noise(c, d, pass.kind != PassPlan::kWave);
    if (rc != SMPC_OK) return rc;
    // moving obstacles: the iteration's seed (scored here if this is its first pass), read from that noise
    rc = use_moving_seed(c, d, pass.kind != PassPlan::kWave);
    if (rc != SMPC_OK) return rc;
  }
  const bool prof = (c->cfg.flags & SMPC_FLAG_PROFILE) && c->evp_used + 2 <= 8;
  if (prof) HIPCK(c, hipEventRecord(c->evp[c->evp_used].get(), c->stream));
  const uint32_t nblk = pass.geom->grid;
  // The block that finishes last reduces the partials inside the scoring launch (smpc_tail.h);
  // larger grids, and launches whose LDS was not sized for it, take the separate reduction.
  // (The lane pass: full-size blocks only.)
  const bool tail = pass.kind != PassPlan::kSplit && c->knobs.fused_reduce && nblk <= SMPC_TAIL_MAX_GRID &&
    (pass.kind != PassPlan::kLane || pass.geom->block == smpc_lane_block()) && pass.geom->lds.total >= smpc_tail_lds_bytes(d.T);
  // completion words: one per block of smpc_reduce_partials, or per reducing block of the tail
  const bool polled = fin.enabled && fin.done_counter;
  c->poll_words = !polled ? 0u : tail ? smpc_tail_reduce_blocks(d.T, nblk) : smpc_reduce_blocks(d.T);
  static_assert(smpc_reduce_blocks(64u * SMPC_MAX_R) <= kPollWords, "one completion word per reducing block");
  if (tail) {
    // the tail's "gave up waiting" mark of an earlier tick must not fail this one (no launch of
    // this ctx is in flight here: every tick ends with fetch_out); the mailbox exchange's mark
    // in the same word is sticky by design and stays
    float& mark = c->h_out.get()[SMPC_RESULT_AT(d.T) + SMPC_R_MARK];
    if (mark == SMPC_MARK_TAIL_LATE) mark = SMPC_MARK_NONE;
    d.tail = 1;
    d.tail_counter = scratch_word(c, SMPC_SCRATCH_TAIL_COUNTER);
    d.tuple = d_tuple;
    d.fin = fin;
  }
  c->launched = true;
  c->last_pass_kind = pass.kind;
  if (pass.kind == PassPlan::kSplit) {
    HIPCK(c, split_launch(static_cast<const SplitInst*>(pass.inst), d, pass.geom->lds, nblk, c->stream));
  } else if (pass.kind == PassPlan::kLane) {
    HIPCK(c, lane_launch(static_cast<const LaneInst*>(pass.inst), d, nullptr, 1, pass.geom->lds, nblk, pass.geom->block, c->stream));
  } else {
    const int rc_rm = ensure_row_major(c);   // the wave-per-rollout pass reads the [B,T] tensors
    if (rc_rm != SMPC_OK) return rc_rm;
    HIPCK(c, wave_launch(static_cast<const WaveInst*>(pass.inst), d, pass.geom->lds, nblk, pass.geom->block, c->stream));
  }
  if (prof) {
    HIPCK(c, hipEventRecord(c->evp[c->evp_used + 1].get(), c->stream));
    c->evp_used += 2;
  }
  if (!tail) HIPCK(c, smpc_launch_reduce(c->d_partials.get(), nblk, d.T, d.neg_inv_temp, d_tuple, fin, c->stream));
  if (finish && c->acker_r >= 0.f)
    HIPCK(c, smpc_launch_ackermann(c->d_out.get(), c->h_out_dev, d.T, c->acker_r, c->acker_seq, c->stream));
  c->passes++;
  return SMPC_OK;
}

int launch_combine(smpc_ctx* c, const float* d_tuples, uint32_t n, const float* d_furthest_used)
{
  const uint32_t T = c->cfg.time_steps;
  uint32_t seq = 0;
  if (c->knobs.poll) {
    seq = next_seq(c);
    c->poll_words = 0;   // (one word, written by the combining block)
  }
  const bool acker = c->acker_r >= 0.f;
  HIPCK(c, smpc_launch_combine(d_tuples, n, T, c->dev.neg_inv_temp, c->c_vx_max, c->c_vx_min,
                               c->c_vy, c->c_wz, c->d_out.get(), c->d_out.get() + SMPC_RESULT_AT(T), d_furthest_used,
                               c->h_out_dev, acker ? 0u : seq, c->stream));
  if (acker) HIPCK(c, smpc_launch_ackermann(c->d_out.get(), c->h_out_dev, T, c->acker_r, seq, c->stream));
  return SMPC_OK;
}

// control_sequence_.vy is never written for a non-holonomic model (optimizer.cpp:387-389):
// the caller's row stays as it was
void store_control_sequence(const smpc_ctx* c, float* u_inout)
{
  const uint32_t T = c->cfg.time_steps;
  if (c->holonomic) {
    memcpy(u_inout, c->h_out.get(), 3 * T * sizeof(float));
    return;
  }
  memcpy(u_inout, c->h_out.get(), T * sizeof(float));
  memcpy(u_inout + 2 * T, c->h_out.get() + 2 * T, T * sizeof(float));
}

// the pass's echo of the tick block's number (SmpcDev::canary): anything but this tick's number
// means the kernels did not read the block the host handed over
static int check_canary(smpc_ctx* c)
{
  c->launched = false;
  if (!c->tick.canary_expect) return SMPC_OK;
  const uint32_t got = reinterpret_cast<const volatile uint32_t*>(c->h_out.get())[SMPC_RESULT_AT(c->cfg.time_steps) + SMPC_R_CANARY];
  if (got == c->tick.canary_expect) return SMPC_OK;
  char msg[200];
  snprintf(msg, sizeof(msg), "the scoring pass read tick block %u, not %u: the per-tick upload did not reach the "
           "device in time (CPU stores through the BAR: %s); SMPC_NO_BAR_TICK=1 selects the copy", got, c->tick.canary_expect,
           c->tick.bar_tick ? "on" : "off");
  c->tick.bar_tick = false;   // later ticks of this ctx take the copy
  return fail(c, SMPC_ERR_DEVICE, msg);
}

int fetch_out(smpc_ctx* c)
{
  // The finishing kernel wrote u and the result into host-mapped memory and then the
  // tick's sequence number: spin on that word (a few microseconds sooner than the
  // runtime's stream wait), and fall back to the stream wait, which also surfaces errors.
  if (c->poll_seq) {
    const volatile uint32_t* flag =
      reinterpret_cast<const volatile uint32_t*>(c->h_out.get() + SMPC_RESULT_AT(c->cfg.time_steps) + SMPC_R_DONE);
    const uint32_t want = c->poll_seq;
    c->poll_seq = 0;
    const uint32_t nwords = c->poll_words;   // > 0: one word per reducing block, from flag[1] on (SMPC_R_BLOCK_DONE)
    static_assert(SMPC_R_BLOCK_DONE == SMPC_R_DONE + 1u, "the per-block words follow the completion word");
    c->poll_words = 0;
    auto arrived = [&]() {
      if (nwords == 0) return *flag == want;
      for (uint32_t r = 0; r < nwords; ++r)
        if (flag[1 + r] != want) return false;
      return true;
    };
    for (uint32_t spin = 0; spin < 4000000u; ++spin) {
      if (arrived()) {
        __atomic_thread_fence(__ATOMIC_ACQUIRE);
        // smpc_grid_tail's mark: a reducing block gave up waiting for the grid's other blocks
        if (tick_result(c).mark() == SMPC_MARK_TAIL_LATE)
          return fail(c, SMPC_ERR_DEVICE, "the scoring launch's reduction did not see every block's partial");
        return check_canary(c);
      }
      __builtin_ia32_pause();
    }
  }
  HIPCK(c, hipStreamSynchronize(c->stream));
  return check_canary(c);
}

float profile_pass_ms(smpc_ctx* c)
{
  float sum = 0.f;
  uint32_t n = 0;
  for (uint32_t i = 0; i + 1 < c->evp_used; i += 2) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, c->evp[i].get(), c->evp[i + 1].get()) == hipSuccess) {
      sum += ms;
      n++;
    }
  }
  return n ? sum / n : 0.f;
}

int fill_tick_out(smpc_ctx* c, smpc_tick_out* out, bool fail_flag, bool furthest_valid, uint32_t furthest,
                  const float* non_colliding, bool device_ms)
{
  if (!out) return SMPC_OK;
  const TickResult r = tick_result(c);
  memset(out, 0, sizeof(*out));
  out->fail_flag = fail_flag ? 1 : 0;
  out->furthest_valid = furthest_valid ? 1 : 0;
  out->furthest_reached_path_point = furthest;
  out->non_colliding = static_cast<uint32_t>(non_colliding ? *non_colliding : r.non_colliding());
  out->min_cost = r.min_cost();
  out->sum_w = r.sum_w();
  out->passes = c->passes;
  if (device_ms && (c->cfg.flags & SMPC_FLAG_PROFILE)) {
    // the polled flag can beat the event's completion signal by a few microseconds
    HIPCK(c, hipEventSynchronize(c->ev1.get()));
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, c->ev0.get(), c->ev1.get()) == hipSuccess) out->device_ms = ms;
  }
  out->score_pass_ms = profile_pass_ms(c);
  out->pass_kind = c->last_pass_kind;
  return SMPC_OK;
}

// What the reference had scored when a collision critic found every rollout colliding
// (critic_manager.cpp:70-73 stops after it): the list of include/smpc.h up to and including
// the first enabled collision critic — Constraint, Cost | Obstacles.
uint32_t fail_only_flags(const smpc_ctx* c)
{
  // (with its consider_footprint switch: the re-score has to find the same collisions)
  const uint32_t coll = (c->gate_flags & SD_COST) ? (SD_COST | SD_FP_COST) : (SD_OBSTACLES | SD_FP_OBSTACLES);
  return c->gate_flags & (SD_CONSTRAINT | coll | SD_STORE_TRAJ | SD_TRACK_UNKNOWN);
}

uint32_t scoring_flags(const smpc_ctx* c, bool fail_sticky)
{
  // CriticManager::evalTrajectoriesScores breaks on fail_flag (critic_manager.cpp:70-73)
  const uint32_t keep = SD_STORE_TRAJ | SD_TRACK_UNKNOWN;
  return fail_sticky ? (c->gate_flags & keep) : c->gate_flags;
}

// the developer knobs (smpc_ctx.h: Knobs), read once per context
static Knobs read_knobs()
{
  Knobs k;
  auto set = [](const char* name) {return getenv(name) != nullptr;};
  auto number = [](const char* name, int unset) {const char* e = getenv(name); return e ? atoi(e) : unset;};
  if (const char* e = getenv("SMPC_PASS"))
    k.pass = !strcmp(e, "wave") ? Knobs::kWave : !strcmp(e, "lane") ? Knobs::kLane : !strcmp(e, "split") ? Knobs::kSplit : Knobs::kAuto;
  k.no_split = set("SMPC_NO_SPLIT");
  k.split_nseg = static_cast<uint32_t>(std::max(0, number("SMPC_SPLIT_NSEG", 0)));
  k.lane_reread = number("SMPC_LANE_REREAD", 0) != 0;
  k.half_blocks = !set("SMPC_NO_HALF_BLOCKS");
  k.max_blocks_per_cu = static_cast<uint32_t>(std::max(0, number("SMPC_MAX_BLOCKS_PER_CU", 0)));
  k.balanced_grid = !set("SMPC_NO_BALANCED_GRID");
  k.fused_reduce = set("SMPC_FUSED_REDUCE");   // (per context: tests compare the two)
  k.no_inline_tick = set("SMPC_NO_INLINE_TICK");
  k.pinned_tick = set("SMPC_PINNED_TICK");
  k.poll = !set("SMPC_NO_POLL");
  k.bar_tick = !set("SMPC_NO_BAR_TICK");
  k.hdp_flush = !set("SMPC_NO_HDP_FLUSH");
  k.repeat_pass = set("SMPC_DEBUG_REPEAT_PASS");
  k.stale_tick = static_cast<uint32_t>(number("SMPC_DEBUG_STALE_TICK", 0));
  k.small_window = set("SMPC_SMALL_WINDOW");
  k.window_side_max = number("SMPC_WINDOW_SIDE_MAX", -1);
  k.furthest_prune = number("SMPC_FURTHEST_PRUNE", 1) != 0;
  if (const char* e = getenv("SMPC_FOOTPRINT_PASS")) k.footprint_general = !strcmp(e, "general");
  if (const char* e = getenv("SMPC_NONHOLO_PASS")) k.nonholo_omni = !strcmp(e, "omni");
  return k;
}

// developer aid (SMPC_TICK_TIMING=1): where the host's share of a tick goes, printed every 1024 ticks
using clk = std::chrono::steady_clock;
static void report_tick_timing(clk::time_point t_in, clk::time_point t_prep, clk::time_point t_launch, clk::time_point t_fetch)
{
  static thread_local double acc[5] = {0, 0, 0, 0, 0};   // (per calling thread: contexts may tick on several)
  static thread_local unsigned n = 0;
  static thread_local clk::time_point t_prev_out;
  const auto t_out = clk::now();
  auto us = [](clk::time_point a, clk::time_point b) {return std::chrono::duration<double, std::micro>(b - a).count();};
  if (n > 0) acc[0] += us(t_prev_out, t_in);   // the caller, between two ticks
  acc[1] += us(t_in, t_prep);
  acc[2] += us(t_prep, t_launch);
  acc[3] += us(t_launch, t_fetch);
  acc[4] += us(t_fetch, t_out);
  t_prev_out = t_out;
  if (++n == 1024) {
    fprintf(stderr, "[smpc tick timing] caller %.2f us, prepare + upload %.2f, launches %.2f, wait %.2f, collect %.2f (per tick, %u ticks)\n",
            acc[0] / (n - 1), acc[1] / n, acc[2] / n, acc[3] / n, acc[4] / n, n);
    n = 0;
    for (double& a : acc) a = 0;
  }
}
}  // namespace smpc_impl

using namespace smpc_impl;

extern "C" {

void smpc_config_default(smpc_config* c)
{
  memset(c, 0, sizeof(*c));
  c->batch_size = 1000;   // ref src/optimizer.cpp:69-82
  c->time_steps = 56;
  c->iteration_count = 1;
  c->motion_model = SMPC_MODEL_OMNI;
  c->model_dt = 0.05f;
  c->temperature = 0.3f;
  c->gamma = 0.015f;
  c->vx_max = 0.5f;
  c->vx_min = -0.35f;
  c->vy_max = 0.5f;
  c->wz_max = 1.9f;
  c->vx_std = 0.2f;
  c->vy_std = 0.2f;
  c->wz_std = 0.4f;
  c->device = -1;
  c->ackermann_min_turning_r = 0.2f;   // ref motion_models.hpp:94
}

void smpc_critic_params_default(smpc_critic_params* p)
{
  memset(p, 0, sizeof(*p));
  p->obstacles = {1, 0, 1, 1.5f, 20.0f, 10000.0f, 0.10f, 0.5f};
  p->path_align = {1, 0, 1, 10.0f, 0.07f, 20, 4, 0.5f};
  p->path_follow = {1, 1, 5.0f, 1.4f, 6};
  p->goal_angle = {1, 1, 3.0f, 0.5f};
  p->prefer_forward = {1, 1, 5.0f, 0.5f};
  // the other registered critics: initialize() defaults, not in the list (enabled 0)
  p->cost = {0, 0, 1, 3.81f, 300.0f, 1000000.0f, 0.5f};
  p->goal = {0, 1, 5.0f, 1.4f};
  p->constraint = {0, 1, 4.0f, 0.5f, 0.5f, -0.35f};
  p->twirling = {0, 1, 10.0f};
  p->path_angle = {0, 1, 2.0f, 4, 0.5f, 1.2f, 1, -0.35f};
  p->velocity_deadband = {0, 1, 35.0f, {0.0f, 0.0f, 0.0f}};
  p->path_align_legacy = {0, 0, 1, 10.0f, 0.07f, 20, 4, 0.5f};   // path_align_legacy_critic.cpp:26-37
}

int smpc_abi_version(void) {return SMPC_ABI_VERSION;}

const char* smpc_build_info(void)
{
  return "libsmpc (MI355X-native sampling-MPC hot path), HIP gfx950, built " __DATE__ " " __TIME__;
}

const char* smpc_last_error(const smpc_ctx* ctx)
{
  return ctx ? ctx->err.c_str() : g_create_error.c_str();
}

int smpc_create(const smpc_config* cfg, smpc_ctx** out)
{
  if (!cfg || !out) return fail(nullptr, SMPC_ERR_INVALID, "null argument");
  *out = nullptr;
  if (cfg->batch_size == 0 || cfg->time_steps == 0 || cfg->iteration_count == 0)
    return fail(nullptr, SMPC_ERR_INVALID, "batch_size, time_steps, iteration_count must be > 0");
  if (cfg->motion_model > SMPC_MODEL_ACKERMANN)
    return fail(nullptr, SMPC_ERR_UNSUPPORTED, "motion_model must be Omni, DiffDrive or Ackermann");
  if (cfg->motion_model == SMPC_MODEL_ACKERMANN && !(cfg->ackermann_min_turning_r >= 0.f))
    return fail(nullptr, SMPC_ERR_INVALID, "ackermann_min_turning_r must be >= 0");
  if (cfg->time_steps > 64 * SMPC_MAX_R)
    return fail(nullptr, SMPC_ERR_UNSUPPORTED, "time_steps > 256");
  if (!(cfg->temperature > 0.f) || !(cfg->model_dt > 0.f))
    return fail(nullptr, SMPC_ERR_INVALID, "temperature and model_dt must be > 0");
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev == 0)
    return fail(nullptr, SMPC_ERR_DEVICE,
                std::string("no HIP device: ") + (e != hipSuccess ? hipGetErrorString(e) : "count 0") +
                " (libsmpc has no CPU fallback)");
  smpc_ctx* c = new (std::nothrow) smpc_ctx();
  if (!c) return fail(nullptr, SMPC_ERR_NOMEM, "out of host memory");
  c->cfg = *cfg;
  c->knobs = read_knobs();
  smpc_critic_params_default(&c->critics);
  c->holonomic = cfg->motion_model == SMPC_MODEL_OMNI;
  c->acker_r = cfg->motion_model == SMPC_MODEL_ACKERMANN ? cfg->ackermann_min_turning_r : -1.f;
  c->c_vx_max = cfg->vx_max; c->c_vx_min = cfg->vx_min; c->c_vy = cfg->vy_max; c->c_wz = cfg->wz_max;
  int dev = cfg->device;
  if (dev < 0) {
    if (hipGetDevice(&dev) != hipSuccess) dev = 0;
  }
  c->device = dev;
#define CK(call)                                                                        \
  do {                                                                                  \
    hipError_t e__ = (call);                                                            \
    if (e__ != hipSuccess) {                                                            \
      g_create_error = std::string(#call) + ": " + hipGetErrorString(e__);              \
      free_ctx(c);                                                                      \
      return SMPC_ERR_DEVICE;                                                           \
    }                                                                                   \
  } while (0)
  CK(hipSetDevice(dev));
  hipDeviceProp_t prop;
  CK(hipGetDeviceProperties(&prop, dev));
  c->num_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  {
    int large_bar = 0;
    if (hipDeviceGetAttribute(&large_bar, hipDeviceAttributeIsLargeBar, dev) != hipSuccess) large_bar = 0;
    c->tick.bar_tick = large_bar != 0 && c->knobs.bar_tick;
    if (c->tick.bar_tick && c->knobs.hdp_flush) {
      c->tick.hdp_flush = find_hdp_flush(dev);
      // without the device's HDP flush register the stores may sit in the host data path's
      // cache when the pass starts: such a device takes the stream copy (SMPC_NO_HDP_FLUSH=1, an
      // experiment, keeps the stores without the flush; the canary then guards every tick)
      if (!c->tick.hdp_flush) c->tick.bar_tick = false;
    }
  }
  CK(c->own_stream.ensure(hipStreamNonBlocking));
  c->stream = c->own_stream.get();
  if (getenv("SMPC_LANE_TIMELINE")) {
    static_assert(SMPC_TAIL_STAMPS_AT == 8192 + kMaxGrid * 8, "the tail's stamps sit behind the lane pass's");
    CK(c->d_timeline.ensure(SMPC_SCAN_COUNT_AT + kMaxGrid * 8));
    CK(hipMemset(c->d_timeline.get(), 0, (SMPC_SCAN_COUNT_AT + kMaxGrid * 8) * sizeof(unsigned long long)));
  }
  CK(c->ev0.ensure());
  CK(c->ev_map.ensure(hipEventDisableTiming));
  CK(c->ev1.ensure());
  for (Event& e : c->evp) CK(e.ensure());
  const uint32_t T = cfg->time_steps;
  c->R = T <= 64 ? 1 : (T <= 128 ? 2 : 4);
  const size_t BT = static_cast<size_t>(cfg->batch_size) * T, n = BT * sizeof(float);
  CK(c->noise.cur.nvx.ensure(BT));
  CK(c->noise.cur.nvy.ensure(BT));
  if (!c->holonomic) CK(hipMemset(c->noise.cur.nvy.get(), 0, n));   // noises_vy_ (noise_generator.cpp:76-91)
  CK(c->noise.cur.nwz.ensure(BT));
  {
    // which streaming pass: a wave per rollout (latency, small batches) or a lane per
    // rollout (throughput, large batches); SMPC_PASS=wave|lane overrides for experiments
    bool tpr = cfg->batch_size >= kLaneMinBatch && cfg->time_steps <= kLaneMaxT;
    // (smpc_pass_split, T = 64: the group-major noise from kSplitMinBatch rollouts up; plan_launch keeps
    // the lane pass itself for batches from kLaneMinBatch up, unless it is asked for)
    if (cfg->time_steps <= 64 && cfg->time_steps >= 36 && (cfg->time_steps & 3u) == 0 && cfg->batch_size >= kSplitMinBatch &&
        !c->knobs.no_split)
      tpr = true;
    if (cfg->flags & SMPC_FLAG_WAVE_PER_ROLLOUT) tpr = false;
    if (cfg->flags & SMPC_FLAG_LANE_PER_ROLLOUT) {
      tpr = true;
      c->lane_forced = true;
    }
    if (c->knobs.pass == Knobs::kWave) tpr = false;
    if (c->knobs.pass == Knobs::kLane || c->knobs.pass == Knobs::kSplit) {   // (split: wherever the instance applies, whatever the batch)
      tpr = true;
      c->lane_forced = true;
    }
    if (cfg->flags & SMPC_FLAG_STORE_TRAJECTORIES) tpr = false;   // visualisation path: wave pass
    // the group-major copies (smpc_dev.h: SMPC_GM_INDEX): the batch padded to whole groups of 64
    const size_t ngm = SMPC_GM_ELEMS(cfg->batch_size, T) * sizeof(float);
    if (3ull * ngm >= (1ull << 32)) tpr = false;   // its buffer descriptor spans the three noise tensors
    c->noise.use_tpr = tpr;
    if (tpr) {
      // back to back: the lane pass addresses the three through one buffer descriptor
      CK(c->noise.cur.tvx.ensure(3 * ngm / sizeof(float)));
      c->noise.cur.tvy = c->noise.cur.tvx.get() + ngm / sizeof(float);
      c->noise.cur.twz = c->noise.cur.tvy + ngm / sizeof(float);
      CK(hipMemset(c->noise.cur.tvx.get(), 0, 3 * ngm));   // the padding steps of a ragged horizon, and vy of a non-holonomic model
      CK(lane_set_lds_limit(static_cast<int>(kLdsPerCu)));
      CK(split_set_lds_limit(static_cast<int>(kLdsPerCu)));
    }
  }
  CK(c->d_costs[0].ensure(cfg->batch_size));
  CK(c->d_costs[1].ensure(cfg->batch_size));
  CK(hipMemset(c->d_costs[0].get(), 0, cfg->batch_size * sizeof(float)));
  CK(hipMemset(c->d_costs[1].get(), 0, cfg->batch_size * sizeof(float)));
  if (cfg->flags & SMPC_FLAG_STORE_TRAJECTORIES) {
    for (int i = 0; i < 3; ++i) {
      CK(c->d_traj[i].ensure(BT));
      CK(hipMemset(c->d_traj[i].get(), 0, n));
    }
  }
  c->tick.cap = tick_layout(T, SMPC_MAX_PATH).total;
  CK(c->tick.own_d.ensure(c->tick.cap));
  CK(c->tick.own_h.ensure(c->tick.cap));
  c->tick.view_own();
  CK(c->d_lut.ensure(256));
  CK(hipMemset(c->d_lut.get(), 0, 256 * sizeof(SmpcLut)));
  CK(c->d_lut_fp.ensure(512));
  CK(hipMemset(c->d_lut_fp.get(), 0, 512 * sizeof(SmpcLut)));
  CK(c->h_lut_fp.ensure(512));
  CK(c->h_lut.ensure(256));
  const size_t TL = SMPC_TUPLE_HEADER + 3 * static_cast<size_t>(T);
  CK(c->d_partials.ensure(kMaxGrid * TL + 16));   // + the canary's slot (SMPC_CANARY_SLOT)
  CK(hipMemset(c->d_partials.get(), 0, (kMaxGrid * TL + 16) * sizeof(float)));
  CK(c->d_tuple.ensure(TL));
  CK(c->d_out.ensure(SMPC_RESULT_FLOATS(T)));
  CK(c->d_u_iter.ensure(3 * T));
  // (the mirror ends in kPollWords completion words, one per publishing block: smpc_reduce_blocks(T), at most 25 at T = 256)
  CK(c->h_out.ensure(SMPC_RESULT_HOST_FLOATS(T), hipHostMallocMapped));
  memset(c->h_out.get(), 0, SMPC_RESULT_HOST_FLOATS(T) * sizeof(float));
  CK(hipHostGetDevicePointer(reinterpret_cast<void**>(&c->h_out_dev), c->h_out.get(), 0));
  CK(c->d_furthest.ensure(SMPC_SCRATCH_WORDS));
  CK(hipMemset(c->d_furthest.get(), 0, SMPC_SCRATCH_WORDS * sizeof(uint32_t)));
  CK(wave_set_lds_limit(static_cast<int>(kLdsPerCu)));
  // the memsets above went to the default stream; the ctx works on its own non-blocking one
  CK(hipDeviceSynchronize());
#undef CK
  *out = c;
  return SMPC_OK;
}

void smpc_destroy(smpc_ctx* ctx) {free_ctx(ctx);}

int smpc_reset(smpc_ctx* c)
{
  if (!c) return SMPC_ERR_INVALID;
  HIPCK(c, hipSetDevice(c->device));
  // Optimizer::reset (optimizer.cpp:116-132): constraints back to base, costs zero,
  // NoiseGenerator::reset re-draws (noise_generator.cpp:76-95)
  c->c_vx_max = c->cfg.vx_max; c->c_vx_min = c->cfg.vx_min;
  c->c_vy = c->cfg.vy_max; c->c_wz = c->cfg.wz_max;
  HIPCK(c, hipMemsetAsync(c->d_costs[0].get(), 0, c->cfg.batch_size * sizeof(float), c->stream));
  HIPCK(c, hipMemsetAsync(c->d_costs[1].get(), 0, c->cfg.batch_size * sizeof(float), c->stream));
  c->tick_ready = false;
  c->pred.forget();
  if (c->noise.rng_mode) {
    c->noise.epoch++;
    return draw_noise(c);
  }
  HIPCK(c, hipStreamSynchronize(c->stream));
  return SMPC_OK;
}

int smpc_set_constraints(smpc_ctx* c, float vx_max, float vx_min, float vy_max, float wz_max)
{
  if (!c) return SMPC_ERR_INVALID;
  c->c_vx_max = vx_max; c->c_vx_min = vx_min; c->c_vy = vy_max; c->c_wz = wz_max;
  return SMPC_OK;
}

int smpc_set_footprint(smpc_ctx* c, const double* xy, uint32_t n_points, double circumscribed_radius,
                       double layer_cost_scaling_factor)
{
  if (!c || (n_points && !xy)) return fail(c, SMPC_ERR_INVALID, "null argument");
  if (n_points > SMPC_MAX_FOOTPRINT) return fail(c, SMPC_ERR_UNSUPPORTED, "footprint with more than 16 points");
  c->fp_x.clear();
  c->fp_y.clear();
  for (uint32_t i = 0; i < n_points; ++i) {
    c->fp_x.push_back(xy[2 * i]);
    c->fp_y.push_back(xy[2 * i + 1]);
  }
  c->fp_circumscribed_radius = circumscribed_radius;
  c->fp_layer_scale = layer_cost_scaling_factor;
  c->critics_version++;
  return SMPC_OK;
}

int smpc_set_critics(smpc_ctx* c, const smpc_critic_params* p)
{
  if (!c || !p) return SMPC_ERR_INVALID;
  c->critics = *p;
  c->critics_version++;
  return SMPC_OK;
}

int smpc_set_costmap(smpc_ctx* c, const uint8_t* cells, uint32_t width, uint32_t height,
                     double origin_x, double origin_y, double resolution, int track_unknown,
                     float inscribed_radius, float cost_scaling_factor, float inflation_radius)
{
  if (!c) return SMPC_ERR_INVALID;
  if (!cells || width == 0 || height == 0 || !(resolution > 0.0))
    return fail(c, SMPC_ERR_INVALID, "bad costmap");
  HIPCK(c, hipSetDevice(c->device));
  int rc = wait_map_upload(c);   // the previous upload reads the mirror this call overwrites
  if (rc != SMPC_OK) return rc;
  HostCostmap& m = c->map;
  const size_t bytes = static_cast<size_t>(width) * height;
  bool same_size = m.set && m.W == width && m.H == height;
  if (bytes > c->d_map.capacity()) {
    // the stream may still read the old device copy (an un-waited tick): drain it first
    HIPCK(c, hipStreamSynchronize(c->stream));
    HIPCK(c, c->d_map.ensure((bytes + 255) / 256 * 256));
    same_size = false;
  }
  if (bytes > m.cells.capacity()) {
    HIPCK(c, m.cells.ensure((bytes + 4095) / 4096 * 4096));
    same_size = false;
  }
  // The controller hands over the whole costmap every tick (controller.cpp:99-103) while the
  // costmap itself changes at its own, lower update rate: only the band of rows that differ
  // from the mirror is copied and uploaded (nothing at all for an unchanged map).
  uint32_t y0 = height, y1 = 0;
  if (same_size) {
    for (uint32_t y = 0; y < height; ++y) {
      const size_t o = static_cast<size_t>(y) * width;
      if (memcmp(m.cells.get() + o, cells + o, width) != 0) {
        memcpy(m.cells.get() + o, cells + o, width);
        if (y < y0) y0 = y;
        y1 = y;
      }
    }
  } else {
    memcpy(m.cells.get(), cells, bytes);
    y0 = 0;
    y1 = height - 1;
  }
  // the lookup tables depend on these, not on the cells
  const bool same_params = m.set && m.res == resolution && m.track_unknown == (track_unknown != 0) &&
    m.inscribed_radius == inscribed_radius && m.cost_scaling_factor == cost_scaling_factor &&
    m.inflation_radius == inflation_radius;
  m.W = width; m.H = height; m.ox = origin_x; m.oy = origin_y; m.res = resolution;
  m.track_unknown = track_unknown != 0;
  m.inscribed_radius = inscribed_radius;
  m.cost_scaling_factor = cost_scaling_factor;
  m.inflation_radius = inflation_radius;
  m.set = true;
  if (!same_params) c->map_version++;
  c->map_bytes_last = 0;
  if (y0 <= y1) {
    const size_t o = static_cast<size_t>(y0) * width, n = static_cast<size_t>(y1 - y0 + 1) * width;
    HIPCK(c, hipMemcpyAsync(c->d_map.get() + o, m.cells.get() + o, n, hipMemcpyHostToDevice, c->stream));
    HIPCK(c, hipEventRecord(c->ev_map.get(), c->stream));
    c->map_pending = true;
    c->map_bytes_last = n;
    c->map_bytes_total += n;
  }
  return SMPC_OK;
}

int smpc_update_costmap_region(smpc_ctx* c, const uint8_t* cells, uint32_t row_stride, uint32_t x0,
                               uint32_t y0, uint32_t width, uint32_t height)
{
  if (!c || !cells) return SMPC_ERR_INVALID;
  HostCostmap& m = c->map;
  if (!m.set) return fail(c, SMPC_ERR_STATE, "smpc_set_costmap first");
  if (width == 0 || height == 0 || row_stride < width || x0 >= m.W || y0 >= m.H || width > m.W - x0 ||
      height > m.H - y0)
    return fail(c, SMPC_ERR_INVALID, "region outside the costmap");
  HIPCK(c, hipSetDevice(c->device));
  int rc = wait_map_upload(c);
  if (rc != SMPC_OK) return rc;
  for (uint32_t y = 0; y < height; ++y)
    memcpy(m.cells.get() + static_cast<size_t>(y0 + y) * m.W + x0, cells + static_cast<size_t>(y) * row_stride, width);
  const size_t o = static_cast<size_t>(y0) * m.W + x0;
  HIPCK(c, hipMemcpy2DAsync(c->d_map.get() + o, m.W, m.cells.get() + o, m.W, width, height, hipMemcpyHostToDevice,
                            c->stream));
  HIPCK(c, hipEventRecord(c->ev_map.get(), c->stream));
  c->map_pending = true;
  c->map_bytes_last = static_cast<uint64_t>(width) * height;
  c->map_bytes_total += c->map_bytes_last;
  return SMPC_OK;
}

int smpc_costmap_upload_bytes(const smpc_ctx* c, uint64_t* last_call, uint64_t* total)
{
  if (!c) return SMPC_ERR_INVALID;
  if (last_call) *last_call = c->map_bytes_last;
  if (total) *total = c->map_bytes_total;
  return SMPC_OK;
}

int smpc_optimize(smpc_ctx* c, const smpc_tick_in* in, float* u_inout, smpc_tick_out* out)
{
  if (!c || !in || !u_inout) return fail(c, SMPC_ERR_INVALID, "null argument");
  static const bool timing = getenv("SMPC_TICK_TIMING") != nullptr;   // (report_tick_timing)
  clk::time_point t_in, t_prep, t_launch, t_fetch;
  if (timing) t_in = clk::now();
  HIPCK(c, hipSetDevice(c->device));
  int rc = begin_tick(c, in, u_inout);
  if (rc != SMPC_OK) return rc;
  if (timing) t_prep = clk::now();
  const uint32_t T = c->cfg.time_steps;
  const TickResult res = tick_result(c);
  bool fail_sticky = c->fail_in;
  bool fail_flag = fail_sticky;
  bool fetched = false;
  // One scoring pass that finishes the control sequence: the launch, the end of the call's GPU
  // time when profiling (`timed`), and the host round trip for the result (`fetch`).  dF: the
  // furthest point on the device, for the critics and reported as the one they used.
  auto score = [&](uint32_t flags, const float* u_dev, const float* dF, uint32_t hintS, bool timed, bool fetch) -> int {
    int e = launch_score(c, flags, u_dev, dF, hintS, c->d_tuple.get(), true, dF);
    if (e != SMPC_OK) return e;
    if (timed && (c->cfg.flags & SMPC_FLAG_PROFILE)) HIPCK(c, hipEventRecord(c->ev1.get(), c->stream));
    const bool first = c->passes == 1;
    if (timing && first) t_launch = clk::now();
    if (fetch) e = fetch_out(c);
    if (timing && first) t_fetch = clk::now();
    fetched = fetch;
    return e;
  };
  // furthest_reached_path_point of this tick: evaluated once, then cached
  // (setPathFurthestPointIfNotSet, utils.hpp:350-355)
  bool S_known = false, S_on_device = false;
  uint32_t S_host = 0;
  float F_host = 0.f;
  bool have_nc_obstacles = false;   // (two_coll_fp: ObstaclesCritic's own non-colliding count, the last one assigned)
  float nc_obstacles = 0.f;
  const bool speculate = !(c->cfg.flags & SMPC_FLAG_NO_SPECULATION);
  for (uint32_t it = 0; it < c->cfg.iteration_count; ++it) {
    uint32_t flags = scoring_flags(c, fail_sticky);
    const uint32_t acc = it > 0 ? SD_ACCUMULATE : 0u;
    flags |= acc;
    have_nc_obstacles = false;   // (the count reported is the LAST iteration's, like every other output)
    // a later iteration starts from what the previous one left in d_out — from a COPY of it: the
    // reduction of this iteration's first pass overwrites d_out, and a second pass of the same
    // iteration (speculation miss, all-collide re-score, the counting pass below) has to read
    // the same control sequence as the first
    const float* u_dev = nullptr;
    if (it > 0) {
      HIPCK(c, hipMemcpyAsync(c->d_u_iter.get(), c->d_out.get(), 3 * T * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
      u_dev = c->d_u_iter.get();
      begin_limit_iteration(c, u_dev);   // this iteration limits the stored noise afresh, against its own u
    }
    c->costs_cur = it & 1;
    const float* dF = nullptr;
    uint32_t hintS = 0;
    bool spec_try = false;
    if (flags & SD_NEED_FURTHEST) {
      if (S_known) {
        hintS = S_host;
      } else if (S_on_device) {
        dF = c->d_furthest.get();
      } else if (speculate && c->pred.hint_valid) {
        // score with the previous tick's furthest point; the pass reports the true
        // one and a miss is re-scored below, so the result is exact either way
        spec_try = true;
        hintS = c->pred.hint;
        flags |= SD_LOCAL_FURTHEST;
      } else {
        rc = launch_furthest(c, c->d_furthest.get());
        if (rc != SMPC_OK) return rc;
        S_on_device = true;
        dF = c->d_furthest.get();
      }
    }
    // ---- the iteration's first pass.  One host round trip where something hangs on it: fail_flag
    // (obstacles_critic.cpp:177), the true furthest point, and on the last iteration the result itself
    const bool last = it + 1 == c->cfg.iteration_count;
    rc = score(flags, u_dev, dF, hintS, true, (flags & (SD_OBSTACLES | SD_COST)) || spec_try || last);
    if (rc != SMPC_OK) return rc;
    if (fetched && dF) {
      F_host = res.F_used();
      S_host = smpc_furthest_index(F_host);
      S_known = true;
    }
    // ---- speculation miss: once more with the true furthest point
    if (spec_try) {
      F_host = res.F_local();
      S_host = smpc_furthest_index(F_host);
      S_known = true;
      if (S_host != hintS) {
        c->spec_misses++;
        flags &= ~SD_LOCAL_FURTHEST;
        rc = score(flags, u_dev, nullptr, S_host, true, true);
        if (rc != SMPC_OK) return rc;
      }
    }
    // ---- debug repeat (tests: a second pass of the iteration must see the first one's inputs)
    if (c->knobs.repeat_pass) {
      rc = score(flags & ~SD_LOCAL_FURTHEST, u_dev, nullptr, S_known ? S_host : hintS, false, true);
      if (rc != SMPC_OK) return rc;
    }
    // ---- both collision critics with a footprint: ObstaclesCritic's own count
    bool failed_at_obstacles = false;
    if (c->two_coll_fp && (flags & SD_OBSTACLES) && (flags & SD_COST) && res.non_colliding() != 0.0f) {
      // CostCritic (scored first, its count is the one the pass reports) let some rollouts
      // through; ObstaclesCritic is scored next and, with a footprint in play, decides on its OWN
      // collisions (obstacles_critic.cpp:177 assigns fail_flag).  One pass that scores it alone
      // counts them; then either the manager stopped behind it (critic_manager.cpp:70-73:
      // Constraint, Cost, Obstacles were scored) or everything is scored again.
      const uint32_t keep = SD_STORE_TRAJ | SD_TRACK_UNKNOWN;
      rc = score((c->gate_flags & (SD_OBSTACLES | SD_FP_OBSTACLES | keep)) | acc, u_dev, nullptr, 0, false, true);
      if (rc != SMPC_OK) return rc;
      nc_obstacles = res.non_colliding();
      uint32_t again = flags & ~SD_LOCAL_FURTHEST;
      if (nc_obstacles == 0.0f) {
        failed_at_obstacles = true;
        fail_flag = true;
        fail_sticky = true;
        again = (c->gate_flags & (SD_CONSTRAINT | SD_COST | SD_FP_COST | SD_OBSTACLES | SD_FP_OBSTACLES | keep)) | acc;
      }
      rc = score(again, u_dev, nullptr, S_known ? S_host : 0u, true, true);
      if (rc != SMPC_OK) return rc;
      have_nc_obstacles = true;
    }
    // ---- every rollout collides: the critics after Obstacles were not scored in the reference
    // (critic_manager.cpp:70-73); redo this iteration with Obstacles only so that costs and u
    // match it exactly
    if (!failed_at_obstacles && (flags & (SD_OBSTACLES | SD_COST)) && res.non_colliding() == 0.0f) {
      fail_flag = true;
      fail_sticky = true;
      rc = score(fail_only_flags(c) | acc, u_dev, nullptr, 0, true, false);
      if (rc != SMPC_OK) return rc;
    }
  }
  if (!fetched) {
    rc = fetch_out(c);
    if (rc != SMPC_OK) return rc;
  }
  if (S_known) remember_furthest(c, in, F_host);
  store_control_sequence(c, u_inout);
  rc = fill_tick_out(c, out, fail_flag, S_known, S_known ? S_host : 0u, have_nc_obstacles ? &nc_obstacles : nullptr, true);
  if (rc != SMPC_OK) return rc;
  if (timing) report_tick_timing(t_in, t_prep, t_launch, t_fetch);
  return SMPC_OK;
}

int smpc_get_trajectories(smpc_ctx* c, float* x, float* y, float* yaws)
{
  if (!c) return SMPC_ERR_INVALID;
  if (!(c->cfg.flags & SMPC_FLAG_STORE_TRAJECTORIES))
    return fail(c, SMPC_ERR_STATE, "ctx was created without SMPC_FLAG_STORE_TRAJECTORIES");
  HIPCK(c, hipSetDevice(c->device));
  HIPCK(c, hipStreamSynchronize(c->stream));
  const size_t n = static_cast<size_t>(c->cfg.batch_size) * c->cfg.time_steps * sizeof(float);
  if (x) HIPCK(c, hipMemcpy(x, c->d_traj[0].get(), n, hipMemcpyDeviceToHost));
  if (y) HIPCK(c, hipMemcpy(y, c->d_traj[1].get(), n, hipMemcpyDeviceToHost));
  if (yaws) HIPCK(c, hipMemcpy(yaws, c->d_traj[2].get(), n, hipMemcpyDeviceToHost));
  return SMPC_OK;
}

int smpc_get_costs(smpc_ctx* c, float* costs)
{
  if (!c || !costs) return SMPC_ERR_INVALID;
  HIPCK(c, hipSetDevice(c->device));
  HIPCK(c, hipStreamSynchronize(c->stream));
  HIPCK(c, hipMemcpy(costs, c->d_costs[c->costs_cur].get(), c->cfg.batch_size * sizeof(float),
                     hipMemcpyDeviceToHost));
  return SMPC_OK;
}

int smpc_set_stream(smpc_ctx* c, void* hip_stream)
{
  if (!c) return SMPC_ERR_INVALID;
  const int rc = wait_map_upload(c);   // it went out on the stream being left
  if (rc != SMPC_OK) return rc;
  c->stream = hip_stream == SMPC_STREAM_OWN ? c->own_stream.get() : static_cast<hipStream_t>(hip_stream);
  return SMPC_OK;
}

int smpc_set_profile(smpc_ctx* c, int enable)
{
  if (!c) return SMPC_ERR_INVALID;
  if (enable) c->cfg.flags |= SMPC_FLAG_PROFILE;
  else c->cfg.flags &= ~static_cast<uint32_t>(SMPC_FLAG_PROFILE);
  return SMPC_OK;
}
}  // extern "C"
