// smpc_lane_pass.inc — the lane-per-rollout scoring pass (see smpc_lane.hip, which includes this file
// three times).  LANE_PASS_KERNEL names the kernel, LANE_PASS_POW says whether its per-rollout epilogue
// scores with general cost powers, LANE_PASS_NH whether the motion model is non-holonomic:
//   smpc_pass_lane      every cost_power == 1 (the lean association of smpc_pass MODE 0)
//   smpc_pass_lane_pow  a cost_power other than 1 among the five critics (a legal tuning value:
//                       obstacles_critic.cpp:173-177, path_align_critic.cpp:135).  The power applies to a
//                       critic's per-rollout TOTAL, so time loop, lookup pipeline, furthest-point scan,
//                       softmax and transpose-reduce are the same text; only the epilogue differs: five
//                       small double-precision powers per rollout, where the loop's registers are dead.
//   smpc_pass_lane_nh   DiffDrive and Ackermann on a plain cruise tick: vy is zero at every step of
//                       every rollout, so this kernel has no vy — no vy noise load (two tensors of the
//                       three per step), no vy control, no vy term in the rotation or the gamma sum,
//                       nothing parked for it and one transpose-reduce less per group.  Everything
//                       else is the same text; every line it leaves out is marked "NH".  It reads
//                       neither p.svy nor the vy row of the tick block nor the vy noise tensor.
// Three kernels from one text, not a tenth template argument and not a shared inlined body: the
// power-1 instances keep their names (profiles and tests know them) and compile to the code they
// compiled to before (a body shared through a __forceinline__ function kept their register counts
// but not their instructions).
template <bool FULL, bool OBST, bool MANY, int NCH, bool RR, bool GA = false, bool QUADS = FULL, int TC = 0, bool DEP = false>
__global__ void __launch_bounds__(RR ? LANE_BLOCK_RR : LANE_BLOCK, 1)
LANE_PASS_KERNEL(const SmpcDev p0, const SmpcLds L, const SmpcDev* __restrict__ many)
{
  constexpr bool POW = LANE_PASS_POW;
  constexpr bool NH = LANE_PASS_NH;
  static_assert(!NH || (OBST && !MANY && !RR && !GA && !DEP && !POW && NCH == 1 && QUADS),
                "no vy stream: the plain ObstaclesCritic rows of whole quads only");
  static_assert(RR || NCH == 1, "parked controls: one chunk of 64 steps");
  static_assert(!POW || (!MANY && !RR && !DEP), "cost powers: the single-context parking form of the five critics");
  // QUADS: T is a multiple of four, so every step of every executed quad is live and the time
  // loop carries no per-step "t < T" branch.  The reference's default horizon is 56: with the
  // branch around every step the scheduler cannot overlap neighbouring steps, and 56 steps took
  // LONGER than 64 (67.7 against 59.1 us at 262 144 rollouts).
  static_assert(!FULL || QUADS, "T == 64 is a multiple of four");
  // TC: a horizon below 64 known at compile time (the reference's default, 56): trip counts,
  // bound checks and the control sequence's offsets fold as they do for T == 64
  static_assert(TC == 0 || (!FULL && QUADS && !RR && TC < 64 && (TC & 3) == 0), "compile-time horizon: whole quads below 64");
  // DEP: the cruise tick of the reference's deployed critic list (robot_bringup/config/
  // nav2_params.yaml:222: Constraint, Cost, Goal, GoalAngle, PathAlign, PathFollow, PathAngle,
  // PreferForward, Twirling).  Away from the goal and on the path, Goal, GoalAngle and PathAngle
  // are gated off (the host checks), Cost takes ObstaclesCritic's place in the lookup pipeline —
  // same costAtPose, same collision rule, its per-cost term in the table's second field — and
  // Constraint and Twirling are two more additive per-step terms (power 1, in float like the
  // other sums of this pass).  Instances of their own: the cruise instances of the five pay nothing.
  static_assert(!DEP || (OBST && !RR && !GA), "deployed-list instances: parking form");
  const SmpcDev& p = MANY ? many[blockIdx.y] : p0;
  // (this pass reads its tick block from device memory only: it fetches u with scalar loads quad
  // by quad, group after group, and reads of the kernarg segment are not cached the way plain
  // device memory is — u inside the kernel arguments cost the 2 097 152-rollout pass 7 %)
  const SmpcTickPtrs tk{p.u, p.px, p.py, p.pyaw, p.D, p.pf_idx, p.pvalid, p.pa_active, p.pang_active, p.pal_active};
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  uint8_t* s_map = smem;
  const SmpcLut* s_lut = reinterpret_cast<const SmpcLut*>(smem + L.off_lut);
  float* s_px = reinterpret_cast<float*>(smem + L.off_px);
  float* s_py = reinterpret_cast<float*>(smem + L.off_py);
  // cumulative path distances D[0..P-1) at s_D[0..], with a sentinel on either side of the
  // part PathAlign searches: s_D[-1] = -3e38 and s_D[S] = +3e38 (S = furthest point)
  float* s_D = reinterpret_cast<float*>(smem + L.off_D) + 1;
  // PathAlign's view of the path: {x, y, segment valid ? 1 : 0, 0} per point, one 16-byte read
  f32x4* s_pts4 = reinterpret_cast<f32x4*>(smem + L.off_pts4);
  // sum_t u[ctrl][t]^2 of this launch's control sequence, ctrl = vx, vy, wz (the gamma terms):
  // the 16 bytes in front of the per-wave scratch (smpc_prepare.cpp lane_lds)
  float* s_su2 = reinterpret_cast<float*>(smem + L.off_scr) - 4;
  // kPrune: the furthest-point section sits at the END of the group body, with the prune test in
  // front of its scan (smpc_lane_furthest.inc).  Per instance, like kWindow: there the parked
  // registers are dead and the plain instances keep 256 VGPRs without scratch; moved in the
  // grouped deployed-list instances it costs 8 bytes of scratch, in the re-read one 30 VGPRs.
  constexpr bool kPrune = !GA && !DEP && !MANY && !RR && !POW;
  // the host's table for it: {k0, n, block-shared bound, 0} and n entries of eight floats (smpc_dev.h)
  float* s_prune = reinterpret_cast<float*>(smem + L.off_prune);

  constexpr int BLK = RR ? LANE_BLOCK_RR : LANE_BLOCK;   // the largest block; small batches launch half of it
  const int blk = blockDim.x;
  const int tid = threadIdx.x;
  const int lane = tid & (WAVE - 1);
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nwave = blockDim.x >> 6;
  // developer aid: shader-clock stamps of wave 0 (null pointer: one uniform branch each)
  auto stamp = [&](int k) {
    if (__builtin_expect(p.timeline != nullptr, 0) && tid == 0)
      p.timeline[blockIdx.x * 8 + k] = __builtin_amdgcn_s_memtime();
  };
  stamp(0);
  // per wave: [64][65] parked wz, [64] softmax weights; the head is re-used by the block combine
  float* park = reinterpret_cast<float*>(smem + L.off_scr) + (size_t)wave * L.scr_stride;
  float* s_w = park + 64 * LANE_PARK_STRIDE;

  // ---- stage costmap window, LUT and path into LDS -------------------------
  // Every global load of the staging goes out before the first LDS store (one memory round trip
  // for window, table and path together); what exceeds one pass of the block is looped over
  // afterwards.
  {
    const int ww = OBST ? p.win_w : 0, wh = OBST ? p.win_h : 0;
    const bool vec = OBST && ((ww & 3) == 0) && ((p.W & 3u) == 0) && ((p.win_x0 & 3) == 0);
    const int w4 = OBST ? (ww >> 2) : 1, n4 = vec ? w4 * wh : 0;   // (1: the map-less variants never divide)
    auto word = [&](int i) -> uint32_t {
      const int ry = i / w4, rx = i - ry * w4;
      return reinterpret_cast<const uint32_t*>(p.map + (size_t)(p.win_y0 + ry) * p.W + p.win_x0)[rx];
    };
    constexpr int kAhead = 96 * 96 / 4 / BLK + 1;   // a 96 x 96 window in one sweep of the block
    uint32_t tmp[kAhead];
#pragma unroll
    for (int k = 0; k < kAhead; ++k) {
      const int i = tid + k * blk;
      tmp[k] = i < n4 ? word(i) : 0u;
    }
    const SmpcLut lut_e = (OBST && tid < 256) ? p.lut[tid] : SmpcLut{0.f, 0.f};
    const bool pt_on = (uint32_t)tid < p.P, seg_on = (uint32_t)tid + 1 < p.P;
    const float g_px = pt_on ? tk.px[tid] : 0.f, g_py = pt_on ? tk.py[tid] : 0.f;
    const float g_D = seg_on ? tk.D[tid] : 0.f;
    const bool g_valid = seg_on && tk.pvalid[tid] != 0;
    const float g_prune = (kPrune && tid < (int)SMPC_PRUNE_FLOATS) ? p.prune[tid] : 0.f;

    if (OBST) {
#pragma unroll
      for (int k = 0; k < kAhead; ++k) {
        const int i = tid + k * blk;
        if (i < n4) reinterpret_cast<uint32_t*>(s_map)[i] = tmp[k];
      }
      for (int i = tid + kAhead * blk; i < n4; i += blk)
        reinterpret_cast<uint32_t*>(s_map)[i] = word(i);
      if (!vec) {
        for (int i = tid; i < ww * wh; i += blockDim.x) {
          const int ry = i / ww, rx = i - ry * ww;
          s_map[i] = p.map[(size_t)(p.win_y0 + ry) * p.W + p.win_x0 + rx];
        }
      }
      if (tid < 256) const_cast<SmpcLut*>(s_lut)[tid] = lut_e;
      if (tid == 0) const_cast<SmpcLut*>(s_lut)[256] = SmpcLut{0.f, 0.f};   // the all-zero entry
      // one byte behind the window answers "off the map" (NO_INFORMATION,
      // obstacles_critic.cpp:209-212); behind it one byte per lane of every wave for costs
      // fetched from the global map (cells outside the window)
      if (tid == 0) s_map[ww * wh] = 255;
    }
    for (uint32_t i = p.P + tid; i < ((p.P + 3u) & ~3u); i += blockDim.x) s_px[i] = s_py[i] = 1.0e18f;
    if (kPrune && tid < (int)SMPC_PRUNE_FLOATS) s_prune[tid] = g_prune;
    if (pt_on) {
      s_px[tid] = g_px;
      s_py[tid] = g_py;
      if (seg_on) s_D[tid] = g_D;
      s_pts4[tid] = f32x4{g_px, g_py, g_valid ? 1.0f : 0.f, 0.f};
    }
    if (tid < WAVE) {   // (one wave: lane t squares u[.][t], then a butterfly)
      float a = 0.f, b = 0.f, c = 0.f;
      const uint32_t Tn = FULL ? 64u * NCH : (TC ? (uint32_t)TC : p.T);
      for (uint32_t t = (uint32_t)tid; t < Tn; t += WAVE) {
        const float ux = tk.u[t], uy = NH ? 0.f : tk.u[Tn + t], uz = tk.u[2 * Tn + t];
        a = fmaf(ux, ux, a);
        b = fmaf(uy, uy, b);
        c = fmaf(uz, uz, c);
      }
      for (int o = 32; o > 0; o >>= 1) {
        a += __shfl_xor(a, o, WAVE);
        b += __shfl_xor(b, o, WAVE);
        c += __shfl_xor(c, o, WAVE);
      }
      if (tid == 0) {
        s_su2[0] = a;
        s_su2[1] = b;
        s_su2[2] = c;
      }
    }
    for (uint32_t i = tid + blk; i < p.P; i += blk) {   // paths beyond one point per thread
      const float qx = tk.px[i], qy = tk.py[i];
      const bool seg = i + 1 < p.P;
      s_px[i] = qx;
      s_py[i] = qy;
      if (seg) s_D[i] = tk.D[i];
      s_pts4[i] = f32x4{qx, qy, (seg && tk.pvalid[i]) ? 1.0f : 0.f, 0.f};
    }
  }
  __syncthreads();
  stamp(1);

  // ---- constants (wave-uniform: scalar registers) -------------------------------
  // u and the path are inputs of the launch: read them through the constant address space,
  // so that uniform loads stay scalar loads although the kernel also stores to global memory
  const cfloat_p cu = (cfloat_p)(uintptr_t)p.u;
  const uint32_t T = FULL ? 64u * NCH : (TC ? (uint32_t)TC : p.T), B = p.B;
  // group-major noise through buffer loads: per QUAD of steps one scalar offset per tensor
  // (tensor * noise_bytes + quad * 1024), the lane's own offset (its group's start + lane * 16) is the
  // vector offset and the same for the whole group — a lane's four steps of a quad are 16 contiguous
  // bytes (smpc_dev.h), one 16-byte load
  // (the host lays the three tensors out back to back: ONE descriptor, four scalar
  // registers instead of twelve — the loop is short of them — and the tensor is part of the
  // scalar offset)
  const uint32_t T4 = SMPC_GM_STEPS(T);
  const uint32_t noise_bytes = (uint32_t)SMPC_GM_ELEMS(B, T) * 4u;   // one tensor, group-major (smpc_dev.h)
  const __amdgpu_buffer_rsrc_t rn = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.tvx), 0, 3u * noise_bytes, 0x00020000);
  const float dt = p.dt, yaw0 = p.yaw0;
  const double x0 = p.x0, y0 = p.y0;
  uint32_t S = 0;
  if (p.flags & SD_NEED_FURTHEST) {
    S = p.d_furthest ? smpc_furthest_index(*p.d_furthest) : p.furthest_hint;
    if (S >= p.P) S = p.P ? p.P - 1 : 0;
  }
  // the sentinels of s_D (every wave writes the same two values before its first read: no
  // second barrier, and S need not be known while the block stages)
  if (lane == 0) {
    s_D[-1] = -3.0e38f;
    s_D[S] = 3.0e38f;
  }
  const bool pa_on = (p.flags & SD_PATH_ALIGN) && p.P > 0 && tk.pa_active[S] && S > 0;
  float pf_x = 0.f, pf_y = 0.f;
  if ((p.flags & SD_PATH_FOLLOW) && p.P > 0) {
    const uint32_t idx = tk.pf_idx[S];
    pf_x = tk.px[idx];
    pf_y = tk.py[idx];
  }
  const uint32_t bs_iters = S > 1 ? 32u - (uint32_t)__builtin_clz(S - 1) : 0u;
  float pa_inv_spacing = 0.f;
  if (pa_on && S > 1 && tk.D[S - 1] > 0.f) pa_inv_spacing = (float)(S - 1) / tk.D[S - 1];
  const bool want_local_furthest = (p.flags & SD_NEED_FURTHEST) && (p.flags & SD_LOCAL_FURTHEST);
  const bool con_on = DEP && (p.flags & SD_CONSTRAINT) != 0, tw_on = DEP && (p.flags & SD_TWIRLING) != 0;
  const float k_con = p.dt * p.con_weight, k_tw = p.tw_weight / (float)(FULL ? 64 * NCH : (TC ? TC : (int)p.T));
  // CostCritic in ObstaclesCritic's place (DEP): the table's second field holds its per-cost term
  const bool cost_mode = DEP && (p.flags & SD_COST) != 0;
  // GoalAngleCritic is a near-goal term: it is compiled into instances of their own (GA), which the
  // launcher picks when the tick's flags carry it — as a run-time branch of the cruise
  // instances it cost them 1.3-3 % (413 against 401 us on the 2 097 152-rollout pass)
  constexpr bool ga_on = GA;
  const uint32_t nquad = (T + 3u) >> 2;

  // ---- per-wave running softmax state; U[ctrl][t] lives in lane t ----------------
  float m_run = 3.0e38f, s_run = 0.f;
  float Ux[NCH], Uy[NCH], Uz[NCH];   // chunk h: steps [64 h, 64 h + 64)
#pragma unroll
  for (int h = 0; h < NCH; ++h) Ux[h] = Uy[h] = Uz[h] = 0.f;
  float F_local = 0.f;   // furthest point of this wave's rollouts, index + fraction (smpc_dev.h)
  bool furthest_pending = false;   // kPrune: the first group's endpoints wait in LDS (smpc_lane_furthest.inc)
  uint32_t n_noncoll = 0;

  const uint32_t ngroups = (B + WAVE - 1) / WAVE;
  const uint32_t gw = blockIdx.x * nwave + wave;
  const uint32_t nW = gridDim.x * nwave;

  // One group of 64 rollouts.  SAFE = false is the fast instance: sin/cos without the
  // huge-argument branch (a divergent branch in the middle of the step would keep the
  // scheduler from overlapping the costmap lookups with it); it only notes whether some
  // |yaw| left the range of the fast reduction, commits nothing in that case and returns
  // true, and the group is redone by the SAFE instance.
  using T_ = std::true_type;
  using F_ = std::false_type;
  auto group_body = [&](auto safe_c, const uint32_t grp) -> bool {
    constexpr bool SAFE = decltype(safe_c)::value;
    const uint32_t b = grp * WAVE + lane;
    const bool live = b < B;
    const uint32_t bl = live ? b : B - 1;        // tail lanes shadow the last rollout
    // parked noised controls of this group, c[ctrl][t] = P<ctrl><t / 32>[t % 32]: register
    // tuples written through the scalar GPR index (s_set_gpr_idx) inside the rolled time loop
    // and read with static indices by the transpose-reduce, which works in place
    // (vx and vy: 128 registers).  wz is parked in this wave's LDS slot instead, [t][65]:
    // the write is lane-contiguous, the transposed read (lane t, rollout b) conflict-free.
    // Element 8 i + q' of PX<h> holds c_vx[t = 32 h + 4 q' + i]: the eight parks of a quad
    // index with the same scalar q' (the constant 8 i folds into the base register) and can
    // share one s_set_gpr_idx_on/off pair.
    f32x32 PX0, PX1, PY0, PY1;
    if constexpr (NH) {   // (nothing is parked for vy: PY0 and PY1 are never touched)
      if (!FULL) PX0 = PX1 = (f32x32)(0.f);
    } else if (!FULL && !RR) PX0 = PX1 = PY0 = PY1 = (f32x32)(0.f);

    // ================= rollout + per-step critics, lane = rollout =====================
    float cpx = p.svx, cpy = NH ? 0.f : p.svy, cpz = p.swz;   // v[:,0] = measured speed, v[:,t] = c[:,t-1]
    float acc_yaw = 0.f, ax = 0.f, ay = 0.f;
    float cs_prev = p.cos0, sn_prev = p.sin0;
    float x = 0.f, y = 0.f;
    float crit = 0.f, rep = 0.f;
    float yaw_max = 0.f;   // largest |yaw| seen (fast instance: range check of the sin/cos reduction)
    float alive = 1.0f;   // 1 until the rollout's first collision, then 0 (a float mask: fma(1, a, c) == c + a)
    // The costmap lookup is two dependent LDS reads (the cell's byte, then the byte's table
    // entry) feeding an in-order accumulation.  It runs as a pipeline two steps deep whose three
    // stages all sit at the END of a step, behind one wait: accumulate the entry of step t - 2,
    // issue the table read for the byte of step t - 1, issue the byte read of step t's own cell —
    // every read has had a whole step to land, so the wait is free.  The reads are plain C++
    // loads carried from one step to the next in cell_q and e_q: the compiler's scheduler places
    // them and its waitcnt pass their waits.  (Pinning their place in the step with
    // inline-assembly reads and a hand-placed wait, which the waitcnt pass does not see, was
    // tried and rejected: neutral on its own, DESIGN.md 4.2.)  Primed with the all-zero table
    // entry 256; drained after the loop.
    uint32_t cell_q = 256u;
    f32x2 e_q = {0.f, 0.f};   // {crit, rep} of SmpcLut
    auto lookup_wait = [&]() {};   // (empty on purpose: without it and its calls some instances' instructions reorder)
    auto lookup_accumulate = [&]() {
      // steps after the first collision are never visited in the reference (masked)
      alive = e_q.x < 0.f ? 0.f : alive;   // inCollision
      crit = fmaf(alive, e_q.x, crit);
      rep = fmaf(alive, e_q.y, rep);
    };
    auto lookup_issue_entry = [&]() {          // e_q <- s_lut[cell_q]
      const SmpcLut e = s_lut[cell_q];
      e_q = f32x2{e.crit, e.rep};
    };
    auto lookup_issue_byte = [&](uint32_t idx) {cell_q = s_map[idx];};   // cell_q <- s_map[idx]
    float pfw = 0.f, gx = 0.f, gy = 0.f, gz = 0.f;
    float ga_sum = 0.f;   // GoalAngleCritic: sum over the steps of |shortest angular distance to the goal's yaw|
    float ext = 0.f;      // DEP: ConstraintCritic + TwirlingCritic, weights and 1/T folded in
    // PathAlign running state (path_align_critic.cpp:92-133)
    // (trajectory point 0 is the same for every rollout: host-computed, same arithmetic)
    float traj_dist = 0.f, pa_sum = 0.f, pa_num = 0.f, sx_prev = p.x00f, sy_prev = p.y00f;
    uint32_t path_pt = 0;

    // loop constants of the cell index, in scalar registers.  (A scalar operand halves the issue
    // rate of the instruction that reads it, tools/ubench; held in vector registers instead they
    // push the parking form into scratch, 514.5 against 380.0 us at 2 097 152 x 64: DESIGN.md 4.2.)
    // kCellVgpr: the two addends of the cell index in vector registers all the same, in the instances
    // that have the room since the noise arrives in quads (a lane offset per step and tensor is gone):
    // the fused multiply-add reads one scalar (k_rinv) and needs no v_mov_b32 for a second one, two
    // instructions less per step.  Per instance, like kPrune: the plain rows of a horizon known at
    // compile time and their twins without vy, which keep ScratchSize 0 with it; not tried elsewhere.
    constexpr bool kCellVgpr = OBST && QUADS && (FULL || TC != 0) && !GA && !DEP && !MANY && !RR && !POW;
    const float k_rinv = p.rinvf, k_cx = kCellVgpr ? in_vgpr(p.cxf) : p.cxf, k_cy = kCellVgpr ? in_vgpr(p.cyf) : p.cyf;
    const float k_edge = 0.5f - p.cell_eps_w;
    // kAddAtTop: the quad's twelve noised controls are formed at its top — the same additions,
    // earlier — so that the noise tuples die at once, and the next quad's loads go out later in the
    // quad, in front of step kFetchAt (run_quad).  Per instance: three rows of T = 64 spill 8-20 bytes
    // to scratch with both the current and the coming tuples live across the whole quad.  The grouped
    // deployed-list row fetches behind the quad's first step, PathAlign's sample step, where the
    // registers are scarcest; the two GoalAngle rows (36 and 20 bytes that way, 36 and 12 a step later)
    // in front of the last step, where the per-step refill held as many registers as this form does.
    constexpr bool kAddAtTop = FULL && !RR && (GA || (MANY && DEP));
    constexpr int kFetchAt = GA ? 3 : 1;
    // one time step for the 64 rollouts of this wave; t, ux, uy, uz are wave-uniform
    // sample_slot: this step is a multiple of four (known at compile time in the unrolled quad)
    auto do_step = [&](const uint32_t t, const bool sample_slot, const float ux, const float uy, const float uz,
                       const float n0, const float n1, const float n2, float& cvx, float& cvy,
                       float& cwz) __attribute__((always_inline)) {
      // NoiseGenerator::setNoisedControls (noise_generator.cpp:65-74)
      if constexpr (!kAddAtTop) {
        cvx = ux + n0;
        if constexpr (!NH) cvy = uy + n1;
        cwz = uz + n2;
      }
      const float vx = cpx, vy = cpy, wz = cpz;
      cpx = cvx;
      if constexpr (!NH) cpy = cvy;
      cpz = cwz;
      // integrateStateVelocities (optimizer.cpp:313-343): sequential float cumsums
      acc_yaw = acc_yaw + wz * dt;
      const float yaw = acc_yaw + yaw0;
      // (NH: vy is +-0 in the other kernels too, and a -+ (+-0) == a but for the sign of a zero,
      // which the cumulative sums below, starting at +0, do not keep)
      const float dxr = NH ? vx * cs_prev : vx * cs_prev - vy * sn_prev;
      const float dyr = NH ? vx * sn_prev : vx * sn_prev + vy * cs_prev;
      ax = ax + dxr * dt;
      ay = ay + dyr * dt;
      if constexpr (DEP) {
        // ConstraintCritic (constraint_critic.cpp:41-75; holonomic and differential models: the
        // host keeps Ackermann off these instances): how far the signed speed leaves
        // [min_vel, max_vel], times dt and the weight
        if (con_on) {
          const float sp = fast_sqrt(vx * vx + vy * vy);
          const float vt = vx > 0.f ? sp : -sp;
          const float e = fmaxf(vt - p.con_max_vel, 0.f) + fmaxf(p.con_min_vel - vt, 0.f);
          ext = fmaf(e, k_con, ext);
        }
        // TwirlingCritic (twirling_critic.cpp:30-42): mean |wz| times the weight
        if (tw_on) ext = fmaf(fabsf(wz), k_tw, ext);
      }
      if (ga_on) {
        // GoalAngleCritic (goal_angle_critic.cpp:36-50), near-goal ticks only (a uniform branch):
        // |normalize_angles(goal yaw - yaw)|.  The reference normalises in double; here the
        // float difference (the reference's own) is reduced by 2 pi in two fused multiply-adds
        // — the remainder is within 2e-7 of the double one, the mean of 64 of them moves the
        // rollout's cost by ~1e-7 relative.
        const float a = p.ga_goal_yaw - yaw;
        const float kf = fmaf(a, 0.15915494309189535f, 12582912.0f);
        const float k = kf - 12582912.0f;
        float r = fmaf(-k, 6.2831854820251465f, a);
        r = fmaf(-k, -1.7484555e-07f, r);
        ga_sum += fabsf(r);
      }
      // The trajectory point itself, x = (float)(x0 + (double)ax) as the reference narrows it
      // (optimizer.cpp:331-342), is formed only where its VALUE is consumed: at PathAlign's
      // sample steps, at the endpoint and on the exact path of the cell index below.  The
      // three double-precision instructions per axis run at half the rate of the plain float
      // ones (tools/ubench: 4 against 2 SIMD cycles per wave64 instruction).

      // ObstaclesCritic lookup (obstacles_critic.cpp:139-171).  Fast cell index first: the
      // window-relative quotient from the accumulated displacement in ONE fused multiply-add,
      // q = ax / res + (x0 - window corner) / res.  Its distance to the quotient the reference
      // truncates — ((double)x - origin) / res with x ROUNDED to float first — is bounded on the
      // host (cell_eps_w: that rounding of x, the float images of the two constants, the fma's
      // own rounding).  Lanes within that bound of a cell edge, outside the window or off the
      // map get their LDS byte index from the exact path (the reference's own double arithmetic
      // on the rounded x); then ONE pair of dependent LDS reads serves every lane and overlaps
      // the sin/cos below.
      uint32_t idx = 0;
      if (OBST) {
        const float qx = fmaf(ax, k_rinv, k_cx), qy = fmaf(ay, k_rinv, k_cy);
        const float rx = __builtin_amdgcn_fractf(qx), ry = __builtin_amdgcn_fractf(qy);
        const int lx = cvt_floor_i32(qx), ly = cvt_floor_i32(qy);
        // guard band as ONE compare: both fractions at least eps away from a cell edge <=>
        // max(|rx - 1/2|, |ry - 1/2|) <= 1/2 - eps (a NaN fails it; the two extra float
        // roundings, < 1e-7, sit inside the factor 2 the host puts on eps).
        const float edge = fmaxf(fabsf(rx - 0.5f), fabsf(ry - 0.5f));
        const bool fast = (edge <= k_edge) &
                          ((uint32_t)lx < (uint32_t)p.win_w) & ((uint32_t)ly < (uint32_t)p.win_h);
        // window cells fit 24 bits: v_mad_u32_u24 instead of a 64-bit multiply-add
        idx = __umul24((uint32_t)ly, (uint32_t)p.win_w) + (uint32_t)lx;   // (meaningless if !fast)
        if (__builtin_expect(__builtin_amdgcn_ballot_w64(!fast) != 0, 0)) {
          if (!fast)
            idx = cell_byte_exact(p, s_map, (float)(x0 + (double)ax), (float)(y0 + (double)ay),
                                  (uint32_t)(wave * WAVE + lane));
        }
      }

      // cos_[t+1] = cos(yaw[t]); the last step's is never used
      if (SAFE) {
        smpc_sincos(yaw, sn_prev, cs_prev);
      } else {
        yaw_max = fmaxf(yaw_max, fabsf(yaw));
        smpc_sincos_fast(yaw, sn_prev, cs_prev);
      }
      // PreferForwardCritic (prefer_forward_critic.cpp:42-46): sum_t max(-vx, 0) dt, here as
      // -dt sum_t min(vx, 0) — the factor once per rollout instead of once per step; minimum and
      // sum in one statement (add_min_zero: the bare v_min_f32, no canonicalising v_max in front)
      pfw = add_min_zero(pfw, vx);
      // updateControlSequence gamma terms (optimizer.cpp:365-380): sum_t u (c - u), here
      // as sum_t u c - sum_t u^2: one fused multiply-add per control here, the constant
      // (s_su2, formed once per launch) subtracted once per rollout.  Half the instructions of
      // u (c - u); the running sums reach T |u| |c| instead of staying near zero, which is ~1e-6
      // absolute on a cost after the gamma / sigma^2 scaling (costs are compared at 2e-4).
      // (c - u is the noise up to the rounding of c = u + n, |c - u - n| <= ulp(c) / 2: a few 1e-8
      // on terms that gamma / sigma^2 scales to ~1e-7 of a cost.  The noise itself as the factor,
      // sum_t u n, is not used: the noise registers' longer life breaks the four-step prefetch,
      // +35 % at 2 M rollouts.)
      gx = fmaf(ux, cvx, gx);
      gz = fmaf(uz, cwz, gz);
      if constexpr (!NH) gy = fmaf(uy, cvy, gy);

      // PathAlignCritic sample (uniform in t): trajectory points step, 2 step, ...
      // (trajectory_point_step is 4 here, the reference's default — the host sends any other
      // value to the wave-per-rollout pass — so the sample steps are the first of every quad
      // but the very first: no per-step bookkeeping, no branch in the other three steps)
      if (sample_slot && pa_on && t != 0) {
        x = (float)(x0 + (double)ax);
        y = (float)(y0 + (double)ay);
        const float ddx = x - sx_prev, ddy = y - sy_prev;
        traj_dist += fast_sqrt(ddx * ddx + ddy * ddy);
        sx_prev = x;
        sy_prev = y;
        // utils::findClosestPathPt(D, traj_dist, path_pt) (tools/utils.hpp:665-675):
        // std::lower_bound over D[0..S) guessed from the mean spacing, confirmed against
        // D[g-1], D[g], D[g+1]; binary search only if some lane is unconfirmed
        const float dist = traj_dist;
        uint32_t gi = (uint32_t)(dist * pa_inv_spacing);
        gi = gi < S ? gi : S - 1;
        const float da = s_D[(int)gi - 1];     // the sentinels stand in at either end
        const float db = s_D[gi];
        const float dc = s_D[gi + 1];
        // D is non-decreasing, so (da < dist) >= (db < dist) >= (dc < dist): the lower bound
        // is g or g + 1 exactly when the first holds and the last does not
        const bool c0 = da < dist, c1 = db < dist, c2 = dc < dist;
        uint32_t lo = gi + (c1 ? 1u : 0u);
        float dl = c1 ? db : da, dh = c1 ? dc : db;
        if (__builtin_expect(__builtin_amdgcn_ballot_w64(!c0 || c2) != 0, 0)) {
          uint32_t base = 0, nn = S;
          for (uint32_t it = 0; it < bs_iters; ++it) {
            const uint32_t half = nn >> 1;
            base = (s_D[base + half - 1 + (half == 0)] < dist && half) ? base + half : base;
            nn -= half;
          }
          const float d_base = s_D[base];
          lo = base + (d_base < dist ? 1u : 0u);
          dl = lo > 0 ? s_D[lo - 1] : 0.f;
          dh = lo < S ? s_D[lo] : 0.f;
        }
        // lower_bound restricted to [path_pt, S) is the global one, since path_pt <= lo
        uint32_t pt;
        if (lo == path_pt) pt = 0;                 // iter == begin + init
        else if (lo >= S) pt = S - 1;              // end(): defined as size-1 (SURVEY H1)
        else pt = (dist - dl < dh - dist) ? lo - 1 : lo;
        path_pt = pt;
        const f32x4 q = s_pts4[pt];
        const float ex = q[0] - x, ey = q[1] - y;
        const float d = fast_sqrt(ex * ex + ey * ey);
        pa_num += q[2];                  // segment valid ? 1 : 0 (path_align_critic.cpp:119-127)
        pa_sum = fmaf(q[2], d, pa_sum);
      }
      if (OBST) {   // the lookup pipeline's three stages (see above)
        lookup_wait();
        lookup_accumulate();       // entry of step t - 2
        lookup_issue_entry();      // byte of step t - 1
        lookup_issue_byte(idx);    // this step's cell
      }
    };

    // noise: a quad of steps is a uniform base + this lane's offset; one quad in flight.
    // The control sequence of the next four steps is fetched (scalar loads) a quad ahead too.
    // noise, group-major: quad q of this wave's 64 rollouts is 1 KB behind quad q - 1
    const uint32_t loff = (bl >> 6) * (T4 * 256u) + (bl & 63u) * 16u;   // SMPC_GM_INDEX(bl, 0, T) in bytes, 32 bits: the descriptor spans < 4 GB
    constexpr uint32_t quad_bytes = 1024u;
    auto ldq = [&](uint32_t tensor, uint32_t q) -> f32x4 {
      // (the instances with a run-time trip count prefetch unconditionally — see run_quad — so their
      // last quad's prefetch is clamped to the last quad; T = 64 or TC: never out of range)
      const uint32_t qc = (FULL || TC || q < nquad) ? q : nquad - 1;
      return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rn, loff, tensor * noise_bytes + qc * quad_bytes, 0));
    };
    auto ldu = [&](uint32_t ctrl, uint32_t t) -> float {return cu[ctrl * T + ((FULL || t < T) ? t : T - 1)];};
    f32x4 nq0, nq1, nq2;   // the quad's four steps of vx, vy, wz noise (NH: nq1 is never written or read)
    float uq[12];          // (NH: the slots 3 i + 1 are never written or read — eight live values)
    nq0 = ldq(0, 0);
    if constexpr (!NH) nq1 = ldq(1, 0);
    nq2 = ldq(2, 0);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        if constexpr (NH) {
          if (k == 1) continue;
        }
        uq[3 * i + k] = ldu(k, i);
      }
    }
    uint64_t clk = __builtin_amdgcn_s_memtime();
    // four steps; the quad returns their noised controls in cq[3 i + ctrl] for the caller to park
    // (parking step by step inside the quad was tried: the parked tuples fall out of registers)
    // swap_c: this quad looks at the clock and sets the wave's priority
    // hi_c: steps [32, 64); not read (the caller parks), kept because without it the instances'
    // scalar register assignment changes
    auto run_quad = [&](auto hi_c, auto swap_c, const uint32_t q, float (&cq)[12]) __attribute__((always_inline)) {
      constexpr bool SWAP = decltype(swap_c)::value;
      // The two waves of a SIMD do not share it evenly by themselves: the older one wins every
      // tie and finishes its groups ~25 % sooner (41 us against 51 us for two groups), then the
      // younger one runs alone.  Swapping their priorities every 2^15 shader clocks — by the clock,
      // read a quad earlier: the same for both whatever their progress, in anti-phase between
      // waves w and w + 4 — lets both finish together at 47 us (measured: tools/lane_timeline.py;
      // shorter periods share less evenly, 2^12: 45 / 48 us).
      // Once per loop iteration where the loops are pairs of quads (kPairLoops: two quads or
      // ~6 000 clocks of the period's 32 768), and as "low, then high if the bit says so": one
      // branch over one instruction where the if / else compiled to two branches and a mask.
      if constexpr (SWAP) {
        __builtin_amdgcn_s_setprio(0);
        if (((uint32_t)(clk >> 15) + (uint32_t)(wave >> 2)) & 1u) __builtin_amdgcn_s_setprio(1);
        clk = __builtin_amdgcn_s_memtime();
      }
      float uc[12];
#pragma unroll
      for (int j = 0; j < 12; ++j) {
        if constexpr (NH) {
          if (j % 3 == 1) continue;
        }
        uc[j] = uq[j];
      }
      // The next quad's controls and noise are fetched a quad ahead.  Where the trip count is a
      // run-time value (T < 64) the fetch is unconditional — the last quad re-reads the last
      // row: behind a run-time "is there a next quad" the waitcnt pass gives up the prefetch
      // depth (every wait became vmcnt(0), and 56 steps took longer than 64).
      constexpr bool kAlwaysAhead = !FULL && TC == 0;
      if (kAlwaysAhead || q + 1 < nquad) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int k = 0; k < 3; ++k) {
            if constexpr (NH) {
              if (k == 1) continue;
            }
            uq[3 * i + k] = ldu(k, 4 * (q + 1) + i);
          }
      }
      // This quad's noise is copied, and the next quad's three 16-byte loads (NH: two) go out at
      // once: one scalar offset per tensor and quad, the lane's offset is the group's.
      const f32x4 nc0 = nq0, nc1 = NH ? (f32x4)(0.f) : nq1, nc2 = nq2;
      if constexpr (kAddAtTop) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          cq[3 * i] = uc[3 * i] + nc0[i];
          cq[3 * i + 1] = uc[3 * i + 1] + nc1[i];
          cq[3 * i + 2] = uc[3 * i + 2] + nc2[i];
        }
      }
      auto fetch = [&]() __attribute__((always_inline)) {
        if (kAlwaysAhead || q + 1 < nquad) {
          nq0 = ldq(0, q + 1);
          if constexpr (!NH) nq1 = ldq(1, q + 1);
          nq2 = ldq(2, q + 1);
        }
      };
      if constexpr (!kAddAtTop) fetch();
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const uint32_t t = 4 * q + i;
        if constexpr (kAddAtTop) {
          // ... and the loads go out later in the quad (pinned: left alone the scheduler moves them back up)
          if (i == kFetchAt) {
            __builtin_amdgcn_sched_barrier(0);
            fetch();
            __builtin_amdgcn_sched_barrier(0);
          }
        }
        const float n0 = nc0[i], n1 = nc1[i], n2 = nc2[i];
        if constexpr (!kAddAtTop) cq[3 * i] = cq[3 * i + 1] = cq[3 * i + 2] = 0.f;
        if (QUADS || t < T)
          do_step(t, i == 0, uc[3 * i], NH ? 0.f : uc[3 * i + 1], uc[3 * i + 2], n0, n1, n2, cq[3 * i], cq[3 * i + 1],
                  cq[3 * i + 2]);
      }
    };
    // (the horizons known at compile time only: with this form of the loops the whole-quads
    // instance spills 12 bytes to scratch and the ragged GoalAngle instance with cost powers 4.7 KB)
    constexpr bool kPairLoops = FULL || TC != 0;
    // Park the quad cq came from: steps [0, 32) into the <..>0 tuples, [32, 64) into <..>1, element
    // t % 32; the re-read form parks nothing (the controls are formed again from the noise once the
    // weights are known).
    // (a macro, not a lambda: behind lambdas the main instance spills 640 bytes to scratch)
#define LANE_PARK_QUAD(HI, Q) \
      if constexpr (!RR) { \
        _Pragma("unroll") for (int i = 0; i < 4; ++i) { \
          if constexpr (HI) { \
            PX1[8 * i + ((Q) - 8)] = cq[3 * i]; \
            if constexpr (!NH) PY1[8 * i + ((Q) - 8)] = cq[3 * i + 1]; \
          } else { \
            PX0[8 * i + (Q)] = cq[3 * i]; \
            if constexpr (!NH) PY0[8 * i + (Q)] = cq[3 * i + 1]; \
          } \
          park[(4 * (Q) + i) * LANE_PARK_STRIDE + lane] = cq[3 * i + 2]; \
        } \
      }
    if constexpr (kPairLoops) {
    // Two quads per loop iteration, by hand, the odd one behind its loop: the first quad of an
    // iteration swaps the priority, the second does not.
    // (macros, not lambdas: see LANE_PARK_QUAD)
#define LANE_QUAD(HI, SWAP, Q) \
    { \
      float cq[12]; \
      run_quad(std::bool_constant<HI>{}, std::bool_constant<SWAP>{}, (Q), cq); \
      LANE_PARK_QUAD(HI, Q) \
    }
#define LANE_QUADS(HI, Q0, QE)   /* quads [Q0, QE) */ \
    { \
      uint32_t q = (Q0); \
      const uint32_t qe = (QE); \
      for (; q + 1 < qe; q += 2) { \
        LANE_QUAD(HI, true, q) \
        LANE_QUAD(HI, false, q + 1) \
      } \
      if (q < qe) LANE_QUAD(HI, true, q) \
    }
    if constexpr (RR) {
      LANE_QUADS(false, 0u, nquad)
    } else {
      LANE_QUADS(false, 0u, nquad < 8u ? nquad : 8u)
      LANE_QUADS(true, 8u, nquad)
    }
#undef LANE_QUADS
#undef LANE_QUAD
    } else if constexpr (RR) {
      // nothing is parked: the controls are formed again from the noise once the weights are known
#pragma unroll 2
      for (uint32_t q = 0; q < nquad; ++q) {
        float cq[12];
        run_quad(F_{}, T_{}, q, cq);
      }
    } else {
      const uint32_t qh = nquad < 8u ? nquad : 8u;
      if constexpr (QUADS && !FULL && TC == 0) {
        auto quad_lo = [&](const uint32_t q) {
          float cq[12];
          run_quad(F_{}, T_{}, q, cq);
          LANE_PARK_QUAD(false, q)
        };
        auto quad_hi = [&](const uint32_t q) {
          float cq[12];
          run_quad(T_{}, T_{}, q, cq);
          LANE_PARK_QUAD(true, q)
        };
        // two quads per iteration by hand: with a run-time trip count "#pragma unroll 2" is not
        // honoured here, and one quad per iteration leaves the scheduler nothing to overlap
        // the next quad's loads and lookups with (699 VALU per 4 steps in a loop of its own)
        uint32_t q = 0;
        for (; q + 1 < qh; q += 2) {
          quad_lo(q);
          quad_lo(q + 1);
        }
        if (q < qh) quad_lo(q);
        q = 8;
        for (; q + 1 < nquad; q += 2) {
          quad_hi(q);
          quad_hi(q + 1);
        }
        if (q < nquad) quad_hi(q);
      } else {
        // (the T = 64 instances: these two loops verbatim — moving their bodies into lambdas cost
        // the main instance 896 bytes of scratch)
#pragma unroll 2
        for (uint32_t q = 0; q < qh; ++q) {
          float cq[12];
          run_quad(F_{}, T_{}, q, cq);
          LANE_PARK_QUAD(false, q)
        }
#pragma unroll 2
        for (uint32_t q = 8; q < nquad; ++q) {
          float cq[12];
          run_quad(T_{}, T_{}, q, cq);
          LANE_PARK_QUAD(true, q)
        }
      }
    }
#undef LANE_PARK_QUAD
    if (OBST) {   // drain the lookup pipeline: the entries of the last two steps
      lookup_wait();
      lookup_accumulate();
      lookup_issue_entry();
      lookup_wait();
      lookup_accumulate();
    }
    // (a NaN yaw is sticky in the cumulative sum: the last one shows it)
    if (!SAFE && __builtin_expect(__any(!(yaw_max < 65536.0f) || !(fabsf(acc_yaw) < 65536.0f)), 0)) return true;

    // the endpoint (trajectory point T - 1), as the reference narrows it
    x = (float)(x0 + (double)ax);
    y = (float)(y0 + (double)ay);

    // ================= per-rollout epilogue, lane = rollout ==============================
    if constexpr (!kPrune) {
#define LANE_FURTHEST_PRUNE false
#include "smpc_lane_furthest.inc"
#undef LANE_FURTHEST_PRUNE
    }
    float cost = (p.flags & (SD_ACCUMULATE | SD_COST_SEED)) ? p.costs_prev[bl] : 0.f;
    if constexpr (POW) {
      // costs with general cost powers: every critic's per-rollout total goes through
      // data.costs += pow(total * weight, power) on its own, with the arithmetic of smpc_pass
      // MODE 2 for what happens once per rollout (true divisions, the double square root) and in
      // the reference's critic order (Obstacles, PathAlign, PathFollow, GoalAngle, PreferForward;
      // then the control-cost terms).  The per-step sums are the lean loop's.
      if (OBST) {
        const bool collided = alive == 0.f;
        const float raw = collided ? p.obs_collision_cost : crit;
        const float v = (p.obs_critical_w * raw) + (p.obs_repulsion_w * rep / (float)T);
        cost = add_cost_pow(cost, (double)v, p.obs_power);
        n_noncoll += (uint32_t)__popcll(__ballot(live && !collided));
      }
      if (pa_on) {
        const float c_pa = pa_num > 0.f ? pa_sum / pa_num : 0.f;
        cost = add_cost_pow(cost, (double)(c_pa * p.pa_weight), p.pa_power);
      }
      // (the uniform factors become doubles HERE, behind in_vgpr: converted once in front of the
      // group loop they would hold register pairs across the time loop, which has none to spare)
      if (p.flags & SD_PATH_FOLLOW) {
        const double ddx = (double)(x - pf_x), ddy = (double)(y - pf_y);
        cost = add_cost_pow(cost, (double)in_vgpr(p.pf_weight) * sqrt_unscaled(ddx * ddx + ddy * ddy), p.pf_power);
      }
      if (ga_on) {
        // (a horizon known at compile time stays a literal: T = 64 divides by a multiplication)
        const double Td = (FULL || TC) ? (double)T : (double)in_vgpr((float)T);
        cost = add_cost_pow(cost, (double)ga_sum / Td * (double)in_vgpr(p.ga_weight), p.ga_power);
      }
      if (p.flags & SD_PREFER_FORWARD) cost = add_cost_pow(cost, (double)((pfw * -dt) * p.pfw_weight), p.pfw_power);
      cost += p.g_vx * (gx - s_su2[0]);
      cost += p.g_wz * (gz - s_su2[2]);
      cost += p.g_vy * (gy - s_su2[1]);
    } else {
      // costs (every cost_power == 1): the lean association of smpc_pass MODE 0
      float lin = 0.f, uni = 0.f;
      if (OBST) {
        const bool collided = alive == 0.f;
        if (cost_mode) {
          // cost_critic.cpp:157-166: collision_cost for a colliding rollout, else the sum of the
          // per-cost terms, times weight / 254 / T
          const float k = p.cost_w254 / (float)T;
          lin = collided ? 0.f : k * rep;
          uni = collided ? k * p.cost_collision_cost : 0.f;
        } else {
          lin = (collided ? 0.f : p.obs_critical_w * crit) + p.obs_rep_over_T * rep;
          uni = collided ? p.obs_critical_w * p.obs_collision_cost : 0.f;
        }
        n_noncoll += (uint32_t)__popcll(__ballot(live && !collided));
      }
      if constexpr (DEP) lin += ext;
      if (p.flags & SD_PATH_FOLLOW) {
        const float fdx = x - pf_x, fdy = y - pf_y;
        uni += p.pf_weight * fast_sqrt(fdx * fdx + fdy * fdy);
      }
      if (p.flags & SD_PREFER_FORWARD) lin += (pfw * -dt) * p.pfw_weight;
      if (ga_on) uni += (ga_sum / (float)T) * p.ga_weight;
      lin += p.g_vx * (gx - s_su2[0]);
      lin += p.g_wz * (gz - s_su2[2]);
      if constexpr (!NH) lin += p.g_vy * (gy - s_su2[1]);
      cost += uni + lin;
      if (pa_on) {
        const float c_pa = pa_num > 0.f ? pa_sum * fast_rcp(pa_num) : 0.f;
        cost += c_pa * p.pa_weight;
      }
    }
    if (live) p.costs[b] = cost;

    // ---- softmax of the group (optimizer.cpp:382-391 as an online sum) --------------
    float cmin = live ? cost : 3.0e38f;
    for (int o = 32; o > 0; o >>= 1) cmin = fminf(cmin, __shfl_xor(cmin, o, WAVE));
    const float m_new = fminf(m_run, cmin);
    const float f = __builtin_amdgcn_exp2f(p.k2 * (m_run - m_new));
    const float w = live ? __builtin_amdgcn_exp2f(p.k2 * (cost - m_new)) : 0.f;
    float wsum = w;
    for (int o = 32; o > 0; o >>= 1) wsum += __shfl_xor(wsum, o, WAVE);
    s_run = fmaf(s_run, f, wsum);
    m_run = m_new;

    // ================= U[t] += sum_b w_b c[b][t]: transpose-reduce in registers ==========
    const LaneW lw = lane_weights(w, lane);
    if constexpr (RR) {
      // the group's noise again (it was read within the last tens of microseconds: served on
      // die), 64 steps of one control at a time in 16 loads of a quad each, and c = u + n with the
      // rounding of the step
#pragma unroll
      for (int h = 0; h < NCH; ++h) {
#pragma unroll
        for (int ctrl = 0; ctrl < 3; ++ctrl) {
          // all 16 loads go out before the first use (left alone the scheduler pairs every load
          // with its adds and waits for each in turn: 48 memory round trips per group)
          float V[64];
#pragma unroll
          for (int j = 0; j < 16; ++j) {
            const f32x4 v = ldq(ctrl, 16u * h + j);
#pragma unroll
            for (int e = 0; e < 4; ++e) V[4 * j + e] = v[e];
          }
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int t = 0; t < 64; ++t) {
            const uint32_t tt = 64u * h + t;
            const float c = ldu(ctrl, tt) + V[t];
            V[t] = (FULL || tt < T) ? c : 0.f;
          }
          const float r = lane_reduce64(V, lw, lane);
          if (ctrl == 0) Ux[h] = fmaf(Ux[h], f, r);
          else if (ctrl == 1) Uy[h] = fmaf(Uy[h], f, r);
          else Uz[h] = fmaf(Uz[h], f, r);
        }
      }
    } else {
      {
        float V[64];
#pragma unroll
        for (int t = 0; t < 32; ++t) {
          V[t] = PX0[8 * (t & 3) + (t >> 2)];
          V[32 + t] = PX1[8 * (t & 3) + (t >> 2)];
        }
        Ux[0] = fmaf(Ux[0], f, lane_reduce64(V, lw, lane));
        if constexpr (!NH) {   // (NH: Uy stays +0, what the weighted sum of zeros is)
#pragma unroll
          for (int t = 0; t < 32; ++t) {
            V[t] = PY0[8 * (t & 3) + (t >> 2)];
            V[32 + t] = PY1[8 * (t & 3) + (t >> 2)];
          }
          Uy[0] = fmaf(Uy[0], f, lane_reduce64(V, lw, lane));
        }
      }
      {
        // wz from the LDS slot: lane t walks its row of 64 rollouts
        s_w[lane] = w;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        const f32x4* row = reinterpret_cast<const f32x4*>(park + lane * LANE_PARK_STRIDE);
        float acc0 = 0.f, acc1 = 0.f;
#pragma unroll
        for (int bq = 0; bq < 16; bq += 2) {
          const f32x4 w0 = reinterpret_cast<const f32x4*>(s_w)[bq], c0 = row[bq];
          const f32x4 w1 = reinterpret_cast<const f32x4*>(s_w)[bq + 1], c1 = row[bq + 1];
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            acc0 = fmaf(w0[e], c0[e], acc0);
            acc1 = fmaf(w1[e], c1[e], acc1);
          }
        }
        Uz[0] = fmaf(Uz[0], f, acc0 + acc1);
        __builtin_amdgcn_wave_barrier();
      }
    }
    if constexpr (kPrune) {
#define LANE_FURTHEST_PRUNE true
#include "smpc_lane_furthest.inc"
#undef LANE_FURTHEST_PRUNE
    }
    return false;
  };

  stamp(2);
  int stamp_k = 3;
  for (uint32_t grp = gw; grp < ngroups; grp += nW) {
    if (__builtin_expect(group_body(F_{}, grp), 0)) group_body(T_{}, grp);
    if (stamp_k < 5) stamp(stamp_k++);
  }

  if (__builtin_expect(p.timeline != nullptr, 0) && lane == 0)
    p.timeline[8192 + blockIdx.x * 8 + wave] = __builtin_amdgcn_s_memtime();
  // ---- block combine -> one partial per block (same tuple as the wave-per-rollout pass)
  __syncthreads();
  stamp(5);
  const uint32_t TL = 4 + 3 * T;
  float* myp = reinterpret_cast<float*>(smem + L.off_scr) + (size_t)wave * L.scr_stride;
  if (lane == 0) {
    myp[0] = m_run;
    myp[1] = s_run;
    myp[2] = F_local;
    myp[3] = (float)n_noncoll;
  }
#pragma unroll
  for (int h = 0; h < NCH; ++h) {
    const uint32_t tt = 64u * h + (uint32_t)lane;
    if (tt < T) {
      myp[4 + tt] = Ux[h];
      myp[4 + T + tt] = Uy[h];
      myp[4 + 2 * T + tt] = Uz[h];
    }
  }
  __syncthreads();
  const float* allp = reinterpret_cast<const float*>(smem + L.off_scr);
  float bm = 3.0e38f;
  for (int w = 0; w < nwave; ++w) bm = fminf(bm, allp[(size_t)w * L.scr_stride]);
  float* outp = p.partials + (size_t)blockIdx.x * TL;
  for (uint32_t i = tid; i < TL; i += blockDim.x) {
    float acc = 0.f;
    if (i == 0) {
      acc = bm;
    } else if (i == 2) {
      for (int w = 0; w < nwave; ++w) acc = fmaxf(acc, allp[(size_t)w * L.scr_stride + 2]);
    } else if (i == 3) {
      for (int w = 0; w < nwave; ++w) acc += allp[(size_t)w * L.scr_stride + 3];
    } else {
      for (int w = 0; w < nwave; ++w) {
        const float mw = allp[(size_t)w * L.scr_stride];
        const float sc = __builtin_amdgcn_exp2f(p.k2 * (mw - bm));   // as the per-wave rescale above
        acc += sc * allp[(size_t)w * L.scr_stride + i];
      }
    }
    smpc_store_partial(outp + i, acc);
  }
  stamp(6);
  // Which tick block this launch read (SmpcDev::canary_echo): its number sits four floats in front
  // of u; block 0 leaves it behind the grid's partials for the reduction to hand to the host.
  // Unconditional wherever u is the tick block's own (the host knows when the word means nothing)
  // and through the two pointers the kernel holds anyway: a pointer or a flag of its own, live
  // across the time loop, cost the T = 64 instance 20 bytes of scratch.
  if (!(p.flags & SD_ACCUMULATE) && blockIdx.x == 0 && tid == 0) outp[SMPC_CANARY_SLOT(T)] = cu[-4];
  if constexpr (!MANY && !RR) {   // (the re-read form's grid is three blocks per CU: over SMPC_TAIL_MAX_GRID)
    if (p.tail) smpc_grid_tail<(RR ? LANE_BLOCK_RR : LANE_BLOCK) / 64>(p, smem);   // (the host: full-size blocks only)
  }
}
