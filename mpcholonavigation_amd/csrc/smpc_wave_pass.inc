// smpc_wave_pass.inc — the wave-per-rollout pass: ONE text, compiled under several kernel names
// (smpc_kernels.hip, smpc_wave_many.hip, smpc_wave_stats.hip and smpc_wave_stats_many.hip include it,
// as smpc_lane.hip does smpc_lane_pass.inc).
//   WAVE_PASS_KERNEL  names the kernel
//   WAVE_PASS_MANY    0: smpc_pass — one planning instance, parameter block and LDS carve-up in the
//                        kernel arguments
//                     1: smpc_pass_many — several planning instances in one launch
//                        (smpc_group_optimize): blockIdx.y picks the instance, whose parameter block
//                        and geometry (SmpcWaveGeom: its own carve-up and its own grid) come from device
//                        memory.  No tick block in the kernel arguments, no in-launch reduction
//                        (smpc_grid_tail waits for other blocks; this kernel never does, so a launch
//                        of more blocks than stay resident just runs in rounds).
// A second name instead of a fourth template argument: the instances of smpc_pass keep their names
// and, the text being the same, their registers, scratch and occupancy.
#if WAVE_PASS_STATS
//   WAVE_PASS_STATS   1: smpc_pass_stats<R, FULL> (smpc_wave_stats.hip, WAVE_PASS_MANY 0) — the general
//                        pass (MODE 2) of one planning instance that also KEEPS every critic's term:
//                        wherever add_cost_pow folds a term into the cost, and at the gamma add, one
//                        lane stores it to stats[row * stats_ld + rollout] (rows: SMPC_CRITIC_* of
//                        include/smpc.h).  Undefined or 0: not a line of this text changes.
//                        With WAVE_PASS_MANY 1: smpc_pass_stats_many<R, FULL> (smpc_wave_stats_many.hip,
//                        smpc_group_critic_breakdown) — blockIdx.y picks the member, whose rows and their
//                        leading dimension (SmpcStatsDst) come from device memory like its parameter block.
template <int R, bool FULL>
#else
template <int R, int MODE, bool FULL>
#endif
#if WAVE_PASS_MANY
__global__ void __launch_bounds__((R == 4 ? 512 : 1024), (R == 4 ? 2 : 4))
#if WAVE_PASS_STATS
WAVE_PASS_KERNEL(const SmpcDev* __restrict__ many, const SmpcWaveGeom* __restrict__ geom, const SmpcStatsDst* __restrict__ dst)
{
  constexpr int MODE = 2;
  static_assert(R == 1, "the grouped rows: T <= 64");
#else
WAVE_PASS_KERNEL(const SmpcDev* __restrict__ many, const SmpcWaveGeom* __restrict__ geom)
{
#if WAVE_PASS_MANY_FURTHEST
  // (smpc_wave_stats_many.hip: the furthest-point pre-pass of smpc_group_critic_breakdown)
  static_assert(R == 1 && MODE == 1, "the grouped pre-pass: T <= 64, furthest point only");
#else
  static_assert(R == 1 && (MODE == 0 || MODE == 3 || MODE == 4), "the grouped rows: T <= 64, the lean scoring modes");
#endif
#endif
  constexpr bool MANY = true;
  // Members differ in batch size, hence in the blocks they need: a block beyond its member's own
  // grid leaves before the first barrier, having written nothing (uniform over the block)
  if (blockIdx.x >= geom[blockIdx.y].grid) return;
  const SmpcDev& p = many[blockIdx.y];
  const SmpcLds& L = geom[blockIdx.y].lds;
#if WAVE_PASS_STATS
  float* __restrict__ const stats = dst[blockIdx.y].stats;
  const uint32_t stats_ld = dst[blockIdx.y].ld;
#endif
#define WAVE_PASS_GRID (geom[blockIdx.y].grid)
#else
#if WAVE_PASS_STATS
__global__ void __launch_bounds__((R == 4 ? 512 : 1024), (R == 4 ? 2 : 4))
WAVE_PASS_KERNEL(const SmpcDev p, const SmpcLds L, float* __restrict__ stats, const uint32_t stats_ld)
{
  constexpr int MODE = 2;
#else
__global__ void __launch_bounds__((R == 4 ? 512 : 1024), (R == 4 ? 2 : 4)) WAVE_PASS_KERNEL(const SmpcDev p, const SmpcLds L)
{
#endif
  constexpr bool MANY = false;
#define WAVE_PASS_GRID (gridDim.x)
#endif
  constexpr bool FURTHEST_ONLY = MODE == 1;
  constexpr bool GENERIC = MODE == 2;
  // MODE 0 is the lean kernel: the rarely used features (trajectory write-out, path
  // orientations) live only in MODE 2, so their pointers and parameters do not occupy scalar
  // registers in the hot loop; the near-goal GoalAngle term is scored by MODE 3 (power 1) or 2
  constexpr bool RARE = MODE == 1 || MODE == 2;
  constexpr bool EXTRA = MODE == 3 || MODE == 4;
  // MODE 4 is MODE 3 with the footprint check of ONE collision critic (consider_footprint): the
  // walk sits behind a wave-uniform branch in the lookup loop below
  constexpr bool FOOTPRINT = MODE == 4;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  uint8_t* s_map = smem;
  const SmpcLut* s_lut = reinterpret_cast<const SmpcLut*>(smem + L.off_lut);
  float* s_px = reinterpret_cast<float*>(smem + L.off_px);
  float* s_py = reinterpret_cast<float*>(smem + L.off_py);
  float* s_pyaw = reinterpret_cast<float*>(smem + L.off_pyaw);
  float* s_D = reinterpret_cast<float*>(smem + L.off_D);
  uint8_t* s_valid = smem + L.off_valid;

  const SmpcTickPtrs tk = smpc_tick_ptrs(p, !MANY);   // (a grouped context never has its tick block in the kernel arguments)
  const int tid = threadIdx.x;
  const int lane = tid & (WAVE - 1);
  // wave-uniform by construction: tell the compiler, so that the rollout index, the row
  // addresses and the loop control live on the scalar unit
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nwave = blockDim.x >> 6;
  float* scr = reinterpret_cast<float*>(smem + L.off_scr) + (size_t)wave * L.scr_stride;
  float* pts_x = scr + L.scr_pts;        // [64] PathAlign sample points, slot = g*SEG + s
  float* pts_y = pts_x + WAVE;
  float* pts_yaw = pts_y + WAVE;
  float* ring_x = scr + L.scr_ring;      // [64] parked rollout endpoints
  float* ring_y = ring_x + WAVE;
  float* cring = scr + L.scr_c;          // [group][3][T] parked noised controls
  // which tick block this launch reads (SmpcDev::canary_echo): its number sits four floats in
  // front of u; left behind the partials for the reduction to hand to the host
  if (!FURTHEST_ONLY && p.canary_echo && !(p.flags & SD_ACCUMULATE) && blockIdx.x == 0 && tid == 0)
    p.partials[SMPC_CANARY_SLOT(p.T)] = p.u[-4];

  // ---- stage costmap window, LUT and path into LDS -------------------------
  if (!FURTHEST_ONLY && (p.flags & (SD_OBSTACLES | SD_COST))) {
    const int ww = p.win_w, wh = p.win_h;
    const bool vec = ((ww & 3) == 0) && ((p.W & 3u) == 0) && ((p.win_x0 & 3) == 0);
    if (vec) {
      const int w4 = ww >> 2;
      for (int i = tid; i < w4 * wh; i += blockDim.x) {
        const int ry = i / w4, rx = i - ry * w4;
        const uint32_t* src = reinterpret_cast<const uint32_t*>(
          p.map + (size_t)(p.win_y0 + ry) * p.W + p.win_x0);
        reinterpret_cast<uint32_t*>(s_map)[ry * w4 + rx] = src[rx];
      }
    } else {
      for (int i = tid; i < ww * wh; i += blockDim.x) {
        const int ry = i / ww, rx = i - ry * ww;
        s_map[i] = p.map[(size_t)(p.win_y0 + ry) * p.W + p.win_x0 + rx];
      }
    }
    for (int i = tid; i < 256; i += blockDim.x)
      const_cast<SmpcLut*>(s_lut)[i] = p.lut[i];
  }
  for (uint32_t i = tid; i < p.P; i += blockDim.x) {
    s_px[i] = tk.px[i];
    s_py[i] = tk.py[i];
    if (!FURTHEST_ONLY) {
      s_pyaw[i] = tk.pyaw[i];
      if (i + 1 < p.P) {
        s_D[i] = tk.D[i];
        s_valid[i] = tk.pvalid[i];
      }
    }
  }
  __syncthreads();

  // ---- per-lane constants --------------------------------------------------
  const uint32_t T = p.T;
  const int t0 = lane * R;
#define STEP_OK(r) (FULL || (uint32_t)(t0 + (r)) < T)
  float uvx[R], uvy[R], uwz[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const bool a = STEP_OK(r);
    uvx[r] = a ? tk.u[t0 + r] : 0.f;
    uvy[r] = a ? tk.u[T + t0 + r] : 0.f;
    uwz[r] = a ? tk.u[2 * T + t0 + r] : 0.f;
  }
  const float dt = in_vgpr(p.dt);
  const float yaw0_v = in_vgpr(p.yaw0);
  const double x0_v = in_vgpr(p.x0), y0_v = in_vgpr(p.y0);
  const CellConsts cellk = {in_vgpr(p.oxf), in_vgpr(p.oyf), in_vgpr(p.rinvf), in_vgpr(p.cell_eps),
                            in_vgpr(1.0f - p.cell_eps)};
  const float obs_cw = in_vgpr(p.obs_critical_w), obs_rt = in_vgpr(p.obs_rep_over_T);
  const float pfw_w = in_vgpr(p.pfw_weight), pf_w = in_vgpr(p.pf_weight), pa_w = in_vgpr(p.pa_weight);
  const float k2_v = in_vgpr(p.k2);
  // MODE 4: centre cost from which a step looks at the footprint tables (never, without a switch)
  float fp_enter = 3.0e38f;
  if (FOOTPRINT && (p.flags & (SD_FP_OBSTACLES | SD_FP_COST))) fp_enter = p.fp_pic < 1.0f ? 0.f : fminf(p.fp_pic, 253.f);
  // {initial value in lane 0, 0 elsewhere}: addends of the fused shift (dpp_shr1_add)
  const float first_vx = lane == 0 ? p.svx : 0.f, first_vy = lane == 0 ? p.svy : 0.f;
  const float first_wz = lane == 0 ? p.swz : 0.f;
  const float first_cos = lane == 0 ? p.cos0 : 0.f, first_sin = lane == 0 ? p.sin0 : 0.f;
  float gux[R], guy[R], guz[R];   // gamma/std^2 * u (optimizer.cpp:367-379), MODE 0
#pragma unroll
  for (int r = 0; r < R; ++r) {
    gux[r] = p.g_vx * uvx[r];
    guy[r] = p.g_vy * uvy[r];
    guz[r] = p.g_wz * uwz[r];
  }

  uint32_t S = 0;       // batch-wide furthest point used for scoring
  bool pa_on = false;
  bool pal_on = false;  // PathAlignLegacyCritic (general pass only)
  float pf_x = 0.f, pf_y = 0.f;
  uint32_t bs_iters = 0;
  float pa_inv_spacing = 0.f;   // (S-1) / D[S-1]: mean inverse spacing of the plan
  if (!FURTHEST_ONLY) {
    if (p.flags & SD_NEED_FURTHEST) {
      S = p.d_furthest ? smpc_furthest_index(*p.d_furthest) : p.furthest_hint;
      if (S >= p.P) S = p.P ? p.P - 1 : 0;
    }
    pa_on = (p.flags & SD_PATH_ALIGN) && p.P > 0 && tk.pa_active[S] && S > 0;
    if (GENERIC) pal_on = (p.flags & SD_PATH_ALIGN_LEGACY) && p.P > 1 && tk.pal_active[S];
    if ((p.flags & SD_PATH_FOLLOW) && p.P > 0) {
      const uint32_t idx = tk.pf_idx[S];
      pf_x = s_px[idx];
      pf_y = s_py[idx];
    }
    bs_iters = S > 1 ? 32u - (uint32_t)__builtin_clz(S - 1) : 0u;  // ceil(log2 S)
    if (pa_on && S > 1 && s_D[S - 1] > 0.f) pa_inv_spacing = (float)(S - 1) / s_D[S - 1];
  }
  pf_x = in_vgpr(pf_x);
  pf_y = in_vgpr(pf_y);
  pa_inv_spacing = in_vgpr(pa_inv_spacing);
  const bool want_local_furthest =
    FURTHEST_ONLY || ((p.flags & SD_NEED_FURTHEST) && (p.flags & SD_LOCAL_FURTHEST));
  // group geometry: GROUP rollouts parked per flush, SEG lanes (sample slots) per rollout
  const uint32_t seg_shift = L.seg_shift, SEG = 1u << seg_shift, GROUP = L.group;
  const uint32_t K = p.nsamp;   // PathAlign samples: trajectory points step, 2 step, ..., K step
  // sample slot of each step this lane owns: t = s*step, s = 0..K  (-1: not a sample)
  int slot[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const uint32_t t = t0 + r;
    const uint32_t q = p.step ? t / p.step : 0u;
    slot[r] = ((pa_on || pal_on) && p.step && STEP_OK(r) && q * p.step == t && q <= K) ? (int)q : -1;
  }
  const uint32_t end_lane = (T - 1) / R, end_r = (T - 1) % R;

  // running softmax state of this wave (optimizer.cpp:382-391 as an online sum)
  float m_run = 3.0e38f, s_run = 0.f;
  float Ux[R], Uy[R], Uz[R];
#pragma unroll
  for (int r = 0; r < R; ++r) Ux[r] = Uy[r] = Uz[r] = 0.f;
  uint32_t S_local = 0, n_noncoll = 0;
  uint32_t n_ring = 0, n_pend = 0;
  float pend_cost = 0.f;        // lanes of segment g: cost so far of parked rollout g

  const uint32_t gw = blockIdx.x * nwave + wave;
  const uint32_t nW = WAVE_PASS_GRID * nwave;

  // flush of the parked group: PathAlign, costs, softmax, weighted controls
  auto flush = [&](uint32_t n, uint32_t b_last) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const uint32_t g = (uint32_t)lane >> seg_shift, s = (uint32_t)lane & (SEG - 1);
    const bool rowon = g < n;
    float cost = pend_cost;
    // ---- PathAlignCritic (path_align_critic.cpp:92-135), lane = (rollout g, sample s) ----
    if (pa_on) {
      const bool smp = rowon && s >= 1 && s <= K;
      const float Tx = pts_x[lane], Ty = pts_y[lane];
      const float Qx = wave_shr1(Tx, 0.f), Qy = wave_shr1(Ty, 0.f);   // previous sample point
      float chord = 0.f;
      if (smp) {
        const float ddx = Tx - Qx, ddy = Ty - Qy;
        chord = GENERIC ? sqrtf(ddx * ddx + ddy * ddy) : fast_sqrt(ddx * ddx + ddy * ddy);
      }
      const float dist = seg_scan_add(chord, seg_shift);
      // std::lower_bound over D[0..S).  Plans are close to uniformly spaced, so the
      // index is guessed from the mean spacing and confirmed against D[g-1], D[g],
      // D[g+1]; a wave with any unconfirmed lane runs the branch-free binary search.
      uint32_t gi = (uint32_t)(dist * pa_inv_spacing);
      gi = gi < S ? gi : S - 1;
      const float da = gi > 0 ? s_D[gi - 1] : -3.0e38f;
      const float db = s_D[gi];
      const float dc = gi + 1 < S ? s_D[gi + 1] : 3.0e38f;
      uint32_t lo;
      float dl, dh;   // D[lo-1], D[lo]
      const bool at_g = da < dist && !(db < dist);
      const bool at_g1 = db < dist && !(dc < dist);
      if (at_g) {
        lo = gi; dl = da; dh = db;
      } else {
        lo = gi + 1; dl = db; dh = dc;
      }
      if (__builtin_expect(__any(!(at_g || at_g1)), 0)) {
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
      uint32_t cand;
      if (lo >= S) {
        cand = S - 1;  // reference dereferences end(): defined as size-1 (SURVEY H1)
      } else if (lo == 0) {
        cand = 0;
      } else {
        cand = (dist - dl < dh - dist) ? lo - 1 : lo;
      }
      // findClosestPathPt's `iter == begin + init -> return 0` chains through path_pt:
      // path_pt_k = 0 where lo_k == path_pt_{k-1}.  With E_k = (lo_k == cand_{k-1} != 0 ...)
      // the chain F_k = E_k & ~F_{k-1} is "every other bit of each run of ones"; slot 0 of
      // a segment is never a sample, so runs do not cross rollouts.
      uint32_t cand_v = cand;
      asm volatile("" : "+v"(cand_v));   // DPP sources must sit in a VGPR
      const uint32_t cand_prev = dpp_u<0x138>(0u, cand_v);   // wave_shr:1
      unsigned long long E = __ballot(smp && lo == cand_prev && cand != 0u);
      uint32_t pt = cand;
      if (E) {
        unsigned long long F = E & ~(E << 1);
        unsigned long long M = E & (E << 1);
        F |= (F << 2) & M;
        M &= M << 2;
        F |= (F << 4) & M;
        M &= M << 4;
        F |= (F << 8) & M;
        M &= M << 8;
        F |= (F << 16) & M;
        M &= M << 16;
        F |= (F << 32) & M;
        if ((F >> lane) & 1ull) pt = 0;
      }
      const bool ok = smp && s_valid[pt];
      float d = 0.f;
      if (ok) {
        const float ddx = s_px[pt] - Tx, ddy = s_py[pt] - Ty;
        if (RARE && (p.flags & SD_USE_PATH_YAW)) {
          const double dd = (double)pts_yaw[lane] - (double)s_pyaw[pt];
          double a = fmod(fmod(dd, 2.0 * M_PI) + 2.0 * M_PI, 2.0 * M_PI);
          if (a > M_PI) a -= 2.0 * M_PI;
          const float dyaw = (float)a;
          d = sqrtf(ddx * ddx + ddy * ddy + dyaw * dyaw);
        } else {
          d = GENERIC ? sqrtf(ddx * ddx + ddy * ddy) : fast_sqrt(ddx * ddx + ddy * ddy);
        }
      }
      // per-rollout sum and count: last lane of the segment after a segmented scan
      const float dsum = seg_scan_add(d, seg_shift);
      const float summed = __shfl(dsum, lane | (int)(SEG - 1), WAVE);
      const unsigned long long okm = __ballot(ok) >> (g << seg_shift);
      const unsigned long long segm = SEG == 64 ? ~0ull : ((1ull << SEG) - 1ull);
      const float num = (float)__popcll(okm & segm);
      const float c_pa = num > 0.f ? (GENERIC ? summed / num : summed * fast_rcp(num)) : 0.f;
      if (GENERIC) cost = add_cost_pow(cost, (double)(c_pa * p.pa_weight), p.pa_power);
      else cost += c_pa * pa_w;
#if WAVE_PASS_STATS
      stats_put(stats, stats_ld, SMPC_CRITIC_PATH_ALIGN, b_last - (n - 1 - g) * nW, rowon && s == 0, (double)(c_pa * p.pa_weight), p.pa_power);
#endif
    }
    // ---- PathAlignLegacyCritic (path_align_legacy_critic.cpp:74-129), lane = (rollout g, sample s):
    // every trajectory point step, 2 step, ... against its nearest path point by brute force over
    // s' = 0 .. P - 3 (the loop runs to path_segments_count - 1 EXCLUSIVE, :101), first minimum
    // wins; the point counts unless it is point 0 or invalid (:119-121); the sum is divided by
    // floor(T / step), not by the count (:124)
    if (GENERIC && pal_on) {
      const bool smp = rowon && s >= 1 && s <= K;
      const float Tx = pts_x[lane], Ty = pts_y[lane];
      float min_dist_sq = 3.4028234663852886e38f;
      uint32_t min_s = 0;
      const uint32_t n_pts = p.P - 2u;      // (P >= 2: the host's gate)
      for (uint32_t q = 0; q < n_pts; ++q) {
        const float dx = s_px[q] - Tx, dy = s_py[q] - Ty;
        float dist_sq = dx * dx + dy * dy;
        if (p.flags & SD_PAL_USE_PATH_YAW) {
          // angles::shortest_angular_distance(P_yaw(s), T_yaw(t, p)) = normalize_angle(to - from)
          const double dd = (double)pts_yaw[lane] - (double)s_pyaw[q];
          double a = fmod(fmod(dd, 2.0 * M_PI) + 2.0 * M_PI, 2.0 * M_PI);
          if (a > M_PI) a -= 2.0 * M_PI;
          const float dyaw = (float)a;
          dist_sq = dx * dx + dy * dy + dyaw * dyaw;
        }
        if (dist_sq < min_dist_sq) {
          min_dist_sq = dist_sq;
          min_s = q;
        }
      }
      const bool ok = smp && min_s != 0u && s_valid[min_s];
      const float d = ok ? sqrtf(min_dist_sq) : 0.f;
      const float dsum = seg_scan_add(d, seg_shift);
      const float summed = __shfl(dsum, lane | (int)(SEG - 1), WAVE);
      const float c_pal = summed / p.pal_eval;
      cost = add_cost_pow(cost, (double)(c_pal * p.pal_weight), p.pal_power);
#if WAVE_PASS_STATS
      stats_put(stats, stats_ld, SMPC_CRITIC_PATH_ALIGN_LEGACY, b_last - (n - 1 - g) * nW, rowon && s == 0, (double)(c_pal * p.pal_weight), p.pal_power);
#endif
    }
    // costs_ [B]: one lane per parked rollout
    if (rowon && s == 0) p.costs[b_last - (n - 1 - g) * nW] = cost;

    // ---- softmax over the group (optimizer.cpp:382-391 as an online sum) ----------
    const float cmin = wave_min_f(rowon ? cost : 3.0e38f);
    const float m_new = fminf(m_run, cmin);
    // exp(-(c - m)/temperature) as one v_exp_f32: 2^(k2 (c - m)), k2 = -log2(e)/temperature
    const float f = __builtin_amdgcn_exp2f(k2_v * (m_run - m_new));   // rescale old sums (<= 1)
    const float w = rowon ? __builtin_amdgcn_exp2f(k2_v * (cost - m_new)) : 0.f;
    s_run = fmaf(s_run, f, wave_sum(s == 0 ? w : 0.f));
#pragma unroll
    for (int r = 0; r < R; ++r) {
      Ux[r] *= f;
      Uy[r] *= f;
      Uz[r] *= f;
    }
    for (uint32_t gg = 0; gg < n; ++gg) {
      const float wg = lane_bcast(w, (int)(gg << seg_shift));
      const float* cg = cring + (size_t)gg * 3 * T;
#pragma unroll
      for (int r = 0; r < R; ++r) {
        if (STEP_OK(r)) {
          Ux[r] = fmaf(wg, cg[t0 + r], Ux[r]);
          Uy[r] = fmaf(wg, cg[T + t0 + r], Uy[r]);
          Uz[r] = fmaf(wg, cg[2 * T + t0 + r], Uz[r]);
        }
      }
    }
    m_run = m_new;
    __builtin_amdgcn_wave_barrier();
  };

  // noise rows are prefetched one rollout ahead
  float n0[R], n1[R], n2[R];
  if (gw < p.B) {
    const size_t row = (size_t)gw * T;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const bool a = STEP_OK(r);
      n0[r] = a ? p.nvx[row + t0 + r] : 0.f;
      n1[r] = a ? p.nvy[row + t0 + r] : 0.f;
      n2[r] = a ? p.nwz[row + t0 + r] : 0.f;
    }
  }

  uint32_t b_prev = gw;
  for (uint32_t b = gw; b < p.B; b += nW) {
    b_prev = b;
    // ---- NoiseGenerator::setNoisedControls (noise_generator.cpp:65-74) -----
    const size_t row = (size_t)b * T;
    float cvx[R], cvy[R], cwz[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      cvx[r] = uvx[r] + n0[r];
      cvy[r] = uvy[r] + n1[r];
      cwz[r] = uwz[r] + n2[r];
    }
    if (b + nW < p.B) {
      const size_t nrow = (size_t)(b + nW) * T;
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const bool a = STEP_OK(r);
        n0[r] = a ? p.nvx[nrow + t0 + r] : 0.f;
        n1[r] = a ? p.nvy[nrow + t0 + r] : 0.f;
        n2[r] = a ? p.nwz[nrow + t0 + r] : 0.f;
      }
    }
    // ---- updateStateVelocities + predict: v[:,0]=speed, v[:,1:]=c[:,:-1] ---
    float vx[R], vy[R], wz[R];
    vx[0] = dpp_shr1_add(cvx[R - 1], first_vx);
    vy[0] = dpp_shr1_add(cvy[R - 1], first_vy);
    wz[0] = dpp_shr1_add(cwz[R - 1], first_wz);
#pragma unroll
    for (int r = 1; r < R; ++r) {
      vx[r] = cvx[r - 1];
      vy[r] = cvy[r - 1];
      wz[r] = cwz[r - 1];
    }
    if (!FULL) {
#pragma unroll
      for (int r = 0; r < R; ++r) {
        if (!STEP_OK(r)) vx[r] = vy[r] = wz[r] = 0.f;
      }
    }
    // ---- integrateStateVelocities (optimizer.cpp:313-343) -------------------
    float yaw[R];
    {
      float acc = wz[0] * dt;
      yaw[0] = acc;
#pragma unroll
      for (int r = 1; r < R; ++r) {
        acc += wz[r] * dt;
        yaw[r] = acc;
      }
      const float incl = wave_scan_add(acc);
      if (R == 1) {
        yaw[0] = incl + yaw0_v;   // one step per lane: the inclusive scan is the cumsum
      } else {
#pragma unroll
        for (int r = 0; r < R; ++r) yaw[r] = dpp_shr1_add(incl, yaw[r]) + yaw0_v;
      }
    }
    float x[R], y[R];
    {
      float sn[R], cs[R];
#pragma unroll
      for (int r = 0; r < R; ++r) smpc_sincos(yaw[r], sn[r], cs[r]);
      // cos_[t] = cos(yaw[t-1]), cos_[0] = cosf(initial_yaw)
      float c_prev = dpp_shr1_add(cs[R - 1], first_cos);
      float s_prev = dpp_shr1_add(sn[R - 1], first_sin);
      float ax = 0.f, ay = 0.f;
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const float dxr = vx[r] * c_prev - vy[r] * s_prev;
        const float dyr = vx[r] * s_prev + vy[r] * c_prev;
        ax = (r == 0) ? dxr * dt : ax + dxr * dt;
        ay = (r == 0) ? dyr * dt : ay + dyr * dt;
        x[r] = ax;
        y[r] = ay;
        c_prev = cs[r];
        s_prev = sn[r];
      }
      float sx = ax, sy = ay;
      wave_scan_add2(sx, sy);
      if (R == 1) {
        x[0] = (float)(x0_v + (double)sx);
        y[0] = (float)(y0_v + (double)sy);
      } else {
#pragma unroll
        for (int r = 0; r < R; ++r) {
          x[r] = (float)(x0_v + (double)dpp_shr1_add(sx, x[r]));
          y[r] = (float)(y0_v + (double)dpp_shr1_add(sy, y[r]));
        }
      }
    }
    if (!FURTHEST_ONLY && (RARE && (p.flags & SD_STORE_TRAJ))) {
#pragma unroll
      for (int r = 0; r < R; ++r) {
        if (STEP_OK(r)) {
          p.traj_x[row + t0 + r] = x[r];
          p.traj_y[row + t0 + r] = y[r];
          p.traj_yaw[row + t0 + r] = yaw[r];
        }
      }
    }
    // endpoint of the rollout (uniform): lane end_lane, step end_r
    float ex, ey;
    {
      float xe = x[0], ye = y[0];
#pragma unroll
      for (int r = 1; r < R; ++r) {
        if ((uint32_t)r == end_r) {
          xe = x[r];
          ye = y[r];
        }
      }
      ex = lane_bcast(xe, (int)end_lane);
      ey = lane_bcast(ye, (int)end_lane);
    }

    // ---- nearest path point of the endpoint (utils.hpp:292-319) -----------
    // Only max_b argmin_j matters and nothing in this rollout's cost depends on it, so
    // the endpoints are parked in a 64-slot LDS ring and resolved 64 rollouts at a time
    // with lane = rollout (sequential j loop: the reference's first-minimum order).
    if (want_local_furthest) {
      if (lane == 0) {
        ring_x[n_ring] = ex;
        ring_y[n_ring] = ey;
      }
      if (++n_ring == WAVE) {
        S_local = max(S_local, flush_endpoint_ring(ring_x, ring_y, WAVE, s_px, s_py, p.P, lane));
        n_ring = 0;
      }
    }
    if (FURTHEST_ONLY) continue;

    float cost = ((p.flags | (p.flags >> SD_COST_SEED_TO_ACCUMULATE)) & SD_ACCUMULATE) ? p.costs_prev[b] : 0.f;
    float lin = 0.f;    // MODE 0: per-lane sum of every additive per-step term
    float uni = 0.f;    // MODE 0: wave-uniform terms
    double lin_d = 0.0; // MODE 3: per-lane sum of the terms the reference forms in double

    // ---- ConstraintCritic (constraint_critic.cpp:41-75); MODE 2 only.  With the Ackermann
    //      model (con_acker_r >= 0) each step also pays min_turning_r - |vx|/|wz| (:54-69;
    //      float quotient, xt::maximum = select(a > b, a, b), so the 0/0 of a robot at rest
    //      adds nothing) ----
    if (RARE && (p.flags & SD_CONSTRAINT)) {
      double sa = 0.0;
#pragma unroll
      for (int r = 0; r < R; ++r) {
        if (STEP_OK(r)) {
          // xt::where(vx > 0.0, 1.0, -1.0) is a double tensor: double from there on
          const double sgn = vx[r] > 0.0f ? 1.0 : -1.0;
          const double vel_total = sgn * (double)sqrtf(vx[r] * vx[r] + vy[r] * vy[r]);
          const double out_max = fmax(vel_total - (double)p.con_max_vel, 0.0);
          const double out_min = fmax((double)p.con_min_vel - vel_total, 0.0);
          if (p.con_acker_r >= 0.f) {
            const double q = (double)(p.con_acker_r - fabsf(vx[r]) / fabsf(wz[r]));
            sa += (out_max + out_min + (q > 0.0 ? q : 0.0)) * (double)p.dt;
          } else {
            sa += (out_max + out_min) * (double)p.dt;
          }
        }
      }
      cost = add_cost_pow(cost, wave_sum_d(sa) * (double)p.con_weight, p.con_power);
#if WAVE_PASS_STATS
      stats_put(stats, stats_ld, SMPC_CRITIC_CONSTRAINT, b, lane == 0, wave_sum_d(sa) * (double)p.con_weight, p.con_power);
#endif
    }

    if (EXTRA && (p.flags & SD_CONSTRAINT)) {
      // the same per-step double arithmetic; with cost_power == 1 the critic's total is additive
      const double kw = (double)p.dt * (double)p.con_weight;
#pragma unroll
      for (int r = 0; r < R; ++r) {
        if (STEP_OK(r)) {
          const double sgn = vx[r] > 0.0f ? 1.0 : -1.0;
          const double vel_total = sgn * (double)sqrtf(vx[r] * vx[r] + vy[r] * vy[r]);
          double e = fmax(vel_total - (double)p.con_max_vel, 0.0) + fmax((double)p.con_min_vel - vel_total, 0.0);
          if (p.con_acker_r >= 0.f) {
            const double q = (double)(p.con_acker_r - fabsf(vx[r]) / fabsf(wz[r]));
            e += q > 0.0 ? q : 0.0;
          }
          lin_d += e * kw;
        }
      }
    }

    // ---- consider_footprint = true for either collision critic, general pass (MODE 4 carries
    //      its lean form in the lookup loop below) ----------
    // (obstacles_critic.cpp:139-171,203-224; cost_critic.cpp:128-166,175-201.)  The centre
    // cost is looked up as always; a step whose centre cost reaches the possibly-inscribed
    // cost gets the SE2 footprint cost.  Obstacles scores the footprint cost, Cost scores the
    // centre cost and only collision-checks with the footprint; each critic keeps its own
    // first collision.
    if (RARE && (p.flags & (SD_FP_OBSTACLES | SD_FP_COST))) {
      float crit = 0.f, rep = 0.f, crep = 0.f;
      int first_o = R, first_c = R;
#pragma unroll
      for (int r = 0; r < R; ++r) {
        if (!STEP_OK(r)) continue;
        const uint32_t c = (t0 + r == 0) ? p.cost_t0 : cost_at(p, cellk, s_map, x[r], y[r]);
        // off the map: NO_INFORMATION without a footprint check (costAtPose returns early)
        uint32_t mxe = 0, mye = 0;
        bool on = cell_index_exact((double)x[r], p.ox, p.res, p.W, mxe);
        on = cell_index_exact((double)y[r], p.oy, p.res, p.H, mye) && on;
        // Obstacles checks the footprint inside costAtPose (on-map centres only); Cost checks it
        // inside inCollision, also for an off-map centre (cost NO_INFORMATION)
        const bool cond = (float)c >= p.fp_pic || p.fp_pic < 1.0f;
        const bool want_o = (p.flags & SD_OBSTACLES) && (p.flags & SD_FP_OBSTACLES) && first_o == R &&
                            cond && on;
        const bool want_c = (p.flags & SD_COST) && (p.flags & SD_FP_COST) && first_c == R && cond &&
                            c >= 1u;
        float cf = (float)c;
        if (want_o || want_c) cf = footprint_cost_at_pose(p, s_map, x[r], y[r], yaw[r]);
        if ((p.flags & SD_OBSTACLES) && first_o == R) {
          const bool fpo = (p.flags & SD_FP_OBSTACLES) != 0;
          const uint32_t co = want_o ? (uint32_t)cf : c;
          const SmpcLut e = fpo ? p.lut_fp[(want_o ? 256u : 0u) + co] : s_lut[co];
          if (e.crit < 0.f) {
            first_o = r;
          } else {
            crit += e.crit;
            rep += e.rep;
          }
        }
        if ((p.flags & SD_COST) && first_c == R && c >= 1u) {
          const bool fpc = (p.flags & SD_FP_COST) != 0;
          const uint32_t cc = want_c ? (uint32_t)cf : c;
          const float marker = fpc ? p.lut_fp[cc].crit : s_lut[cc].crit;
          if (marker < 0.f) first_c = r;
          else crep += p.lut_cost[c];
        }
      }
      bool coll_o = false, coll_c = false;
      if (p.flags & SD_OBSTACLES) {
        const unsigned long long cm = __ballot(first_o < R);
        coll_o = cm != 0ull;
        if (coll_o) {
          const int lc = __ffsll((long long)cm) - 1;
          if (lane > lc) rep = 0.f;
        }
      }
      if (p.flags & SD_COST) {
        const unsigned long long cm = __ballot(first_c < R);
        coll_c = cm != 0ull;
        if (coll_c) {
          const int lc = __ffsll((long long)cm) - 1;
          if (lane > lc) crep = 0.f;
        }
      }
      // the critic that would stop the manager decides the batch-wide fail flag: Cost first
      if (!((p.flags & SD_COST) ? coll_c : coll_o)) n_noncoll++;
      if (p.flags & SD_COST) {
        const float repulsive = coll_c ? p.cost_collision_cost : wave_sum(crep);
        const float v = p.cost_w254 * repulsive / (float)T;
        cost = add_cost_pow(cost, (double)v, p.cost_power);
#if WAVE_PASS_STATS
        stats_put(stats, stats_ld, SMPC_CRITIC_COST, b, lane == 0, (double)v, p.cost_power);
#endif
      }
      if (p.flags & SD_OBSTACLES) {
        const float rep_sum = wave_sum(rep);
        const float raw = coll_o ? p.obs_collision_cost : wave_sum(crit);
        const float v = (p.obs_critical_w * raw) + (p.obs_repulsion_w * rep_sum / (float)T);
        cost = add_cost_pow(cost, (double)v, p.obs_power);
#if WAVE_PASS_STATS
        stats_put(stats, stats_ld, SMPC_CRITIC_OBSTACLES, b, lane == 0, (double)v, p.obs_power);
#endif
      }
    } else
    // ---- costmap lookups shared by CostCritic and ObstaclesCritic ----------------
    // (cost_critic.cpp:128-166, obstacles_critic.cpp:114-178: the same costAtPose and the same
    // inCollision switch in point mode, so one lookup and one first-collision search)
    if (p.flags & (SD_OBSTACLES | SD_COST)) {
      float crit = 0.f, rep = 0.f, crep = 0.f;
      int first_r = R;  // first colliding step inside this lane
#pragma unroll
      for (int r = 0; r < R; ++r) {
        if (STEP_OK(r) && first_r == R) {
          // point 0 is the same for every rollout (v[:,0] is the measured speed): its
          // cell was looked up once on the host with the same arithmetic
          const uint32_t c = (t0 + r == 0) ? p.cost_t0 : cost_at(p, cellk, s_map, x[r], y[r]);
          SmpcLut e = s_lut[c];
          // MODE 4, consider_footprint (obstacles_critic.cpp:139-171,203-224; cost_critic.cpp:
          // 128-166,175-201; the general pass's block above, one critic).  Below fp_enter the
          // point table and the footprint tables agree (they differ from cost 253 on), so only a
          // wave with a lane at or above it leaves MODE 3's stream; those lanes take their entry
          // from the footprint tables: [0..255] for a centre cost, [256..511] for a walked one.
          if (FOOTPRINT) {
            const bool enter = (float)c >= fp_enter;
            if (__builtin_expect(__any(enter), 0)) {
              if (enter) {
                bool want = (float)c >= p.fp_pic || p.fp_pic < 1.0f;
                if (p.flags & SD_COST) {
                  // inCollision checks the footprint for every scored step (c >= 1), also off the
                  // map; the centre cost stays the one scored, the walk gives the collision marker
                  want = want && c >= 1u;
                } else if (want && c == 255u) {
                  // costAtPose returns NO_INFORMATION for an off-map centre before any footprint
                  uint32_t mxe = 0, mye = 0;
                  want = cell_index_exact((double)x[r], p.ox, p.res, p.W, mxe);
                  want = cell_index_exact((double)y[r], p.oy, p.res, p.H, mye) && want;
                }
                uint32_t cc = c;
                if (want) cc = (uint32_t)footprint_cost_at_pose_inl(p, s_map, x[r], y[r], yaw[r]);
                e = p.lut_fp[((want && !(p.flags & SD_COST)) ? 256u : 0u) + cc];
              }
            }
          }
          if (e.crit < 0.f) {   // inCollision
            first_r = r;
          } else {
            crit += e.crit;
            rep += e.rep;
            if (RARE && (p.flags & SD_COST)) crep += p.lut_cost[c];
            // cost_critic.cpp:141-155 per 8-bit cost, as arithmetic (the table sits in global memory)
            if (EXTRA && (p.flags & SD_COST) && c >= 1u)
              crep += c >= 253u ? p.cost_critical : (p.cost_near_goal ? 0.f : (float)c);
          }
        }
      }
      const unsigned long long cm = __ballot(first_r < R);
      const bool collided = cm != 0ull;
      if (collided) {
        const int lc = __ffsll((long long)cm) - 1;
        if (lane > lc) rep = 0.f;  // steps after the first collision are never visited
      } else {
        n_noncoll++;
      }
      if (RARE && (p.flags & SD_COST)) {
        // repulsive_cost is a sum of 8-bit costs / critical_cost: exact in float in any order
        const float repulsive = collided ? p.cost_collision_cost : wave_sum(crep);
        const float v = p.cost_w254 * repulsive / (float)T;
        cost = add_cost_pow(cost, (double)v, p.cost_power);
#if WAVE_PASS_STATS
        stats_put(stats, stats_ld, SMPC_CRITIC_COST, b, lane == 0, (double)v, p.cost_power);
#endif
      }
      if (EXTRA && (p.flags & SD_COST)) {
        const float k = p.cost_w254 / (float)T;
        if (collided) uni += k * p.cost_collision_cost;
        else lin += k * crep;
      }
      if (p.flags & SD_OBSTACLES) {
        if (GENERIC) {
          const float rep_sum = wave_sum(rep);
          const float raw = collided ? p.obs_collision_cost : wave_sum(crit);
          const float v = (p.obs_critical_w * raw) + (p.obs_repulsion_w * rep_sum / (float)T);
          cost = add_cost_pow(cost, (double)v, p.obs_power);
#if WAVE_PASS_STATS
          stats_put(stats, stats_ld, SMPC_CRITIC_OBSTACLES, b, lane == 0, (double)v, p.obs_power);
#endif
        } else {
          // (added, not assigned: with CostCritic in the list too its terms are already in here)
          lin += (collided ? 0.f : obs_cw * crit) + obs_rt * rep;
          uni += collided ? p.obs_critical_w * p.obs_collision_cost : 0.f;
        }
      }
    }

    // ---- PathFollowCritic (path_follow_critic.cpp:56-70) ---------------------
    if (p.flags & SD_PATH_FOLLOW) {
      const float fdx = ex - pf_x, fdy = ey - pf_y;
      if (GENERIC) {
        const double ddx = (double)fdx, ddy = (double)fdy;
        const double dist = sqrt(ddx * ddx + ddy * ddy);
        cost = add_cost_pow(cost, (double)p.pf_weight * dist, p.pf_power);
#if WAVE_PASS_STATS
        stats_put(stats, stats_ld, SMPC_CRITIC_PATH_FOLLOW, b, lane == 0, (double)p.pf_weight * dist, p.pf_power);
#endif
      } else {
        uni += pf_w * fast_sqrt(fdx * fdx + fdy * fdy);
      }
    }

    // ---- GoalAngleCritic (goal_angle_critic.cpp:36-50) -----------------------
    if (RARE && (p.flags & SD_GOAL_ANGLE)) {
      double sa = 0.0;
#pragma unroll
      for (int r = 0; r < R; ++r) {
        if (STEP_OK(r)) sa += fabs(normalize_angle((double)(p.ga_goal_yaw - yaw[r])));
      }
      const double mean = wave_sum_d(sa) / (double)T;
      if (GENERIC) cost = add_cost_pow(cost, mean * (double)p.ga_weight, p.ga_power);
      else uni += (float)(mean * (double)p.ga_weight);
#if WAVE_PASS_STATS
      stats_put(stats, stats_ld, SMPC_CRITIC_GOAL_ANGLE, b, lane == 0, mean * (double)p.ga_weight, p.ga_power);
#endif
    }

    // ---- PreferForwardCritic (prefer_forward_critic.cpp:33-47) ---------------
    if (p.flags & SD_PREFER_FORWARD) {
      float sb = 0.f;
#pragma unroll
      for (int r = 0; r < R; ++r) sb += fmaxf(-vx[r], 0.f) * dt;
      if (GENERIC) cost = add_cost_pow(cost, (double)(wave_sum(sb) * p.pfw_weight), p.pfw_power);
      else lin += sb * pfw_w;
#if WAVE_PASS_STATS
      stats_put(stats, stats_ld, SMPC_CRITIC_PREFER_FORWARD, b, lane == 0, (double)(wave_sum(sb) * p.pfw_weight), p.pfw_power);
#endif
    }

    // ---- GoalCritic, PathAngleCritic, TwirlingCritic, VelocityDeadbandCritic: MODE 2 only ----
    if (RARE && (p.flags & SD_GOAL)) {
      // goal.position is double: distances in double, xt::mean in double (goal_critic.cpp:44-54)
      double sa = 0.0;
#pragma unroll
      for (int r = 0; r < R; ++r) {
        if (STEP_OK(r)) {
          const double ddx = (double)x[r] - p.goal_x, ddy = (double)y[r] - p.goal_y;
          sa += sqrt(ddx * ddx + ddy * ddy);
        }
      }
      cost = add_cost_pow(cost, wave_sum_d(sa) / (double)T * (double)p.goal_weight, p.goal_power);
#if WAVE_PASS_STATS
      stats_put(stats, stats_ld, SMPC_CRITIC_GOAL, b, lane == 0, wave_sum_d(sa) / (double)T * (double)p.goal_weight, p.goal_power);
#endif
    }
    if (RARE && (p.flags & SD_PATH_ANGLE) && tk.pang_active[S]) {
      // path_angle_critic.cpp:72-100: float atan2, then the double angle arithmetic of
      // utils::shortest_angular_distance / normalize_angles (tools/utils.hpp:258-284)
      const uint32_t idx = min(S + p.pang_offset, p.P - 1);
      const float tgx = s_px[idx], tgy = s_py[idx];
      double sa = 0.0;
#pragma unroll
      for (int r = 0; r < R; ++r) {
        if (STEP_OK(r)) {
          const float ybp = atan2f(tgy - y[r], tgx - x[r]);
          const double d = fabs(normalize_angle((double)(ybp - yaw[r])));
          if (p.pang_correct) {
            const double ybp_c = d < M_PI_2 ? (double)ybp : normalize_angle((double)ybp + M_PI);
            sa += fabs(normalize_angle(ybp_c - (double)yaw[r]));
          } else {
            sa += d;
          }
        }
      }
      cost = add_cost_pow(cost, wave_sum_d(sa) / (double)T * (double)p.pang_weight, p.pang_power);
#if WAVE_PASS_STATS
      stats_put(stats, stats_ld, SMPC_CRITIC_PATH_ANGLE, b, lane == 0, wave_sum_d(sa) / (double)T * (double)p.pang_weight, p.pang_power);
#endif
    }
    if (RARE && (p.flags & SD_TWIRLING)) {
      double sa = 0.0;   // twirling_critic.cpp:40-41
#pragma unroll
      for (int r = 0; r < R; ++r) {
        if (STEP_OK(r)) sa += (double)fabsf(wz[r]);
      }
      cost = add_cost_pow(cost, wave_sum_d(sa) / (double)T * (double)p.tw_weight, p.tw_power);
#if WAVE_PASS_STATS
      stats_put(stats, stats_ld, SMPC_CRITIC_TWIRLING, b, lane == 0, wave_sum_d(sa) / (double)T * (double)p.tw_weight, p.tw_power);
#endif
    }
    if (RARE && (p.flags & SD_DEADBAND)) {
      double sa = 0.0;   // velocity_deadband_critic.cpp:52-76 (::fabs(double): double arithmetic)
#pragma unroll
      for (int r = 0; r < R; ++r) {
        if (STEP_OK(r)) {
          sa += (fmax(p.db_vx - (double)fabsf(vx[r]), 0.0) + fmax(p.db_vy - (double)fabsf(vy[r]), 0.0) +
                 fmax(p.db_wz - (double)fabsf(wz[r]), 0.0)) * (double)p.dt;
        }
      }
      cost = add_cost_pow(cost, wave_sum_d(sa) * (double)p.db_weight, p.db_power);
#if WAVE_PASS_STATS
      stats_put(stats, stats_ld, SMPC_CRITIC_VELOCITY_DEADBAND, b, lane == 0, wave_sum_d(sa) * (double)p.db_weight, p.db_power);
#endif
    }

    if (EXTRA) {
      if (p.flags & SD_GOAL_ANGLE) {
        // GoalAngleCritic with cost_power 1 (goal_angle_critic.cpp:36-50): the mean over the steps
        // of |shortest_angular_distance(yaw, goal yaw)|, as a sum of per-step shares like the
        // other additive critics of this pass — a tick inside the goal thresholds stays on the
        // lean kernel instead of falling to the general one (3.7 ms against 0.43 ms for
        // 2 097 152 x 64 when it did, tools/near_goal_tick.py)
        const double kw = (double)p.ga_weight / (double)T;
#pragma unroll
        for (int r = 0; r < R; ++r) {
          if (STEP_OK(r)) lin_d += fabs(normalize_angle((double)(p.ga_goal_yaw - yaw[r]))) * kw;
        }
      }
      if (p.flags & SD_GOAL) {
        const double kw = (double)p.goal_weight / (double)T;
#pragma unroll
        for (int r = 0; r < R; ++r) {
          if (STEP_OK(r)) {
            const double ddx = (double)x[r] - p.goal_x, ddy = (double)y[r] - p.goal_y;
            lin_d += sqrt(ddx * ddx + ddy * ddy) * kw;
          }
        }
      }
      if ((p.flags & SD_PATH_ANGLE) && tk.pang_active[S]) {
        const uint32_t idx = min(S + p.pang_offset, p.P - 1);
        const float tgx = s_px[idx], tgy = s_py[idx];
        const double kw = (double)p.pang_weight / (double)T;
#pragma unroll
        for (int r = 0; r < R; ++r) {
          if (STEP_OK(r)) {
            const float ybp = atan2f(tgy - y[r], tgx - x[r]);
            const double d = fabs(normalize_angle((double)(ybp - yaw[r])));
            if (p.pang_correct) {
              const double ybp_c = d < M_PI_2 ? (double)ybp : normalize_angle((double)ybp + M_PI);
              lin_d += fabs(normalize_angle(ybp_c - (double)yaw[r])) * kw;
            } else {
              lin_d += d * kw;
            }
          }
        }
      }
      if (p.flags & SD_TWIRLING) {
        const double kw = (double)p.tw_weight / (double)T;
#pragma unroll
        for (int r = 0; r < R; ++r) {
          if (STEP_OK(r)) lin_d += (double)fabsf(wz[r]) * kw;
        }
      }
    }

    // ---- updateControlSequence gamma terms (optimizer.cpp:365-380) -----------
    if (GENERIC) {
      float gx = 0.f, gz = 0.f, gy = 0.f;
#pragma unroll
      for (int r = 0; r < R; ++r) {
        gx += uvx[r] * (cvx[r] - uvx[r]);
        gz += uwz[r] * (cwz[r] - uwz[r]);
        gy += uvy[r] * (cvy[r] - uvy[r]);
      }
      cost += p.g_vx * wave_sum(gx);
      cost += p.g_wz * wave_sum(gz);
      cost += p.g_vy * wave_sum(gy);
#if WAVE_PASS_STATS
      // (the control row keeps ONE float: the three gamma terms summed in the order they are added)
      stats_put(stats, stats_ld, SMPC_STATS_CONTROL, b, lane == 0,
                (double)(p.g_vx * wave_sum(gx) + p.g_wz * wave_sum(gz) + p.g_vy * wave_sum(gy)), 1u);
#endif
    } else {
#pragma unroll
      for (int r = 0; r < R; ++r) {
        lin = fmaf(gux[r], cvx[r] - uvx[r], lin);
        lin = fmaf(guz[r], cwz[r] - uwz[r], lin);
        lin = fmaf(guy[r], cvy[r] - uvy[r], lin);
      }
      if (EXTRA) cost += uni + (float)wave_sum_d(lin_d + (double)lin);
      else cost += uni + wave_sum(lin);
    }

    // ---- park the rollout -----------------------------------------------------
    {
      float* cg = cring + (size_t)n_pend * 3 * T;
#pragma unroll
      for (int r = 0; r < R; ++r) {
        if (STEP_OK(r)) {
          cg[t0 + r] = cvx[r];
          cg[T + t0 + r] = cvy[r];
          cg[2 * T + t0 + r] = cwz[r];
        }
        if (slot[r] >= 0) {
          const uint32_t q = (n_pend << seg_shift) + (uint32_t)slot[r];
          pts_x[q] = x[r];
          pts_y[q] = y[r];
          if (RARE && (p.flags & (SD_USE_PATH_YAW | SD_PAL_USE_PATH_YAW))) pts_yaw[q] = yaw[r];
        }
      }
      if (((uint32_t)lane >> seg_shift) == n_pend) pend_cost = cost;
      if (++n_pend == GROUP) {
        flush(n_pend, b);
        n_pend = 0;
      }
    }
  }
  if (!FURTHEST_ONLY && n_pend) flush(n_pend, b_prev);
  if (want_local_furthest && n_ring)
    S_local = max(S_local, flush_endpoint_ring(ring_x, ring_y, n_ring, s_px, s_py, p.P, lane));

  // ---- block combine -> one partial per block --------------------------------
  __syncthreads();
  if (FURTHEST_ONLY) {
    // S_local holds the bits of F >= 0: order preserving
    uint32_t* s_red = reinterpret_cast<uint32_t*>(smem + L.off_scr);
    if (lane == 0) s_red[wave] = S_local;
    __syncthreads();
    if (tid == 0) {
      uint32_t m = 0;
      for (int w = 0; w < nwave; ++w) m = max(m, s_red[w]);
      atomicMax(p.furthest_out, m);
    }
    return;
  }
  const uint32_t TL = 4 + 3 * T;  // scr_stride >= TL is guaranteed by the host
  float* myp = reinterpret_cast<float*>(smem + L.off_scr) + (size_t)wave * L.scr_stride;
  if (lane == 0) {
    myp[0] = m_run;
    myp[1] = s_run;
    myp[2] = __uint_as_float(S_local);   // F = index + fraction (smpc_dev.h)
    myp[3] = (float)n_noncoll;
  }
#pragma unroll
  for (int r = 0; r < R; ++r) {
    if (STEP_OK(r)) {
      myp[4 + t0 + r] = Ux[r];
      myp[4 + T + t0 + r] = Uy[r];
      myp[4 + 2 * T + t0 + r] = Uz[r];
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
        const float sc = expf(p.neg_inv_temp * (mw - bm));
        acc += sc * allp[(size_t)w * L.scr_stride + i];
      }
    }
    smpc_store_partial(outp + i, acc);
  }
#undef STEP_OK
#undef WAVE_PASS_GRID
  if constexpr (!MANY) {
    if (p.tail) smpc_grid_tail<(R == 4 ? 8 : 16)>(p, smem);
  }
}
