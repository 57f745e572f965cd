// smpc_stats_reduce.inc — the reduction of the critic breakdown: ONE text for its two kernel pairs
// (smpc_wave_stats.hip: smpc_reduce_stats / smpc_reduce_stats_final of one planning instance;
// smpc_wave_stats_many.hip: the same with the member of a group as a further grid dimension), as
// reduce_partials_body is for the tick's reduction.  The bodies take the slice, the row and the
// slice count as arguments instead of reading the grid: the sums are the same sums in the same order
// whichever kernel runs them.  Needs WAVE, wave_min_f, wave_sum_d (smpc_wave_common.h) and
// SmpcStatsOut (smpc_inst.h).

// ---------------------------------------------------------------------------
// the reduction
// ---------------------------------------------------------------------------
constexpr uint32_t kRows = SMPC_STATS_ROWS;          // 13: the twelve critics and the control row
constexpr uint32_t kPartDoubles = 4;                 // per (row, slice)
constexpr uint32_t kReduceBlock = 1024;

__device__ __forceinline__ uint32_t wave_min_u(uint32_t v)
{
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, (uint32_t)__shfl_xor((int)v, o, WAVE));
  return v;
}
__device__ __forceinline__ float wave_max_f(float v) {return -wave_min_f(-v);}

// four consecutive floats from index i (a multiple of four) of a 16-byte aligned row whose
// allocation is padded to whole quads; elements at or beyond `end` read as `fill`
__device__ __forceinline__ void load_quad(const float* __restrict__ row, uint32_t i, uint32_t end, float fill, float (&v)[4])
{
  const float4 q = *reinterpret_cast<const float4*>(row + i);
  v[0] = i < end ? q.x : fill;
  v[1] = i + 1 < end ? q.y : fill;
  v[2] = i + 2 < end ? q.z : fill;
  v[3] = i + 3 < end ? q.w : fill;
}

// part[(row * S + slice) * 4 + k]: rows 0..12 {sum, min, max, sum w t}; row 13 {sum w, sum w^2, least
// cost, its rollout}, the weights relative to the slice's least cost
// sx: the slice this block reduces, of S; row: its row (kRows: the weights)
__device__ __forceinline__ void reduce_stats_body(const float* __restrict__ stats, uint32_t ld, const float* __restrict__ costs,
                                                  uint32_t B, uint32_t slice, float k2, double* __restrict__ part, uint32_t S,
                                                  uint32_t sx, uint32_t row)
{
  __shared__ float s_m[16], s_x[16];
  __shared__ uint32_t s_i[16];
  __shared__ double s_a[16], s_b[16];
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid >> 6, nwave = blockDim.x >> 6;
  const uint32_t b0 = sx * slice, b1 = min(B, b0 + slice);   // (slice: a multiple of four)
  // ---- the slice's least cost, and the first rollout that has it ----
  float m = 3.0e38f;
  uint32_t mi = 0xffffffffu;
  for (uint32_t i = b0 + 4u * tid; i < b1; i += 4u * blockDim.x) {
    float c[4];
    load_quad(costs, i, b1, 3.0e38f, c);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (c[k] < m) {   // (strict, rising index: the lowest index among ties)
        m = c[k];
        mi = i + k;
      }
    }
  }
  {
    const float wm = wave_min_f(m);
    const uint32_t wi = wave_min_u(m == wm ? mi : 0xffffffffu);
    if (lane == 0) {
      s_m[wave] = wm;
      s_i[wave] = wi;
    }
  }
  __syncthreads();
  m = s_m[0];
  mi = s_i[0];
  for (int w = 1; w < nwave; ++w) {
    const float wm = s_m[w];
    const uint32_t wi = s_i[w];
    if (wm < m || (wm == m && wi < mi)) {
      m = wm;
      mi = wi;
    }
  }
  // ---- the row over the slice ----
  const bool weights = row == kRows;
  const float* __restrict__ r = weights ? costs : stats + (size_t)row * ld;
  double a = 0.0, aw = 0.0;
  float mn = 3.0e38f, mx = -3.0e38f;
  for (uint32_t i = b0 + 4u * tid; i < b1; i += 4u * blockDim.x) {
    float c[4], t[4];
    load_quad(costs, i, b1, 3.0e38f, c);
    load_quad(r, i, b1, 0.f, t);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const bool on = i + k < b1;
      // exp(-(c - m)/temperature) as the pass forms it: one v_exp_f32 of k2 (c - m)
      const double w = on ? (double)__builtin_amdgcn_exp2f(k2 * (c[k] - m)) : 0.0;
      if (weights) {
        a += w;
        aw += w * w;
      } else {
        a += (double)t[k];
        aw += w * (double)t[k];
        if (on) {
          mn = fminf(mn, t[k]);
          mx = fmaxf(mx, t[k]);
        }
      }
    }
  }
  a = wave_sum_d(a);
  aw = wave_sum_d(aw);
  mn = wave_min_f(mn);
  mx = wave_max_f(mx);
  __syncthreads();   // (s_m is read above)
  if (lane == 0) {
    s_a[wave] = a;
    s_b[wave] = aw;
    s_m[wave] = mn;
    s_x[wave] = mx;
  }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < nwave; ++w) {   // (wave order: the same sum on every run)
      a += s_a[w];
      aw += s_b[w];
      mn = fminf(mn, s_m[w]);
      mx = fmaxf(mx, s_x[w]);
    }
    double* o = part + ((size_t)row * S + sx) * kPartDoubles;
    if (weights) {
      o[0] = a; o[1] = aw; o[2] = (double)m; o[3] = (double)mi;
    } else {
      o[0] = a; o[1] = (double)mn; o[2] = (double)mx; o[3] = aw;
    }
  }
}

// wave k < 13: row k over the slices; wave 13: the weights; wave 14: the pass's non-colliding count
// (slot 3 of its per-block partials)
__device__ __forceinline__ void reduce_stats_final_body(const double* __restrict__ part, uint32_t S, float k2,
                                                        const float* __restrict__ stats, uint32_t ld,
                                                        const float* __restrict__ pass_partials, uint32_t nblk, uint32_t TL,
                                                        SmpcStatsOut* __restrict__ out)
{
  __shared__ double s_sum[kRows + 1], s_w[kRows + 1];
  __shared__ float s_mn[kRows], s_mx[kRows];
  __shared__ float s_best_cost;
  __shared__ uint32_t s_best;
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid >> 6;
  const double* pw = part + (size_t)kRows * S * kPartDoubles;   // the weights' slices
  // the batch's least cost and the first rollout that has it (every wave for itself)
  float m = 3.0e38f;
  uint32_t mi = 0xffffffffu;
  for (uint32_t s = lane; s < S; s += WAVE) {
    const float ms = (float)pw[s * kPartDoubles + 2];
    const uint32_t is = (uint32_t)pw[s * kPartDoubles + 3];
    if (ms < m || (ms == m && is < mi)) {
      m = ms;
      mi = is;
    }
  }
  const float gm = wave_min_f(m);
  uint32_t gi = wave_min_u(m == gm ? mi : 0xffffffffu);
  if (gi >= ld) gi = 0u;   // (no cost below 3e38, a NaN among them: no rollout is "best"; stay inside the rows)
  double a = 0.0, aw = 0.0;
  float mn = 3.0e38f, mx = -3.0e38f;
  if (wave <= (int)kRows) {
    const double* pr = part + (size_t)wave * S * kPartDoubles;
    for (uint32_t s = lane; s < S; s += WAVE) {
      // a slice's weights are relative to its own least cost: rescale as the pass rescales its running sums
      const double f = (double)__builtin_amdgcn_exp2f(k2 * ((float)pw[s * kPartDoubles + 2] - gm));
      const double* o = pr + s * kPartDoubles;
      if (wave == (int)kRows) {
        a += f * o[0];
        aw += f * f * o[1];
      } else {
        a += o[0];
        mn = fminf(mn, (float)o[1]);
        mx = fmaxf(mx, (float)o[2]);
        aw += f * o[3];
      }
    }
  } else if (wave == (int)kRows + 1) {
    for (uint32_t g = lane; g < nblk; g += WAVE) a += (double)pass_partials[(size_t)g * TL + 3];
  }
  a = wave_sum_d(a);
  aw = wave_sum_d(aw);
  mn = wave_min_f(mn);
  mx = wave_max_f(mx);
  if (lane == 0) {
    if (wave <= (int)kRows) {
      s_sum[wave] = a;
      s_w[wave] = aw;
    }
    if (wave < (int)kRows) {
      s_mn[wave] = mn;
      s_mx[wave] = mx;
    }
    if (wave == (int)kRows) {
      s_best_cost = gm;
      s_best = gi;
    }
    if (wave == (int)kRows + 1) out->non_colliding = (float)a;
  }
  __syncthreads();
  const double W = s_sum[kRows], W2 = s_w[kRows];
  if (tid < (int)kRows) {
    out->sum[tid] = (float)s_sum[tid];
    out->min[tid] = s_mn[tid];
    out->max[tid] = s_mx[tid];
    out->weighted[tid] = (float)(s_w[tid] / W);
    out->at_best[tid] = stats[(size_t)tid * ld + s_best];
  }
  if (tid == (int)kRows) {
    out->best_rollout = s_best;
    out->best_cost = s_best_cost;
    out->effective_samples = (float)(W * W / W2);
  }
}
