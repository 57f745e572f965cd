// smpc_moving_cost.inc — the two forms of the moving-obstacle term (DESIGN.md 4.6), ONE text compiled
// under two pairs of names, as smpc_wave_pass.inc serves smpc_pass and smpc_pass_many:
//   smpc_moving.hip       smpc_moving_cost_gm<VY>, smpc_moving_cost_rm<R>: one context, its arguments
//                         (SmpcMovingArgs, u of iteration 0 included) in the kernel argument segment
//   smpc_moving_many.hip  smpc_moving_cost_gm_many<VY>, smpc_moving_cost_rm_many<R> (MOVING_COST_MANY):
//                         the member of a group is blockIdx.y, its arguments (SmpcMovingMember) come
//                         from device memory, u always from the device, and a block beyond the member's
//                         own grid leaves before the first barrier having written nothing
// The arithmetic and its order are the same by construction: the two compilations differ in where `p`
// comes from and in which blocks exist, nothing else.
//
// The includer defines MOVING_COST_GM and MOVING_COST_RM (the kernels' names) and, for the grouped
// form, MOVING_COST_MANY.

#if defined(MOVING_COST_MANY)
#define MOVING_ARGS SmpcMovingMember
#define MOVING_PARAMS const SmpcMovingMember* __restrict__ many
#define MOVING_MEMBER                                 \
  const SmpcMovingMember& p = many[blockIdx.y];       \
  if (blockIdx.x >= p.grid) return;   // (the whole block, in front of every barrier)
#else
#define MOVING_ARGS SmpcMovingArgs
#define MOVING_PARAMS const SmpcMovingArgs p
#define MOVING_MEMBER
#endif

namespace {

// u of the iteration: device memory (a later iteration, or a group's member) or this launch's own kernel arguments
__device__ __forceinline__ const float* moving_u(const MOVING_ARGS& p)
{
#if defined(__HIP_DEVICE_COMPILE__) && !defined(MOVING_COST_MANY)
  if (!p.u_dev)
    return reinterpret_cast<const float*>(reinterpret_cast<const uint8_t*>(__builtin_amdgcn_kernarg_segment_ptr()) +
                                          __builtin_offsetof(SmpcMovingArgs, u_arg));
#endif
  return p.u_dev;
}

// one disc at one trajectory point; `reach`: radius + margin as the host formed it in float
__device__ __forceinline__ void moving_term(float d2, float radius, float reach, float margin, float& sum, bool& hit)
{
  const float d = sqrtf(d2);
  const float q = fminf(fmaxf((reach - d) / margin, 0.f), 1.f);
  sum += q;
  hit = hit || d < radius;
}

__device__ __forceinline__ void moving_store(const MOVING_ARGS& p, uint32_t b, float sum, bool hit)
{
  const float m = (float)((double)p.repulsion_weight * (double)sum / (double)p.T + (hit ? (double)p.collision_cost : 0.0));
  p.seed[b] = p.add ? (float)((double)p.seed[b] + (double)m) : m;
  if (p.m_out) p.m_out[b] = m;
  if (p.hit_out) p.hit_out[b] = hit ? 1 : 0;
}

}  // namespace

// Group-major form.  A wave takes one group of 64 rollouts, a block four groups.
template <bool VY>
__global__ void __launch_bounds__(256) MOVING_COST_GM(MOVING_PARAMS)
{
  MOVING_MEMBER
  __shared__ float4 su4[3 * SMPC_MOVING_MAX_T / 4];   // u in quads [3][T4 / 4], zeros in the padding steps
  float* su = reinterpret_cast<float*>(su4);
  const uint32_t T = p.T, T4 = SMPC_GM_STEPS(T), Q = T4 >> 2, K = p.K;
  {
    const float* u = moving_u(p);
    for (uint32_t i = threadIdx.x; i < 3 * T4; i += 256) {
      const uint32_t k = i / T4, t = i - k * T4;
      su[i] = t < T ? u[k * T + t] : 0.f;
    }
  }
  __syncthreads();
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t g = blockIdx.x * 4u + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (g >= (p.B + 63u) / 64u) return;
  const uint32_t b = g * 64u + lane;
  const size_t at = static_cast<size_t>(g) * Q * 64u + lane;   // in quads; the next quad of the lane is 64 further
  const float4* __restrict__ s0 = reinterpret_cast<const float4*>(p.n[0]) + at;
  const float4* __restrict__ s1 = reinterpret_cast<const float4*>(p.n[VY ? 1 : 0]) + at;
  const float4* __restrict__ s2 = reinterpret_cast<const float4*>(p.n[2]) + at;
  const float4* __restrict__ tab = reinterpret_cast<const float4*>(p.tab);
  const float dt = p.dt, yaw0 = p.yaw0, margin = p.margin;
  const double x0 = p.x0, y0 = p.y0;
  float cpx = p.v0[0], cpy = VY ? p.v0[1] : 0.f, cpz = p.v0[2];   // v[:,0] = measured speed, v[:,t] = c[:,t-1]
  float acc_yaw = 0.f, ax = 0.f, ay = 0.f;
  float cs_prev = p.cos0, sn_prev = p.sin0;
  float sum = 0.f;
  bool hit = false;
  // one time step for the 64 rollouts of this wave, as the lane-per-rollout pass takes it
  auto step = [&](uint32_t t, float ux, float uy, float uz, float n0, float n1, float n2) {
    const float cvx = ux + n0, cvy = VY ? uy + n1 : 0.f, cwz = uz + n2;
    const float vx = cpx, vy = cpy, wz = cpz;
    cpx = cvx; cpy = cvy; cpz = cwz;
    acc_yaw = acc_yaw + wz * dt;
    const float yaw = acc_yaw + yaw0;
    const float dxr = VY ? vx * cs_prev - vy * sn_prev : vx * cs_prev;
    const float dyr = VY ? vx * sn_prev + vy * cs_prev : vx * sn_prev;
    ax = ax + dxr * dt;
    ay = ay + dyr * dt;
    smpc_sincos(yaw, sn_prev, cs_prev);
    const float x = (float)(x0 + (double)ax), y = (float)(y0 + (double)ay);
    const float4* __restrict__ row = tab + static_cast<size_t>(t) * K;
    for (uint32_t k = 0; k < K; ++k) {
      const float4 o = row[k];   // wave-uniform: {x, y, guarded squared reach, radius}
      const float dx = x - o.x, dy = y - o.y;
      const float d2 = dx * dx + dy * dy;
      if (__builtin_amdgcn_ballot_w64(d2 < o.z) != 0) moving_term(d2, o.w, o.w + margin, margin, sum, hit);
    }
  };
  float4 n0 = s0[0], n1 = VY ? s1[0] : make_float4(0.f, 0.f, 0.f, 0.f), n2 = s2[0];
  for (uint32_t q = 0; q < Q; ++q) {
    float4 m0 = n0, m1 = n1, m2 = n2;
    if (q + 1 < Q) {
      const size_t o = static_cast<size_t>(q + 1) * 64u;
      m0 = s0[o];
      if (VY) m1 = s1[o];
      m2 = s2[o];
    }
    const float4 ux = su4[q], uy = su4[Q + q], uz = su4[2u * Q + q];
    const uint32_t t0 = 4u * q;   // (t0 < T always: T4 - 4 < T)
    step(t0, ux.x, uy.x, uz.x, n0.x, n1.x, n2.x);
    if (t0 + 1 < T) step(t0 + 1, ux.y, uy.y, uz.y, n0.y, n1.y, n2.y);
    if (t0 + 2 < T) step(t0 + 2, ux.z, uy.z, uz.z, n0.z, n1.z, n2.z);
    if (t0 + 3 < T) step(t0 + 3, ux.w, uy.w, uz.w, n0.w, n1.w, n2.w);
    n0 = m0; n1 = m1; n2 = m2;
  }
  if (b < p.B) moving_store(p, b, sum, hit);   // (padding rollouts of the last group: zero noise, scored, never stored)
}

// Row-major form.  A wave takes one rollout, a block four; lane l owns steps l R .. l R + R - 1.
template <int R>
__global__ void __launch_bounds__(256) MOVING_COST_RM(MOVING_PARAMS)
{
  MOVING_MEMBER
  const uint32_t T = p.T, K = p.K;
  const int lane = threadIdx.x & (WAVE - 1);
  const uint32_t b = blockIdx.x * 4u + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (b >= p.B) return;   // (the whole wave: every lane of the others stays active for the scans)
  const int t0 = lane * R;
#define STEP_OK(r) ((uint32_t)(t0 + (r)) < T)
  const float* u = moving_u(p);
  const size_t row = static_cast<size_t>(b) * T;
  float cvx[R], cvy[R], cwz[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const bool a = STEP_OK(r);
    // NoiseGenerator::setNoisedControls: c = u + noise (vy of a non-holonomic model: none)
    cvx[r] = a ? u[t0 + r] + p.n[0][row + t0 + r] : 0.f;
    cvy[r] = (a && p.n[1]) ? u[T + t0 + r] + p.n[1][row + t0 + r] : 0.f;
    cwz[r] = a ? u[2 * T + t0 + r] + p.n[2][row + t0 + r] : 0.f;
  }
  const float dt = in_vgpr(p.dt), yaw0_v = in_vgpr(p.yaw0);
  const double x0_v = in_vgpr(p.x0), y0_v = in_vgpr(p.y0);
  const float first_vx = lane == 0 ? p.v0[0] : 0.f, first_vy = lane == 0 ? p.v0[1] : 0.f;
  const float first_wz = lane == 0 ? p.v0[2] : 0.f;
  const float first_cos = lane == 0 ? p.cos0 : 0.f, first_sin = lane == 0 ? p.sin0 : 0.f;
  // ---- updateStateVelocities + predict: v[:,0]=speed, v[:,1:]=c[:,:-1] (smpc_wave_pass.inc) ---
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
#pragma unroll
  for (int r = 0; r < R; ++r) {
    if (!STEP_OK(r)) vx[r] = vy[r] = wz[r] = 0.f;
  }
  // ---- integrateStateVelocities ------------------------------------------------------------
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
      yaw[0] = incl + yaw0_v;
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
  // ---- the discs: lane = its steps, the table read [k][t] ----------------------------------
  const float2* __restrict__ tab = reinterpret_cast<const float2*>(p.tab);
  const float4* __restrict__ disc = reinterpret_cast<const float4*>(p.disc);
  const float margin = p.margin;
  float sum = 0.f;
  bool hit = false;
  for (uint32_t k = 0; k < K; ++k) {
    const float4 dk = disc[k];   // wave-uniform: {radius, radius + margin, guarded squared reach, 0}
#pragma unroll
    for (int r = 0; r < R; ++r) {
      float d2 = 3.0e38f;   // (a step past the horizon: out of every reach)
      if (STEP_OK(r)) {
        const float2 o = tab[static_cast<size_t>(k) * T + t0 + r];
        const float dx = x[r] - o.x, dy = y[r] - o.y;
        d2 = dx * dx + dy * dy;
      }
      if (d2 < dk.z) moving_term(d2, dk.x, dk.y, margin, sum, hit);
    }
  }
#undef STEP_OK
  const float total = wave_sum(sum);
  const bool any_hit = __builtin_amdgcn_ballot_w64(hit) != 0;
  if (lane == 0) moving_store(p, b, total, any_hit);
}

#undef MOVING_ARGS
#undef MOVING_PARAMS
#undef MOVING_MEMBER
