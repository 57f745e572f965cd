// smpc_wave_common.h — what the translation units of the wave-per-rollout pass share (smpc_kernels.hip:
// smpc_pass; smpc_wave_many.hip: smpc_pass_many): the cross-lane helpers the text of the pass
// (smpc_wave_pass.inc) is written with.  Device code only.
#ifndef SMPC_WAVE_COMMON_H_
#define SMPC_WAVE_COMMON_H_

#define WAVE 64

// ---------------------------------------------------------------------------
// cross-lane helpers (DPP; gfx9 row_shr / row_bcast / wave_shr)
// ---------------------------------------------------------------------------
template <int CTRL, int ROW_MASK = 0xF>
__device__ __forceinline__ float dpp_f(float old, float v)
{
  return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(old), __float_as_int(v), CTRL,
                                                    ROW_MASK, 0xF, false));
}
template <int CTRL, int ROW_MASK = 0xF>
__device__ __forceinline__ uint32_t dpp_u(uint32_t old, uint32_t v)
{
  return (uint32_t)__builtin_amdgcn_update_dpp((int)old, (int)v, CTRL, ROW_MASK, 0xF, false);
}

// Inclusive + scan over the 64 lanes (all lanes must be active): Kogge–Stone inside the
// 16-lane DPP rows, then row_bcast:15 / :31 carry the row totals.  Written as one asm
// block so that every step is a single v_add_f32_dpp (hipcc leaves the two broadcast steps
// as mov + add + re-zeroing) and the VALU-write -> DPP-read wait states are explicit.
__device__ __forceinline__ float wave_scan_add(float v)
{
  asm volatile(
    "s_nop 1\n\t"
    "v_add_f32_dpp %0, %0, %0 row_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
    "s_nop 1\n\t"
    "v_add_f32_dpp %0, %0, %0 row_shr:2 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
    "s_nop 1\n\t"
    "v_add_f32_dpp %0, %0, %0 row_shr:4 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
    "s_nop 1\n\t"
    "v_add_f32_dpp %0, %0, %0 row_shr:8 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
    "s_nop 1\n\t"
    "v_add_f32_dpp %0, %0, %0 row_bcast:15 row_mask:0xa bank_mask:0xf\n\t"
    "s_nop 1\n\t"
    "v_add_f32_dpp %0, %0, %0 row_bcast:31 row_mask:0xc bank_mask:0xf\n\t"
    "s_nop 1\n\t"
    : "+v"(v));
  return v;
}
// two independent scans interleaved: one wait state between dependent steps instead of two
__device__ __forceinline__ void wave_scan_add2(float& a, float& b)
{
  asm volatile(
    "s_nop 1\n\t"
    "v_add_f32_dpp %0, %0, %0 row_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
    "v_add_f32_dpp %1, %1, %1 row_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
    "s_nop 0\n\t"
    "v_add_f32_dpp %0, %0, %0 row_shr:2 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
    "v_add_f32_dpp %1, %1, %1 row_shr:2 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
    "s_nop 0\n\t"
    "v_add_f32_dpp %0, %0, %0 row_shr:4 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
    "v_add_f32_dpp %1, %1, %1 row_shr:4 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
    "s_nop 0\n\t"
    "v_add_f32_dpp %0, %0, %0 row_shr:8 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
    "v_add_f32_dpp %1, %1, %1 row_shr:8 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
    "s_nop 0\n\t"
    "v_add_f32_dpp %0, %0, %0 row_bcast:15 row_mask:0xa bank_mask:0xf\n\t"
    "v_add_f32_dpp %1, %1, %1 row_bcast:15 row_mask:0xa bank_mask:0xf\n\t"
    "s_nop 0\n\t"
    "v_add_f32_dpp %0, %0, %0 row_bcast:31 row_mask:0xc bank_mask:0xf\n\t"
    "v_add_f32_dpp %1, %1, %1 row_bcast:31 row_mask:0xc bank_mask:0xf\n\t"
    "s_nop 1\n\t"
    : "+v"(a), "+v"(b));
}
__device__ __forceinline__ float wave_sum(float v)
{
  v = wave_scan_add(v);
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}
__device__ __forceinline__ double wave_sum_d(double v)
{
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, WAVE);
  return v;
}
// shr1(src) + addend in ONE instruction: lane l gets src[l-1] + addend[l], lane 0 gets
// 0 + addend[0] (bound_ctrl).  With addend = {first, 0, 0, ...} it is the reference's
// "column 0 is the initial value, column t is the previous column" shift.
__device__ __forceinline__ float dpp_shr1_add(float src, float addend)
{
  float d;
  asm volatile("s_nop 1\n\t"
               "v_add_f32_dpp %0, %1, %2 wave_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1"
               : "=v"(d) : "v"(src), "v"(addend));
  return d;
}
// value of lane-1 (lane 0 gets `first`)
__device__ __forceinline__ float wave_shr1(float v, float first)
{
  return dpp_f<0x138>(first, v);  // wave_shr:1
}
__device__ __forceinline__ float lane_bcast(float v, int lane)
{
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}

// max over the parked endpoints of argmin_j |path_j - endpoint|^2 (first minimum wins), as the
// BITS of the float F = index + fraction (smpc_dev.h): F >= 0, so its bits order like the value
__device__ __forceinline__ float furthest_fraction(float d_j, float d_next, float seg2)
{
  // the endpoint's coordinate along the segment from point j to j + 1, in segment lengths:
  // (L^2 + d_j^2 - d_{j+1}^2) / (2 L^2); clamped so that the sum still rounds to j
  const float t = seg2 > 0.f ? 0.5f + 0.5f * (d_j - d_next) / seg2 : 0.f;
  return fminf(fmaxf(t, -0.45f), 0.45f);
}

__device__ __forceinline__ uint32_t flush_endpoint_ring(const float* ring_x, const float* ring_y,
                                                        uint32_t n, const float* s_px,
                                                        const float* s_py, uint32_t P, int lane)
{
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  const bool on = (uint32_t)lane < n;
  const float ex = on ? ring_x[lane] : 0.f, ey = on ? ring_y[lane] : 0.f;
  float best = 3.4028234663852886e38f;  // numeric_limits<float>::max()
  uint32_t bi = 0;
  for (uint32_t j = 0; j < P; ++j) {
    const float ddx = s_px[j] - ex, ddy = s_py[j] - ey;
    const float d = ddx * ddx + ddy * ddy;
    if (d < best) {
      best = d;
      bi = j;
    }
  }
  float F = (float)bi;
  if (bi + 1 < P) {
    const float nx = s_px[bi + 1], ny = s_py[bi + 1];
    const float sx = nx - s_px[bi], sy = ny - s_py[bi];
    const float d_next = (nx - ex) * (nx - ex) + (ny - ey) * (ny - ey);
    F = fmaxf(F + furthest_fraction(best, d_next, sx * sx + sy * sy), 0.f);
  }
  uint32_t m = on ? __float_as_uint(F) : 0u;
  m = max(m, dpp_u<0x111>(0u, m));
  m = max(m, dpp_u<0x112>(0u, m));
  m = max(m, dpp_u<0x114>(0u, m));
  m = max(m, dpp_u<0x118>(0u, m));
  m = max(m, dpp_u<0x142, 0xA>(0u, m));
  m = max(m, dpp_u<0x143, 0xC>(0u, m));
  __builtin_amdgcn_wave_barrier();
  return (uint32_t)__builtin_amdgcn_readlane((int)m, 63);
}

// float min over the wave (any sign): one v_min_f32_dpp per step, no canonicalisation
__device__ __forceinline__ float wave_min_f(float v)
{
  asm volatile(
    "s_nop 1\n\t"
    "v_min_f32_dpp %0, %0, %0 row_shr:1 row_mask:0xf bank_mask:0xf\n\t"
    "s_nop 1\n\t"
    "v_min_f32_dpp %0, %0, %0 row_shr:2 row_mask:0xf bank_mask:0xf\n\t"
    "s_nop 1\n\t"
    "v_min_f32_dpp %0, %0, %0 row_shr:4 row_mask:0xf bank_mask:0xf\n\t"
    "s_nop 1\n\t"
    "v_min_f32_dpp %0, %0, %0 row_shr:8 row_mask:0xf bank_mask:0xf\n\t"
    "s_nop 1\n\t"
    "v_min_f32_dpp %0, %0, %0 row_bcast:15 row_mask:0xa bank_mask:0xf\n\t"
    "s_nop 1\n\t"
    "v_min_f32_dpp %0, %0, %0 row_bcast:31 row_mask:0xc bank_mask:0xf\n\t"
    "s_nop 1\n\t"
    : "+v"(v));
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}

// inclusive + scan inside segments of 16 << (seg_shift - 4) lanes (16, 32 or 64)
__device__ __forceinline__ float seg_scan_add(float v, uint32_t seg_shift)
{
  asm volatile(
    "s_nop 1\n\t"
    "v_add_f32_dpp %0, %0, %0 row_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
    "s_nop 1\n\t"
    "v_add_f32_dpp %0, %0, %0 row_shr:2 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
    "s_nop 1\n\t"
    "v_add_f32_dpp %0, %0, %0 row_shr:4 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
    "s_nop 1\n\t"
    "v_add_f32_dpp %0, %0, %0 row_shr:8 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
    "s_nop 1\n\t"
    : "+v"(v));
  if (seg_shift >= 5) {
    asm volatile("v_add_f32_dpp %0, %0, %0 row_bcast:15 row_mask:0xa bank_mask:0xf\n\ts_nop 1\n\t"
                 : "+v"(v));
  }
  if (seg_shift >= 6) {
    asm volatile("v_add_f32_dpp %0, %0, %0 row_bcast:31 row_mask:0xc bank_mask:0xf\n\ts_nop 1\n\t"
                 : "+v"(v));
  }
  return v;
}

#endif  // SMPC_WAVE_COMMON_H_
