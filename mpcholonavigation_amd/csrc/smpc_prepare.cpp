// smpc_prepare.cpp — the per-tick host work behind the C-ABI (include/smpc.h): what the
// reference's critics do once per tick (goal-distance gates, path validity, cumulative path
// lengths, the per-candidate PathAlign / PathFollow tables), the 256-entry lookup tables of
// the collision critics, the tick block the kernels read, and the LDS carve-up of the passes.
#include "smpc_ctx.h"

namespace smpc_impl {

TickLayout tick_layout(uint32_t T, uint32_t P)
{
  TickLayout l{};
  size_t o = 0;
  // the tick's number sits right in front of u: a pass finds it at u[-4] with no pointer of its
  // own (the lane pass has no scalar register to spare for one)
  l.canary = o; o += 16;
  l.u = o; o += align_up(3 * T * 4, 16);
  l.px = o; o += align_up(P * 4, 16);
  l.py = o; o += align_up(P * 4, 16);
  l.pyaw = o; o += align_up(P * 4, 16);
  l.D = o; o += align_up(P * 4, 16);
  l.pf_idx = o; o += align_up(P * 4, 16);
  l.pvalid = o; o += align_up(P, 16);
  l.pa_active = o; o += align_up(P, 16);
  l.pang_active = o; o += align_up(P, 16);
  l.pal_active = o; o += align_up(P, 16);   // PathAlignLegacy gate per candidate furthest point
  l.lut_cost = o; o += 256 * 4;   // CostCritic repulsive term per 8-bit cost
  l.prune = o; o += SMPC_PRUNE_FLOATS * 4;   // lane pass: furthest-point prune table (build_prune_table)
  l.total = o;
  return l;
}

SmpcLds make_lds(uint32_t window_bytes, uint32_t P, uint32_t T, uint32_t nwave, bool with_map,
                 uint32_t nsamp)
{
  SmpcLds L{};
  uint32_t o = with_map ? align_up(window_bytes, 16) : 0;
  // 256 entries + one all-zero entry (index 256: the lane pass primes its lookup pipeline with it)
  L.off_lut = o; o += with_map ? (256 + 2) * sizeof(SmpcLut) : 0;
  const uint32_t pf = align_up(std::max(P, 1u) * 4, 16);
  L.off_px = o; o += pf;
  L.off_py = o; o += pf;
  L.off_pyaw = o; o += pf;
  L.off_D = o; o += align_up((std::max(P, 1u) + 2) * 4, 16);   // + a sentinel on either side (lane pass)
  L.off_valid = o; o += align_up(std::max(P, 1u), 16);
  L.off_scr = o;
  // lanes per parked rollout: sample slots 0..nsamp fit one segment of 16/32/64 lanes;
  // rollouts per flush: as many segments as a wave has, capped so that the parked
  // controls stay <= 3 KiB per wave
  const uint32_t R = T <= 64 ? 1 : (T <= 128 ? 2 : 4);
  L.seg_shift = nsamp + 1 <= 16 ? 4 : (nsamp + 1 <= 32 ? 5 : 6);
  L.group = std::max(1u, std::min(64u >> L.seg_shift, 4u / R));
  // per wave: [sample points 3x64][endpoint ring 2x64][parked controls group x 3T]; the head is
  // re-used for the block combine [4+3T]
  L.scr_pts = 0;
  L.scr_ring = 3 * 64;
  L.scr_c = L.scr_ring + 2 * 64;
  L.scr_stride = align_up(std::max(L.scr_c + L.group * 3 * T, 4 + 3 * T), 4);
  o += nwave * L.scr_stride * 4;
  L.total = o;
  return L;
}

// LDS layout of the lane-per-rollout pass: window + the NO_INFORMATION byte + one scratch byte
// per lane (cell_byte_exact), LUT, path, per wave the parked wz [64][68] + weights [64]; the
// re-read form parks nothing (per wave only the block combine's tuple)
SmpcLds lane_lds(uint32_t window_bytes, uint32_t P, uint32_t T, bool rr)
{
  const uint32_t lblock = rr ? smpc_lane_block_rr() : smpc_lane_block();
  SmpcLds Lt = make_lds(window_bytes ? window_bytes + 1 + lblock : 0, P, T, lblock / 64,
                        window_bytes != 0, 0);
  // the furthest-point prune table (528 bytes; the parked wz dominates: 8 x 17.7 KB of the 160 KB)
  Lt.off_prune = Lt.off_scr;
  Lt.off_pts4 = Lt.off_prune + SMPC_PRUNE_FLOATS * 4;
  Lt.off_scr = Lt.off_pts4 + align_up(std::max(P, 1u) * 16, 16) + 16;   // + sum u^2 per control (the gamma terms), 16 bytes
  Lt.scr_stride = rr ? align_up(4u + 3u * T, 4) : align_up(std::max(64u * 68u + 64u, 4u + 3u * T), 4);
  Lt.total = Lt.off_scr + (lblock / 64) * Lt.scr_stride * 4;
  return Lt;
}

// LDS layout of smpc_pass_split: as the lane pass up to the path points, then sum u^2 [4] and the
// control sequence [3][64] in front of the per-wave scratch (parked wz [16][64]; the block
// combine's tuple re-uses it)
SmpcLds split_lds(uint32_t window_bytes, uint32_t P, uint32_t T, uint32_t nseg)
{
  const uint32_t lblock = smpc_split_block();
  SmpcLds Lt = make_lds(window_bytes ? window_bytes + 1 + lblock : 0, P, T, lblock / 64, window_bytes != 0, 0);
  Lt.off_pts4 = Lt.off_scr;
  Lt.off_scr += align_up(std::max(P, 1u) * 16, 16) + 16 + 3 * 64 * 4;
  // parked wz [steps per lane][64]; two segments: vy too (smpc_split.hip PARK_VY)
  Lt.scr_stride = align_up(std::max((nseg == 2 ? 2u : 1u) * (64u / nseg) * 64u, 4u + 3u * T), 4);
  Lt.total = Lt.off_scr + (lblock / 64) * Lt.scr_stride * 4;
  return Lt;
}

// distanceToObstacle (obstacles_critic.cpp:99-112) for an 8-bit cost, point mode
static float distance_to_obstacle(const HostCostmap& m, float cost, bool using_footprint = false)
{
  const float scale_factor = m.cost_scaling_factor;
  const float min_radius = m.inscribed_radius;
  float d = static_cast<float>(
    (static_cast<double>(scale_factor * min_radius) - std::log(static_cast<double>(cost)) +
    std::log(static_cast<double>(253.0f))) / static_cast<double>(scale_factor));
  if (!using_footprint) d -= min_radius;   // obstacles_critic.cpp:106-108
  return d;
}

// consider_fp: the critic's consider_footprint collision rule; using_fp: the cost came from the
// footprint (no inscribed-radius offset, obstacles_critic.cpp:106-108)
// cost_terms (non-null: CostCritic scored WITHOUT ObstaclesCritic): the table's second field is the
// CostCritic's per-cost term (cost_critic.cpp:141-155) instead of ObstaclesCritic's repulsion — the
// first field keeps the shared collision marker and is otherwise zero — so that the lane pass's
// lookup pipeline scores CostCritic as it stands; the wave pass reads only the marker then
static void build_lut(const HostCostmap& m, const smpc_obstacles_params& p, bool near_goal, SmpcLut* lut,
                      bool consider_fp = false, bool using_fp = false, const float* cost_terms = nullptr)
{
  for (int v = 0; v < 256; ++v) {
    lut[v].crit = 0.f;
    lut[v].rep = 0.f;
    if (cost_terms) {
      if (v == SMPC_COST_LETHAL || (v == SMPC_COST_INSCRIBED && !consider_fp) ||
        (v == SMPC_COST_NO_INFORMATION && !m.track_unknown))
      {
        lut[v].crit = -1.0f;
      } else {
        lut[v].rep = cost_terms[v];
      }
      continue;
    }
    // inCollision (obstacles_critic.cpp:185-201), consider_footprint = false
    if (v == SMPC_COST_LETHAL || (v == SMPC_COST_INSCRIBED && !consider_fp) ||
      (v == SMPC_COST_NO_INFORMATION && !m.track_unknown))
    {
      lut[v].crit = -1.0f;                                   // :152 collision marker
      continue;
    }
    if (v < 1) continue;                                     // :150 free space
    if (m.inflation_radius == 0.0f || m.cost_scaling_factor == 0.0f) continue;  // :155
    const float d = distance_to_obstacle(m, static_cast<float>(v), using_fp);
    if (d < p.collision_margin_distance) {
      lut[v].crit = p.collision_margin_distance - d;         // :165
    } else if (!near_goal) {
      lut[v].rep = m.inflation_radius - d;                   // :167
    }
  }
}

// The lane pass's furthest-point prune table (smpc_lane_furthest.inc reads it).
//
// A speculating lane pass reports max over the live rollouts of F_b = bi + clamp(tt, +-0.45), bi the
// first nearest path point of the rollout's endpoint e and tt the endpoint's projection parameter on
// the segment behind p_bi.  Given a bound theta = K + phi (K = rint(theta)) that some rollout has
// already attained, a rollout with F_b <= theta adds nothing to the maximum.  Entry K lets a lane
// prove that in ~12 instructions.  With e' = e - p_K, n the unit vector along p_K -> p_K+1,
// s = n.e', t = n_perp.e', all divided by a radius R = 64 segment lengths (so that the entry is
// scale-free: {p_K, n / R, kappa, rho~, R / seg, m'}):
//   (0) max(|s|, |t|) <= 1            the endpoint is within R of p_K: bounds every rounding error
//                                     below, and a NaN or far-away endpoint fails it;
//   (a) s + kappa |t| <= rho~         p_K is at least as near as every LATER point p_j, so the first
//                                     nearest index is <= K.  With v_j = p_j - p_K = alpha_j n +
//                                     beta_j n_perp: d_j - d_K = |v_j|^2 - 2 e'.v_j and e'.v_j <=
//                                     alpha_j (s + kappa |t|) for kappa = max |beta_j| / alpha_j, so
//                                     rho = min |v_j|^2 / (2 alpha_j) suffices.  Points further than
//                                     3 R away cannot be nearer than p_K under (0) and are left out;
//                                     an alpha_j <= 0 among the rest (the plan doubles back, points
//                                     repeat) makes the entry "never prune" (rho~ = -4: (0) has s >= -1);
//   (b) K + max(s R / seg + m',       if the nearest index IS K: s R / seg + m' >= the kernel's tt,
//       -0.45) <= theta               and the clamp, the float sum with K and the final max(., 0) are
//                                     monotone, so the left side is >= F_b (the upper clamp is left
//                                     out: beyond it the left side exceeds K + 0.45 >= theta anyway).
//                                     A nearest index below K gives F_b <= K - 0.55 <= theta whatever
//                                     (b) says.
//   K = P - 1: no later point, F_b = K exactly: R / seg = 0 and m' = 0, (b) reads K <= theta.
// Margins, u = 2^-24.  The kernel's dd = ex * ex + ey * ey (ex = q - x rounded, no contraction) is
// within 5 u dd of the true squared distance.  (a) must make the FLOAT d_K <= the float d_j: the
// true difference has to exceed 5 u (d_j + d_K), where d_K <= 2 R^2 and d_j <= (sqrt 2 R + |v_j|)^2
// <= 4 R^2 + 2 |v_j|^2 under (0); rho is lowered by m = 4 max_j 5 u (d_j + d_K) / (2 alpha_j) (four times what is
// needed).  The test's own arithmetic (e' rounded, n / R rounded, two products, a sum, kappa |t|)
// is off by less than 16 u (1 + kappa) in units of R; rho~ is lowered by 64 u (1 + kappa), kappa is
// rounded up and rho~ down.  (b): the kernel's tt = 0.5 + 0.5 (d_K - d_K+1) * rcp(seg2) differs from
// the true parameter by at most 0.5 * 5 u (d_K + d_K+1) / seg^2 (the two distances) plus 10 u |tt -
// 0.5| + u (difference, reciprocal of a rounded seg2, products, sum; |tt| <= 92 under (0)), the
// test's s R / seg by 16 u * 64 + 2 u * 92: m' is twice the sum of all of them, ~5.2e-3; m is 3 % of
// half a segment on a straight plan.
// A false "cannot raise the maximum" would be a wrong result, a false "can" costs one scan.
// on = false (SMPC_FURTHEST_PRUNE=0, plans beyond kPruneMaxPath points): every entry "never prune".
void build_prune_table(const float* px, const float* py, uint32_t P, uint32_t k0, bool on, float* out)
{
  const double u = 5.9604644775390625e-08;   // 2^-24
  const uint32_t n = P > k0 ? std::min(P - k0, SMPC_PRUNE_ENTRIES) : 0u;
  memset(out, 0, SMPC_PRUNE_FLOATS * sizeof(float));
  memcpy(out, &k0, 4);
  memcpy(out + 1, &n, 4);
  for (uint32_t i = 0; i < n; ++i) {
    const uint32_t K = k0 + i;
    float* e = out + 4 + 8 * i;
    const double kx = px[K], ky = py[K];
    e[0] = px[K];
    e[1] = py[K];
    e[5] = -4.0f;   // never prune, until everything below holds
    if (!on) continue;
    // the segment behind p_K; at the plan's last point the one in front of it gives the frame
    const bool last = K + 1 >= P;
    double gx = 1.0, gy = 0.0;
    if (!last) {
      gx = static_cast<double>(px[K + 1]) - kx;
      gy = static_cast<double>(py[K + 1]) - ky;
    } else if (K > 0) {
      gx = kx - px[K - 1];
      gy = ky - py[K - 1];
    }
    const double seg = std::sqrt(gx * gx + gy * gy);
    if (!(seg > 0.0) || !std::isfinite(seg)) {
      if (!last) continue;
      gx = 1.0; gy = 0.0;   // (a one-point plan, or its last two points coincide: any frame)
    } else {
      gx /= seg; gy /= seg;
    }
    const double R = 64.0 * (seg > 0.0 && std::isfinite(seg) ? seg : 1.0);
    double kappa = 0.0, rho = 1.0e30, m = 0.0;
    bool ok = true;
    for (uint32_t j = K + 1; j < P; ++j) {
      const double vx = static_cast<double>(px[j]) - kx, vy = static_cast<double>(py[j]) - ky;
      const double v2 = vx * vx + vy * vy;
      if (v2 >= 9.0 * R * R) continue;      // cannot be nearer than p_K while (0) holds
      const double al = gx * vx + gy * vy, be = gx * vy - gy * vx;
      if (!(al > 0.0)) {
        ok = false;
        break;
      }
      // d_j <= (sqrt 2 R + |v_j|)^2 <= 4 R^2 + 2 |v_j|^2 (no square root: this runs 16 P times a tick)
      const double ial = 1.0 / al, dj = 4.0 * R * R + 2.0 * v2;
      kappa = std::max(kappa, std::fabs(be) * ial);
      rho = std::min(rho, 0.5 * v2 * ial);
      m = std::max(m, 2.5 * u * (dj + 2.0 * R * R) * ial);
    }
    if (!ok || !std::isfinite(kappa) || kappa > 64.0) continue;
    const double rho_s = (rho - 4.0 * m) / R - 64.0 * u * (1.0 + kappa);
    double inv = 0.0, mb = 0.0;
    if (!last) {
      const double dsum = 2.0 * R * R + (1.4142136 * R + seg) * (1.4142136 * R + seg);
      inv = R / seg;
      mb = 2.0 * (0.5 * 5.0 * u * dsum / (seg * seg) + 10.0 * u * 92.0 + u + 16.0 * u * inv + 2.0 * u * 92.0);
    }
    e[2] = static_cast<float>(gx / R);
    e[3] = static_cast<float>(gy / R);
    e[4] = kappa > 0.0 ? std::nextafter(static_cast<float>(kappa * (1.0 + 4.0 * u)), 3.0e38f) : 0.f;
    e[6] = static_cast<float>(inv);
    e[7] = mb > 0.0 ? std::nextafter(static_cast<float>(mb), 3.0e38f) : 0.f;
    // (1e30: no later point)
    e[5] = std::nextafter(static_cast<float>(std::min(rho_s, 1.0e30)), -3.0e38f);
  }
}

void remember_furthest(smpc_ctx* c, const smpc_tick_in* in, float F)
{
  // what the prediction for THIS tick missed is how far the rollouts' endpoints moved relative
  // to the robot since the last tick (the control sequence is still changing: an accelerating
  // robot reaches further every tick); to first order it does so again
  static const bool trace = getenv("SMPC_TRACE_FURTHEST") != nullptr;
  if (trace)
    fprintf(stderr, "[smpc furthest] true %.3f predicted %.3f (geometry %.3f, valid %d, drift %.3f)\n", F,
            c->pred.hint_Fp + c->pred.hint_drift, c->pred.hint_Fp, (int)c->pred.hint_Fp_valid, c->pred.hint_drift);
  // A tick scored with NEW noise (regenerate_noises = true) moves the extreme rollout by itself:
  // at 2 097 152 rollouts the true value jitters by +-0.5 of an index from epoch to epoch.  What
  // the last prediction missed is then mostly that jitter, not a trend: carrying it forward as
  // drift doubles it (observed: 1.55 scoring passes per tick).  Such ticks update a smoothed
  // estimate instead — the next prediction starts from F' + 0.4 (F - F'), F' the geometric
  // prediction of this tick — and leave the drift alone.
  const bool fresh_noise = c->noise.noise_gen != c->pred.noise_gen_remembered;
  c->pred.noise_gen_remembered = c->noise.noise_gen;
  float F_next = F;
  if (c->pred.hint_Fp_valid) {
    const float d = F - c->pred.hint_Fp;
    if (fresh_noise && std::fabs(d) < 2.f) {
      F_next = c->pred.hint_Fp + c->pred.hint_drift + 0.4f * (F - (c->pred.hint_Fp + c->pred.hint_drift));
      c->pred.hint_drift *= 0.5f;
    } else {
      c->pred.hint_drift = std::fabs(d) < 2.f ? d : 0.f;
    }
  } else {
    c->pred.hint_drift = 0.f;
  }
  c->pred.hint_Fp_valid = false;
  c->pred.hint_F = F_next;
  c->pred.hint = smpc_furthest_index(F_next);
  c->pred.hint_valid = true;
  c->pred.anchor_x = in->pose_x;
  c->pred.anchor_y = in->pose_y;
  c->pred.anchor_ex = c->pred.cur_ex;
  c->pred.anchor_ey = c->pred.cur_ey;
  c->pred.anchor_e_valid = c->pred.cur_e_valid;
  c->pred.cur_e_valid = false;
  c->pred.anchor_px.assign(in->path_x, in->path_x + in->path_len);
  c->pred.anchor_py.assign(in->path_y, in->path_y + in->path_len);
  c->pred.anchor_valid = true;
}

// The index a tick is first scored with.  Between two ticks the robot advances and the plan
// handed over by the controller is pruned to the robot (path_handler.cpp:48-143), so the
// furthest reached path point of the last tick is stale by construction: at 0.3 m/s, 20 Hz
// and 0.05 m between path points the index moves once every three ticks from the motion and
// once every three ticks, the other way, from the pruning.  Both are known on the host: the
// displacement of the pose along the plan at the furthest point, in segment lengths, and the
// number of points the plan lost at its start (the old point the new first point coincides
// with).  F' = F + displacement - shift, index = round(F').  Exactness never depends on this:
// the scoring pass reports the true value and a miss is re-scored.
// Where the rollout WITHOUT noise ends: pose + sum of the rotated state velocities (v[0] the measured
// speed, v[t] = u[t - 1]; optimizer.cpp:258-267, 313-343), in double with the rotation advanced by
// its Taylor terms — this feeds the prediction only, 0.2 us per tick.
static void nominal_endpoint(const smpc_ctx* c, const smpc_tick_in* in, const float* u, double& ex, double& ey)
{
  const uint32_t T = c->cfg.time_steps;
  const double dt = c->cfg.model_dt;
  double co = std::cos(static_cast<double>(in->pose_yaw)), si = std::sin(static_cast<double>(in->pose_yaw));
  double x = 0.0, y = 0.0;
  double vx = in->speed_vx, vy = c->holonomic ? in->speed_vy : 0.0, wz = in->speed_wz;
  for (uint32_t t = 0; t < T; ++t) {
    x += (vx * co - vy * si) * dt;      // cos_[t] = cos(yaw[t - 1])
    y += (vx * si + vy * co) * dt;
    const double a = wz * dt, a2 = a * a;
    const double ca = 1.0 - 0.5 * a2 + a2 * a2 * (1.0 / 24.0), sa = a * (1.0 - a2 * (1.0 / 6.0));
    const double cn = co * ca - si * sa;
    si = si * ca + co * sa;
    co = cn;
    vx = u[t];
    vy = c->holonomic ? u[T + t] : 0.0;
    wz = u[2 * T + t];
  }
  ex = in->pose_x + x;
  ey = in->pose_y + y;
}

void predict_hint(smpc_ctx* c, const smpc_tick_in* in, const float* u_in)
{
  // The rollouts are the nominal one plus the SAME noise tick after tick: their furthest point
  // moves with the nominal endpoint — the robot's motion and the change of the control sequence
  // (a sequence still accelerating reaches further every tick, and stops doing so where it meets
  // the constraints: the kink a tick-to-tick drift estimate overshoots).
  c->pred.cur_e_valid = false;
  if (u_in) {
    nominal_endpoint(c, in, u_in, c->pred.cur_ex, c->pred.cur_ey);
    c->pred.cur_e_valid = true;
  }
  if (!c->pred.hint_valid || !c->pred.anchor_valid) return;
  const uint32_t P0 = static_cast<uint32_t>(c->pred.anchor_px.size()), P = in->path_len;
  c->pred.hint = smpc_furthest_index(c->pred.hint_F);
  if (c->pred.hint_is_this_ticks) {
    // smpc_group_optimize re-runs a member whose prediction missed: hint_F is this very tick's
    // true value.  Score with it, and leave the drift as remember_furthest measured it.
    c->pred.hint_is_this_ticks = false;
    c->pred.hint_Fp = c->pred.hint_F - c->pred.hint_drift;
    c->pred.hint_Fp_valid = true;
    return;
  }
  c->pred.hint_Fp_valid = false;
  if (P0 < 2 || P < 1) return;
  const float* ox = c->pred.anchor_px.data();
  const float* oy = c->pred.anchor_py.data();
  auto d2 = [](float ax, float ay, float bx, float by) {return (ax - bx) * (ax - bx) + (ay - by) * (ay - by);};
  // the old point the new plan starts at
  uint32_t k = 0;
  float best = std::numeric_limits<float>::max();
  for (uint32_t j = 0; j < P0; ++j) {
    const float d = d2(ox[j], oy[j], in->path_x[0], in->path_y[0]);
    if (d < best) {
      best = d;
      k = j;
    }
  }
  const uint32_t kn = k + 1 < P0 ? k + 1 : k - 1;
  const float seg_k = d2(ox[k], oy[k], ox[kn], oy[kn]);
  if (!(best <= 0.0625f * seg_k)) return;   // not a pruned copy of the old plan: nothing to carry over
  uint32_t S0 = c->pred.hint;
  if (S0 >= P0) S0 = P0 - 1;
  const uint32_t Sn = S0 + 1 < P0 ? S0 + 1 : S0 - 1;
  const float sx = (S0 + 1 < P0 ? 1.f : -1.f) * (ox[Sn] - ox[S0]), sy = (S0 + 1 < P0 ? 1.f : -1.f) * (oy[Sn] - oy[S0]);
  const float seg2 = sx * sx + sy * sy;
  if (!(seg2 > 0.f)) return;
  // displacement along the plan at the furthest point, in segment lengths: of the nominal endpoint
  // when both ticks have one, else of the pose alone
  const bool by_endpoint = c->pred.cur_e_valid && c->pred.anchor_e_valid;
  const double dx = by_endpoint ? c->pred.cur_ex - c->pred.anchor_ex : in->pose_x - c->pred.anchor_x;
  const double dy = by_endpoint ? c->pred.cur_ey - c->pred.anchor_ey : in->pose_y - c->pred.anchor_y;
  const float disp = static_cast<float>(dx * sx + dy * sy) / seg2;
  if (!(std::fabs(disp) < (by_endpoint ? 8.f : 4.f))) return;     // a jump, not a controller period's motion
  const float Fp0 = c->pred.hint_F + disp - static_cast<float>(k);   // carried by the geometry alone
  const float Fp = Fp0 + c->pred.hint_drift;                          // ... and by last tick's drift
  c->pred.hint_Fp = Fp0;
  c->pred.hint_Fp_valid = true;
  long h = std::lround(Fp);
  if (h < 0) h = 0;
  if (h > static_cast<long>(P) - 1) h = static_cast<long>(P) - 1;
  c->pred.hint = static_cast<uint32_t>(h);
}

int check_tick(smpc_ctx* c, const smpc_tick_in* in)
{
  if (!c || !in) return SMPC_ERR_INVALID;
  if (!c->noise.have_noise) return fail(c, SMPC_ERR_STATE, "no noise: call smpc_set_noise or smpc_seed");
  if (in->path_len > 0 && (!in->path_x || !in->path_y || !in->path_yaw))
    return fail(c, SMPC_ERR_INVALID, "path arrays missing");
  if (in->path_len > SMPC_MAX_PATH)
    return fail(c, SMPC_ERR_UNSUPPORTED, "path longer than SMPC_MAX_PATH (1024) points");
  if (!c->map.set && (c->critics.obstacles.enabled || c->critics.cost.enabled || !in->path_pts_valid))
    return fail(c, SMPC_ERR_STATE, "no costmap: call smpc_set_costmap");
  if (((c->critics.obstacles.enabled && c->critics.obstacles.consider_footprint) ||
    (c->critics.cost.enabled && c->critics.cost.consider_footprint)) && c->fp_x.empty())
    return fail(c, SMPC_ERR_STATE, "consider_footprint=true needs a footprint: call smpc_set_footprint");
  return SMPC_OK;
}

// Which critics score this tick: membership in the critics list, and for the gated ones the
// reference's withinPositionGoalTolerance test at the top of score().  Also the
// number of PathAlign samples per trajectory.
static int tick_gates(smpc_ctx* c, const smpc_tick_in* in, uint32_t& gates_out, uint32_t& nsamp_out)
{
  const uint32_t T = c->cfg.time_steps, P = in->path_len;
  const auto& cr = c->critics;
  const double rx = in->pose_x, ry = in->pose_y, gx = in->goal_x, gy = in->goal_y;
  uint32_t gates = 0;
  if (cr.obstacles.enabled) gates |= SD_OBSTACLES;
  if (cr.path_align.enabled && !within_tol(cr.path_align.threshold_to_consider, rx, ry, gx, gy))
    gates |= SD_PATH_ALIGN;                                   // path_align_critic.cpp:49-54
  if (cr.path_follow.enabled && P >= 2 &&
    !within_tol(cr.path_follow.threshold_to_consider, rx, ry, gx, gy))
    gates |= SD_PATH_FOLLOW;                                  // path_follow_critic.cpp:37-42
  if (cr.goal_angle.enabled && P >= 1 &&
    within_tol(cr.goal_angle.threshold_to_consider, rx, ry, gx, gy))
    gates |= SD_GOAL_ANGLE;                                   // goal_angle_critic.cpp:38-43
  if (cr.prefer_forward.enabled &&
    !within_tol(cr.prefer_forward.threshold_to_consider, rx, ry, gx, gy))
    gates |= SD_PREFER_FORWARD;                               // prefer_forward_critic.cpp:36-41
  // the other registered critics (general pass only)
  if (cr.constraint.enabled) gates |= SD_CONSTRAINT;
  if (cr.cost.enabled) gates |= SD_COST;
  if (cr.obstacles.enabled && cr.obstacles.consider_footprint) gates |= SD_FP_OBSTACLES;
  if (cr.cost.enabled && cr.cost.consider_footprint) gates |= SD_FP_COST;
  if (cr.goal.enabled && within_tol(cr.goal.threshold_to_consider, rx, ry, gx, gy))
    gates |= SD_GOAL;                                         // goal_critic.cpp:38-42
  if (cr.twirling.enabled) {
    // utils::withinPositionGoalTolerance(goal_checker, ...) (tools/utils.hpp:201-224)
    bool within = false;
    if (in->goal_checker_xy_tolerance >= 0.0f) {
      const double tol = static_cast<double>(in->goal_checker_xy_tolerance);
      const double dx = rx - gx, dy = ry - gy;
      within = dx * dx + dy * dy < tol * tol;
    }
    if (!within) gates |= SD_TWIRLING;                        // twirling_critic.cpp:33-37
  }
  if (cr.path_angle.enabled && P >= 1 &&
    !within_tol(cr.path_angle.threshold_to_consider, rx, ry, gx, gy))
    gates |= SD_PATH_ANGLE;                                   // path_angle_critic.cpp:60-69
  if (cr.velocity_deadband.enabled) gates |= SD_DEADBAND;
  // PathAlignLegacyCritic (path_align_legacy_critic.cpp:48-54, :86-88: at least one path segment)
  if (cr.path_align_legacy.enabled && P >= 2 &&
    !within_tol(cr.path_align_legacy.threshold_to_consider, rx, ry, gx, gy))
    gates |= SD_PATH_ALIGN_LEGACY;
  if (P == 0) gates &= ~(SD_PATH_ALIGN | SD_PATH_FOLLOW);
  uint32_t nsamp = 0;
  const uint32_t step = cr.path_align.trajectory_point_step;
  if (gates & SD_PATH_ALIGN) {
    nsamp = step > 0 ? (T - 1) / step : 0;
    if (nsamp > 63)
      return fail(c, SMPC_ERR_UNSUPPORTED,
                  "PathAlign: more than 63 samples per trajectory (time_steps / trajectory_point_step)");
    if (nsamp == 0) gates &= ~SD_PATH_ALIGN;  // no samples: cost 0 for every rollout
    if (cr.path_align.use_path_orientations) gates |= SD_USE_PATH_YAW;
  }
  if (gates & SD_PATH_ALIGN_LEGACY) {
    // its trajectory points are PathAlign's: p = step, 2 step, ... < T (path_align_legacy_critic.cpp:97)
    const uint32_t lstep = cr.path_align_legacy.trajectory_point_step;
    if ((gates & SD_PATH_ALIGN) && lstep != step)
      return fail(c, SMPC_ERR_UNSUPPORTED,
                  "PathAlignCritic and PathAlignLegacyCritic in one list need the same trajectory_point_step");
    const uint32_t ns = lstep > 0 ? (T - 1) / lstep : 0;
    if (ns > 63)
      return fail(c, SMPC_ERR_UNSUPPORTED,
                  "PathAlignLegacy: more than 63 samples per trajectory (time_steps / trajectory_point_step)");
    if (ns == 0) gates &= ~SD_PATH_ALIGN_LEGACY;   // no samples: summed_dist 0, cost 0 for every rollout
    else nsamp = ns;
    if (cr.path_align_legacy.use_path_orientations && (gates & SD_PATH_ALIGN_LEGACY)) gates |= SD_PAL_USE_PATH_YAW;
  }
  if (gates & (SD_PATH_ALIGN | SD_PATH_FOLLOW | SD_PATH_ANGLE | SD_PATH_ALIGN_LEGACY)) gates |= SD_NEED_FURTHEST;
  if (c->map.track_unknown) gates |= SD_TRACK_UNKNOWN;
  if (c->cfg.flags & SMPC_FLAG_STORE_TRAJECTORIES) gates |= SD_STORE_TRAJ;

  gates_out = gates;
  nsamp_out = nsamp;
  return SMPC_OK;
}

// Path validity (utils::findPathCosts) and PathAlign's cumulative path lengths, into the tick
// block: pvalid[P-1], D[P-1].
static void path_tables(const HostCostmap& map, const smpc_tick_in* in, uint32_t gates, const float* px,
                        const float* py, uint8_t* pvalid, float* D)
{
  const uint32_t P = in->path_len;
  // ---- path validity (utils::findPathCosts, tools/utils.hpp:361-395) ----------
  const uint32_t nseg = P > 0 ? P - 1 : 0;
  if (in->path_pts_valid) {
    memcpy(pvalid, in->path_pts_valid, nseg);
  } else if (gates & (SD_PATH_ALIGN | SD_PATH_FOLLOW | SD_PATH_ALIGN_LEGACY)) {
    for (uint32_t i = 0; i < nseg; ++i) {
      unsigned mx, my;
      uint8_t v = 1;
      if (!world_to_map(map, px[i], py[i], mx, my)) {
        v = 0;
      } else {
        const uint8_t cost = map.cells.get()[static_cast<size_t>(my) * map.W + mx];
        if (cost == SMPC_COST_LETHAL || cost == SMPC_COST_INSCRIBED) v = 0;
        else if (cost == SMPC_COST_NO_INFORMATION) v = map.track_unknown ? 1 : 0;
      }
      pvalid[i] = v;
    }
  } else {
    memset(pvalid, 0, std::max(nseg, 1u));
  }

  // ---- PathAlign: cumulative path lengths (path_align_critic.cpp:82-90) --------
  if (nseg) {
    D[0] = 0.0f;
    for (uint32_t i = 1; i < nseg; ++i) {
      const float dx = px[i] - px[i - 1];
      const float dy = py[i] - py[i - 1];
      D[i] = D[i - 1] + sqrtf(dx * dx + dy * dy);
    }
  }

}

// ---- the stages of plan_launch ---------------------------------------------------------------

// The costmap window staged in LDS, centred on the robot: its corner and size into d, its bytes
// returned (0: no collision critic scored, or no map).
static uint32_t plan_window(const smpc_ctx* c, const smpc_tick_in* in, uint32_t gates, SmpcDev& d)
{
  const uint32_t T = c->cfg.time_steps;
  uint32_t window_bytes = 0;
  if (c->map.set && (gates & (SD_OBSTACLES | SD_COST))) {
    uint32_t side = 4;
    while ((side + 4) * (side + 4) <= kWindowBytes) side += 4;   // 96 cells
    // Long horizons reach further than that: 128 steps of 0.05 s at 0.5 m/s are 3.2 m, and a
    // rollout outside the window fetches its cells from the global map behind a full memory
    // wait, inside the time loop (the 262 144 x 128 pass: 183 us with the 96-cell window, 150 us
    // with 128..144 cells; beyond that the staging of the window by every block costs more than
    // the stragglers, tools/kbench.py with SMPC_WINDOW_SIDE_MAX).  For T > 64 the window covers
    // the reach at the largest constrained speed plus four standard deviations of the mean
    // noise, up to kWindowSideMax cells; the passes that run T > 64 (the re-read form, the
    // wave-per-rollout pass) have the LDS for it.
    if (T > 64 && !c->knobs.small_window) {
      const float sigma = std::max(c->cfg.vx_std, c->holonomic ? c->cfg.vy_std : 0.f);
      const float vmax = std::max(std::max(std::fabs(c->c_vx_max), std::fabs(c->c_vx_min)), std::fabs(c->c_vy)) +
        4.f * sigma / std::sqrt(static_cast<float>(T));
      const double reach_cells = static_cast<double>(T) * c->cfg.model_dt * vmax / c->map.res;
      const uint32_t want = (static_cast<uint32_t>(2.0 * reach_cells) + 8u + 3u) & ~3u;
      const uint32_t side_max = c->knobs.window_side_max < 0 ? kWindowSideMax : static_cast<uint32_t>(c->knobs.window_side_max) & ~3u;
      side = std::max(side, std::min(want, side_max));
    }
    const uint32_t ww = std::min(c->map.W, side), wh = std::min(c->map.H, side);
    long cx = static_cast<long>((in->pose_x - c->map.ox) / c->map.res);
    long cy = static_cast<long>((in->pose_y - c->map.oy) / c->map.res);
    long wx0 = cx - ww / 2, wy0 = cy - wh / 2;
    wx0 = std::max(0L, std::min(wx0, static_cast<long>(c->map.W) - static_cast<long>(ww)));
    wy0 = std::max(0L, std::min(wy0, static_cast<long>(c->map.H) - static_cast<long>(wh)));
    wx0 &= ~3L;
    d.win_x0 = static_cast<int32_t>(wx0); d.win_y0 = static_cast<int32_t>(wy0);
    d.win_w = static_cast<int32_t>(ww); d.win_h = static_cast<int32_t>(wh);
    window_bytes = ww * wh;
  }
  return window_bytes;
}

// The wave-pass MODE the tick's critics need.  Decides and writes nothing.
static int wave_mode(uint32_t gates, const smpc_critic_params& cr, const Knobs& knobs)
{
  int mode_now = smpc_ctx::score_mode_for(cr);
  // the lean kernels: MODE 0 scores the north star's five away from the goal, MODE 3 also the
  // additive forms of Cost, Goal, Constraint, Twirling, PathAngle (the deployed list) and of the
  // near-goal GoalAngle term; MODE 4 is MODE 3 with the footprint check of the list's one collision
  // critic (consider_footprint: the deployed YAML as written).  Everything else (a cost_power other
  // than 1, trajectory write-out, path orientations, VelocityDeadband, PathAlignLegacy, a footprint
  // with BOTH collision critics in the list: its counting pass is the general one's) takes the
  // general pass — or, for a cost_power among the five and nothing else, the lane pass's power rows
  // (below).  No lane or split instance carries a footprint: such a tick runs the wave pass at any
  // batch.  SMPC_FOOTPRINT_PASS=general keeps footprint ticks on the general pass.
  const uint32_t fp_gates = SD_FP_OBSTACLES | SD_FP_COST;
  const uint32_t lean_extra = SD_CONSTRAINT | SD_COST | SD_GOAL | SD_TWIRLING | SD_PATH_ANGLE | SD_GOAL_ANGLE;
  const bool fp_general = knobs.footprint_general || ((gates & SD_OBSTACLES) && (gates & SD_COST));
  if (gates & (SD_STORE_TRAJ | SD_USE_PATH_YAW | (SD_EXTRA_CRITICS & ~(lean_extra | fp_gates)))) {
    mode_now = 2;
  } else if ((gates & fp_gates) && fp_general) {
    mode_now = 2;
  } else if (gates & (lean_extra | fp_gates)) {
    const bool unit_powers = (!cr.constraint.enabled || cr.constraint.cost_power == 1) &&
      (!cr.cost.enabled || cr.cost.cost_power == 1) && (!cr.goal.enabled || cr.goal.cost_power == 1) &&
      (!cr.twirling.enabled || cr.twirling.cost_power == 1) && (!cr.path_angle.enabled || cr.path_angle.cost_power == 1) &&
      (!(gates & SD_GOAL_ANGLE) || cr.goal_angle.cost_power == 1);
    mode_now = (mode_now == 0 && unit_powers) ? ((gates & fp_gates) ? 4 : 3) : 2;
  }
  return mode_now;
}

// The wave-per-rollout pass: planned for every tick.  Its LDS carve-up and persistent grid.
static int plan_wave(smpc_ctx* c, uint32_t window_bytes, uint32_t P, uint32_t nsamp, int mode_now, PassPlan& pl)
{
  const uint32_t T = c->cfg.time_steps, B = c->cfg.batch_size;
  pl.wave.block = pass_block(c->R);
  pl.wave.lds = make_lds(window_bytes, P, T, (pass_block(c->R) / 64), window_bytes != 0, nsamp);
  if (pl.wave.lds.total > kLdsPerCu) return fail(c, SMPC_ERR_UNSUPPORTED, "LDS budget exceeded");
  // room for the reduction inside the scoring launch (smpc_tail.h works in the launch's LDS) —
  // only for contexts that run that experiment: for 128 < T <= 256 the padding would halve the
  // wave pass's blocks per CU
  if (c->knobs.fused_reduce) pl.wave.lds.total = std::max(pl.wave.lds.total, smpc_tail_lds_bytes(T));

  // persistent grid: as many blocks as stay resident, never more than the work
  const uint32_t waves_per_block = (pass_block(c->R) / 64);
  const WaveInst* wave = wave_select(c->R, mode_now, T);
  if (!wave) return fail(c, SMPC_ERR_UNSUPPORTED, "no instance of the wave-per-rollout pass for this horizon");
  uint32_t per_cu = std::min(c->occ_wave.get(wave->fn, pl.wave.block, pl.wave.lds.total), 32u / waves_per_block);
  if (c->knobs.max_blocks_per_cu >= 1) per_cu = std::min(per_cu, c->knobs.max_blocks_per_cu);   // SMPC_MAX_BLOCKS_PER_CU
  uint32_t grid = std::min((B + waves_per_block - 1) / waves_per_block,
                           static_cast<uint32_t>(c->num_cu) * per_cu);
  pl.wave.grid = std::max(1u, std::min(grid, kMaxGrid));
  return SMPC_OK;
}

// The lane-per-rollout pass takes the tick when the kernels score with unit cost powers (MODE 0
// or 3) and lane_select has an instance for the gates: the north star's five, with the near-goal
// GoalAngle term (ObstaclesCritic scored, T <= 64), or with the deployed list's Constraint / Cost /
// Twirling on a cruise tick (T = 64 or the default 56).  Known to the host only: PathAngle must
// be inside its angle for every candidate furthest point (it then adds nothing), and the lane
// pass samples PathAlign's trajectory points at the first step of every quad
// (trajectory_point_step = 4, the reference's default: path_align_critic.cpp:36).
static bool lane_eligible(const smpc_ctx* c, uint32_t gates, int mode_now, uint32_t step)
{
  const uint32_t T = c->cfg.time_steps;
  return c->noise.use_tpr && (mode_now == 0 || mode_now == 3) && T <= kLaneMaxT &&
    lane_select(gates, T, T > 64, false, c->acker_r, false) != nullptr &&
    !((gates & SD_PATH_ANGLE) && c->pang_any) && !((gates & SD_PATH_ALIGN) && step != 4);
}

// The re-read form (no parked controls) is the only one for T > 64; SMPC_LANE_REREAD=1 selects
// it for T <= 64 too (experiments) where it has an instance.
static bool lane_reread_form(const smpc_ctx* c, uint32_t gates)
{
  const uint32_t T = c->cfg.time_steps;
  return (T > 64 || c->knobs.lane_reread) && lane_select(gates, T, true, false, c->acker_r, false) != nullptr;
}

// A cost_power other than 1 among the five critics (near the goal: GoalAngle's too) puts the tick
// in MODE 2.  When that power is the ONLY reason — no trajectory write-out, no path orientations,
// no critic beyond the five — the tick still takes the lane pass, on the rows of
// smpc_pass_lane_pow (parking form: T <= 64, trajectory_point_step 4), which apply each power to
// its critic's per-rollout total in the epilogue.  From kLaneMinBatch rollouts up only, also for
// a context that asks for the lane pass (SMPC_FLAG_LANE_PER_ROLLOUT, SMPC_PASS=lane): that is the
// crossover below which the lane pass loses to the wave pass, and the power rows have not been
// measured below it.  Never the split or the re-read form.
static bool lane_power_rows(const smpc_ctx* c, uint32_t gates, int mode_now, uint32_t step, bool rr)
{
  const uint32_t T = c->cfg.time_steps, B = c->cfg.batch_size;
  return mode_now == 2 && c->score_mode_for(c->critics) == 2 && c->noise.use_tpr && !rr && T <= 64 && step == 4 &&
    B >= kLaneMinBatch && !(gates & (SD_STORE_TRAJ | SD_USE_PATH_YAW | SD_EXTRA_CRITICS)) &&
    lane_select(gates, T, false, false, c->acker_r, true) != nullptr;
}

// The lane pass's cell lookup: window-relative float cell index and its guard band, into d (the
// window itself is plan_window's).  The pass forms
//   q~ = fma(ax, (1/res)_f, cxf),   cxf = ((x0 - window corner) / res)_f
// from the accumulated displacement ax; the reference truncates
//   Q = ((double)x - origin) / res - win_x0,   x = (float)(x0 + (double)ax).
// |q~ - Q| is at most: the rounding of x to float, (1/2) ulp(|x|) / res with |x| inside the
// window (lanes outside it never take the fast path); three float roundings of quantities
// no larger than the window (the two constants' images and the fma's own); and the rounding
// of the window corner origin + win0 * res in double.
// (cell_eps_w; the wave pass's guard band cell_eps has other terms: fill_dev_state)
static void lane_cell_constants(const HostCostmap& map, const smpc_tick_in* in, SmpcDev& d)
{
  const double rinv = 1.0 / map.res;
  const double wx = map.ox + static_cast<double>(d.win_x0) * map.res;
  const double wy = map.oy + static_cast<double>(d.win_y0) * map.res;
  d.wxf = static_cast<float>(wx);
  d.wyf = static_cast<float>(wy);
  d.cxf = static_cast<float>((in->pose_x - wx) * rinv);
  d.cyf = static_cast<float>((in->pose_y - wy) * rinv);
  const double ext_x = static_cast<double>(d.win_w + 1) * map.res, ext_y = static_cast<double>(d.win_h + 1) * map.res;
  const double xmax = std::max(std::max(std::fabs(wx - map.res), std::fabs(wx + ext_x)),
                               std::max(std::fabs(wy - map.res), std::fabs(wy + ext_y)));
  const double u24 = 5.9604644775390625e-08;   // 2^-24
  const double e_c = 2.3e-16 * (std::fabs(wx) + std::fabs(wy) + 1.0);
  const double qmax = static_cast<double>(std::max(d.win_w, d.win_h)) + 2.0;
  const double eps = 2.0 * (u24 * xmax * rinv + 3.0 * u24 * qmax + e_c * rinv) + 1e-7;
  d.cell_eps_w = static_cast<float>(std::min(eps, 0.5));
}

// The lane pass's LDS, block and grid into pl, its cell-index constants into c->dev.  False: the
// pass does not fit (long paths: the parked wz no longer fits) and the tick takes the wave pass.
static bool plan_lane(smpc_ctx* c, const smpc_tick_in* in, uint32_t window_bytes, PassPlan& pl)
{
  const uint32_t T = c->cfg.time_steps, B = c->cfg.batch_size, P = in->path_len;
  pl.window_bytes = window_bytes;
  pl.lane.lds = lane_lds(window_bytes, P, T, pl.rr);
  const bool fits = pl.lane.lds.total <= kLdsPerCu;
  // (the re-read form: no in-launch reduction, smpc_lane.hip)
  if (!pl.rr && c->knobs.fused_reduce) pl.lane.lds.total = std::max(pl.lane.lds.total, smpc_tail_lds_bytes(T));
  if (!fits) return false;
  const uint32_t lblock = pl.rr ? smpc_lane_block_rr() : smpc_lane_block();
  uint32_t occ_blocks = c->occ_lane.get(lane_occupancy_row(T, pl.rr)->fn, lblock, pl.lane.lds.total);
  if (pl.rr) occ_blocks = std::min(occ_blocks, 3u);   // (four-wave blocks: launch bounds of three waves per SIMD)
  const uint32_t groups = (B + 63) / 64;
  uint32_t wpb = lblock / 64;
  pl.lane.block = lblock;
  // Small batches: when every group can have a SIMD to itself (at most four groups per CU),
  // blocks of four waves, one per CU.  Two waves on a SIMD share its VALU and each runs its
  // group in 22.5 us; a wave alone runs it in 20.5 (tools/lane_timeline.py) — and a batch
  // this small is one group per wave anyway: -2 us per tick at 65 536 x 64.
  if (!pl.rr && c->knobs.half_blocks && !c->in_group && groups <= static_cast<uint32_t>(c->num_cu) * 4u) {
    wpb = 4;
    pl.lane.block = 256;
  }
  uint32_t g = std::min((groups + wpb - 1) / wpb, static_cast<uint32_t>(c->num_cu) * occ_blocks);
  g = std::max(1u, std::min(g, kMaxGrid));
  // Every wave takes whole groups, so a launch lasts ceil(groups / waves) group-times whatever
  // the remainder: launch only the waves that fill every round, and — where several blocks fit
  // a CU — pad the launch's LDS so that the dispatcher cannot stack them unevenly.  (Built for
  // the re-read form's first shape, four-wave blocks at three per CU: 4096 groups on 3072 waves;
  // with the eight-wave blocks it has now the grid is one block per CU and this trims nothing
  // at the benchmarked sizes.  SMPC_NO_BALANCED_GRID=1: off.)
  if (pl.rr && c->knobs.balanced_grid) {
    const uint32_t waves = g * wpb;
    const uint32_t rounds = (groups + waves - 1) / waves;
    const uint32_t need = (groups + rounds - 1) / rounds;
    const uint32_t g2 = (need + wpb - 1) / wpb;
    const uint32_t per_cu = (g2 + c->num_cu - 1) / static_cast<uint32_t>(c->num_cu);
    if (g2 < g && per_cu < occ_blocks) {
      g = g2;
      const uint32_t pad = align_up(kLdsPerCu / (per_cu + 1) + 1024u, 16);
      if (pad <= kLdsPerCu / per_cu) pl.lane.lds.total = std::max(pl.lane.lds.total, pad);
    }
  }
  pl.lane.grid = g;
  lane_cell_constants(c->map, in, c->dev);
  return true;
}

// Small batches at T = 64: while the waves of smpc_pass_split (16 rollouts, four lanes each) have
// at most two groups each, the horizon split over four lanes runs the tick's one scoring pass in
// a fraction of a 64-step chain (65 536 x 64: one wave per SIMD on the lane pass).  The plain five
// critics only; the lane pass's geometry (window, cell index constants) is shared.  For a tick
// the lane pass takes; true: the split pass takes it instead, its LDS, block and grid in pl.
static bool plan_split(smpc_ctx* c, uint32_t gates, int mode_now, uint32_t step, uint32_t window_bytes, uint32_t P,
                       PassPlan& pl)
{
  const uint32_t T = c->cfg.time_steps, B = c->cfg.batch_size;
  const bool force_split = c->knobs.pass == Knobs::kSplit;
  bool split_now = false;
  if (!pl.rr && mode_now == 0 && T >= 36 && !c->in_group && !c->knobs.no_split && !c->knobs.fused_reduce &&
      (!c->lane_forced || force_split)) {
    // (a context that ASKS for the lane pass — SMPC_FLAG_LANE_PER_ROLLOUT, SMPC_PASS=lane — gets it)
    // one block per CU (two waves per SIMD: the kernel's registers), and ONE group per wave: four
    // lanes per rollout while 16-rollout groups fit (32 768 rollouts on 256 CUs), two up to twice that
    const uint32_t waves = static_cast<uint32_t>(c->num_cu) * (smpc_split_block() / 64u);
    // (the two-segment instance — 32 steps per lane, up to 65 536 rollouts at one group per wave —
    // is built and parity-tested but not selected: a half chain at twice the instructions per
    // step, 50.0 us per tick at 65 536 x 64 where the lane pass takes 49.9; SMPC_SPLIT_NSEG=2)
    uint32_t nseg = 0;
    if ((B + 15u) / 16u <= waves) nseg = 4;
    // (horizons below 64 run the masked instance: 16 384 x 56 takes 38.0 us against 37.2 on the wave
    // pass, 20 000 x 60 37.0 against 39.5, 32 768 x 56 39.0 against 43.5)
    if (T != 64 && B < kSplitMinBatchShort && !force_split) nseg = 0;
    if (c->knobs.split_nseg == 2 || c->knobs.split_nseg == 4) nseg = (nseg || force_split) ? c->knobs.split_nseg : 0;
    if (nseg == 2 && T != 64) nseg = 4;   // (the two-segment instance: T = 64 only)
    if (!nseg && force_split) nseg = 4;
    // (the plain five critics with ObstaclesCritic on, whole quads: split_select)
    if (nseg && split_select(gates, T, step, nseg)) {
      const SmpcLds Ls = split_lds(window_bytes, P, T, nseg);
      if (Ls.total <= kLdsPerCu) {
        const uint32_t occ_blocks = c->occ_split.get(split_occupancy_row(nseg)->fn, smpc_split_block(), Ls.total);
        const uint32_t per_block = smpc_split_rollouts_per_block(nseg);
        const uint32_t blocks = (B + per_block - 1) / per_block;
        const uint32_t resident = static_cast<uint32_t>(c->num_cu) * occ_blocks;
        split_now = true;
        pl.split_nseg = nseg;
        pl.split.lds = Ls;
        pl.split.block = smpc_split_block();
        pl.split.grid = std::max(1u, std::min(std::min(blocks, resident), kMaxGrid));   // (persistent: forced runs loop over groups)
      }
    }
  }
  return split_now;
}

// DiffDrive and Ackermann: vy is zero at every step, and the Omni-form rows read a zero-filled
// noise tensor and carry zeros through the rotation, the gamma sum, 64 parked registers and a
// transpose-reduce per group.  A tick that would run a PLAIN lane row anyway — lean MODE 0 with
// ObstaclesCritic scored, no GoalAngle term, no deployed-list critic, no cost power, the parking
// form in whole quads, one context — runs that row's twin of smpc_pass_lane_nh, which has no vy
// (same grid, block, LDS and group order: the geometry planned above; same results, DESIGN.md
// 4.2d).  From kLaneMinBatch rollouts up only, also for a context that asks for the lane pass
// (SMPC_FLAG_LANE_PER_ROLLOUT, SMPC_PASS=lane): nothing about these rows is measured below it.
// Every other tick of such a model keeps the Omni-form instance it had.  SMPC_NONHOLO_PASS=omni:
// the Omni-form rows for these ticks too.
static bool lane_nonholonomic_rows(const smpc_ctx* c, uint32_t gates, int mode_now, uint32_t step, const PassPlan& pl,
                                   bool lane_now, bool split_now)
{
  const uint32_t T = c->cfg.time_steps, B = c->cfg.batch_size;
  return !c->holonomic && !c->knobs.nonholo_omni && lane_now && !split_now && mode_now == 0 && !pl.pow && !pl.rr &&
    !c->in_group && step == 4 && T <= 64 && (T & 3u) == 0 && B >= kLaneMinBatch &&
    [&] {
      const LaneInst* k = lane_select(gates, T, false, false, c->acker_r, false, true);
      return k && k->nh;
    }();
}

// Launch geometry of the tick: the costmap window staged in LDS (centred on the robot), the LDS
// carve-up and persistent grid of the wave-per-rollout pass, which scoring mode the enabled
// critics need, and whether — and how — the lane-per-rollout pass takes the tick.  Reads
// c->pang_any (prepare_tick's PathAngle gates) and writes, into the c->dev prepare_tick has filled,
// the window (plan_window) and wxf / cxf / cell_eps_w (lane_cell_constants).  c->plan, which the
// NEXT tick's prune-table decision reads, is written only when everything succeeded.
static int plan_launch(smpc_ctx* c, const smpc_tick_in* in, uint32_t gates, uint32_t nsamp, int& mode_out)
{
  const uint32_t B = c->cfg.batch_size, P = in->path_len;
  const uint32_t step = c->critics.path_align.trajectory_point_step;
  const uint32_t window_bytes = plan_window(c, in, gates, c->dev);
  const int mode_now = wave_mode(gates, c->critics, c->knobs);
  PassPlan pl;
  const int rc = plan_wave(c, window_bytes, P, nsamp, mode_now, pl);
  if (rc != SMPC_OK) return rc;

  pl.rr = lane_reread_form(c, gates);
  bool lane_now = lane_eligible(c, gates, mode_now, step);
  pl.pow = lane_power_rows(c, gates, mode_now, step, pl.rr);
  if (pl.pow) lane_now = true;
  if (lane_now) lane_now = plan_lane(c, in, window_bytes, pl);
  const bool split_now = lane_now && plan_split(c, gates, mode_now, step, window_bytes, P, pl);

  // below kLaneMinBatch the lane pass itself loses to the wave pass (one group per CU's worth of
  // waves: crossover measured at ~50 k rollouts); such contexts keep the group-major noise only
  // for the split form
  if (lane_now && !split_now && B < kLaneMinBatch && !c->lane_forced) lane_now = false;

  pl.pow = pl.pow && lane_now;   // (a path too long for the lane pass's LDS: the wave pass after all)
  pl.nh = lane_nonholonomic_rows(c, gates, mode_now, step, pl, lane_now, split_now);
  pl.kind = split_now ? PassPlan::kSplit : (lane_now ? PassPlan::kLane : PassPlan::kWave);
  c->plan = pl;
  mode_out = mode_now;
  return SMPC_OK;
}

// ---- the stages of prepare_tick --------------------------------------------------------------
// The table builders among them take plain arrays, a critic's parameters and the costmap, never
// the context.

// the tick block's regions in its host copy (TickLayout's offsets as typed pointers)
struct TickFields {
  uint8_t* h;
  float *px, *py, *pyaw, *D;
  uint32_t* pf_idx;
  uint8_t *pvalid, *pa_active, *pang_active, *pal_active;
  float *lut_cost, *prune;
};
static TickFields tick_block(uint8_t* h, const TickLayout& tl)
{
  TickFields b{};
  b.h = h;
  b.px = reinterpret_cast<float*>(h + tl.px);
  b.py = reinterpret_cast<float*>(h + tl.py);
  b.pyaw = reinterpret_cast<float*>(h + tl.pyaw);
  b.D = reinterpret_cast<float*>(h + tl.D);
  b.pf_idx = reinterpret_cast<uint32_t*>(h + tl.pf_idx);
  b.pvalid = h + tl.pvalid;
  b.pa_active = h + tl.pa_active;
  b.pang_active = h + tl.pang_active;
  b.pal_active = h + tl.pal_active;
  b.lut_cost = reinterpret_cast<float*>(h + tl.lut_cost);
  b.prune = reinterpret_cast<float*>(h + tl.prune);
  return b;
}

// the control sequence (vy row zeroed for a non-holonomic model) and the plan into the tick block
static void copy_plan(const TickFields& b, const TickLayout& tl, const smpc_tick_in* in, const float* u_in, uint32_t T,
                      bool holonomic)
{
  const uint32_t P = in->path_len;
  uint8_t* h = b.h;
  memcpy(h + tl.u, u_in, 3 * T * sizeof(float));
  if (!holonomic) memset(h + tl.u + T * sizeof(float), 0, T * sizeof(float));
  if (P) {
    memcpy(b.px, in->path_x, P * 4);
    memcpy(b.py, in->path_y, P * 4);
    memcpy(b.pyaw, in->path_yaw, P * 4);
  }
}

// the robot's state as the kernels take it, the first rollout point and the cost under it
struct FirstPoint {
  float yaw0, cos0, sin0, svx, svy, swz, x00, y00;
  uint32_t cost_t0;
};
static FirstPoint first_point(const smpc_tick_in* in, bool holonomic, float dt, const HostCostmap& map)
{
  const float yaw0 = in->pose_yaw;
  const float cos0 = cosf(yaw0), sin0 = sinf(yaw0);
  const float svx = static_cast<float>(in->speed_vx);
  // state.vy[:,0] = speed.linear.y only if holonomic (optimizer.cpp:264-266)
  const float svy = holonomic ? static_cast<float>(in->speed_vy) : 0.f;
  const float swz = static_cast<float>(in->speed_wz);
  // trajectories(0,0): first rollout point, identical for every rollout because
  // v[:,0] is the measured speed (optimizer.cpp:258-267,331-342)
  const float dx0 = svx * cos0 - svy * sin0;
  const float dy0 = svx * sin0 + svy * cos0;
  const float x00 = static_cast<float>(in->pose_x + static_cast<double>(dx0 * dt));
  const float y00 = static_cast<float>(in->pose_y + static_cast<double>(dy0 * dt));
  uint32_t cost_t0 = SMPC_COST_NO_INFORMATION;   // costAtPose of that point (obstacles_critic.cpp:203-212)
  if (map.set) {
    unsigned mx, my;
    if (world_to_map(map, x00, y00, mx, my))
      cost_t0 = map.cells.get()[static_cast<size_t>(my) * map.W + mx];
  }
  return FirstPoint{yaw0, cos0, sin0, svx, svy, swz, x00, y00, cost_t0};
}

// ---- per-candidate-furthest-point tables -------------------------------------

// PathAlignCritic's and PathAlignLegacyCritic's gate per candidate furthest point S
// (path_align_critic.cpp:58-74, path_align_legacy_critic.cpp:56-72: the same code)
static void occupancy_gate(const float* px, const float* py, const uint8_t* pvalid, uint32_t P, float x00, float y00,
                           const smpc_path_align_params& q, uint8_t* active)
{
  // utils::findPathTrajectoryInitialPoint (tools/utils.hpp:327-344)
  size_t init = 0;
  float best = std::numeric_limits<float>::max();
  for (uint32_t j = 0; j < P; ++j) {
    const float ddx = px[j] - x00, ddy = py[j] - y00;
    const float d = ddx * ddx + ddy * ddy;
    if (d < best) {
      best = d;
      init = j;
    }
  }
  // occupancy of the path between the initial and the furthest point.  The reference
  // walks i = init..S-1 with a running count of invalid points and stops at the first i where
  // count / range > ratio and count > 2; the count only grows and range is fixed per S, so
  // that happens iff it holds for the final count: prefix sums, O(P).
  std::vector<uint32_t> inval(P + 1, 0);
  for (uint32_t i = 0; i < P; ++i) inval[i + 1] = inval[i] + ((i + 1 < P && !pvalid[i]) ? 1u : 0u);
  for (uint32_t S = 0; S < P; ++S) {
    bool on = S >= q.offset_from_furthest;
    if (on && S > init) {
      const unsigned int invalid_ctr = inval[S] - inval[init];
      const float range = static_cast<float>(static_cast<size_t>(S) - init);
      if (static_cast<float>(invalid_ctr) / range > q.max_path_occupancy_ratio && invalid_ctr > 2) on = false;
    }
    active[S] = on ? 1 : 0;
  }
}

// PathFollowCritic's target point per candidate furthest point S
static void path_follow_targets(const uint8_t* pvalid, uint32_t P, uint32_t offset_from_furthest, uint32_t* pf_idx)
{
  // path_follow_critic.cpp:46-57
  const size_t path_size = P - 1;
  for (uint32_t S = 0; S < P; ++S) {
    size_t idx = std::min(static_cast<size_t>(S) + offset_from_furthest, path_size);
    bool valid = false;
    while (!valid && idx < path_size - 1) {
      valid = pvalid[idx];
      if (!valid) idx++;
    }
    pf_idx[S] = static_cast<uint32_t>(idx);
  }
}

// PathAngleCritic per candidate furthest point S: pang_active[S] = 1 where the critic is live (the
// angle to the offset point is not inside max_angle_to_furthest)
struct PathAngleGates {
  bool any_live;   // live for some S: the lane pass cannot take the tick (lane_eligible)
  bool correct;    // SmpcDev::pang_correct
};
static PathAngleGates path_angle_gates(const float* px, const float* py, uint32_t P, const smpc_tick_in* in,
                                       const smpc_path_angle_params& q, uint8_t* pang_active)
{
  const double rx = in->pose_x, ry = in->pose_y;
  bool pang_correct = false, pang_any = false;
  // path_angle_critic.cpp:24-31,52-54: reversing / forward preference
  bool reversing_allowed = true;
  if (std::fabs(q.vx_min) < 1e-6) reversing_allowed = false;
  else if (q.vx_min < 0.0f) reversing_allowed = true;
  bool forward_preference = q.forward_preference != 0;
  if (!reversing_allowed) forward_preference = true;
  pang_correct = reversing_allowed && !forward_preference;
  for (uint32_t S = 0; S < P; ++S) {
    // :73-83 utils::posePointAngle (tools/utils.hpp:417-434) against the offset point
    const size_t idx = std::min(static_cast<size_t>(S) + q.offset_from_furthest,
                                static_cast<size_t>(P) - 1);
    const float pose_x = static_cast<float>(rx), pose_y = static_cast<float>(ry);
    const double point_x = px[idx], point_y = py[idx];
    const float yaw = atan2f(static_cast<float>(point_y - static_cast<double>(pose_y)),
                             static_cast<float>(point_x - static_cast<double>(pose_x)));
    auto norm = [](double a) {
      const double theta = std::fmod(a + M_PI, 2.0 * M_PI);
      return theta <= 0.0 ? theta + M_PI : theta - M_PI;
    };
    const double pyaw0 = static_cast<double>(in->pose_yaw);
    float ang = static_cast<float>(std::fabs(norm(pyaw0 - static_cast<double>(yaw))));
    if (!forward_preference) {
      const double b = std::fabs(norm(norm(pyaw0 + M_PI) - static_cast<double>(yaw)));
      ang = static_cast<float>(std::min(std::fabs(norm(pyaw0 - static_cast<double>(yaw))), b));
    }
    pang_active[S] = ang < q.max_angle_to_furthest ? 0 : 1;
    if (pang_active[S]) pang_any = true;
  }
  return PathAngleGates{pang_any, pang_correct};
}

// CostCritic's term per 8-bit cost
static void cost_lut(const smpc_cost_params& q, bool near_goal_c, float* lut_cost)
{
  // cost_critic.cpp:120-124,141-155 per 8-bit cost (collisions are marked in the shared LUT)
  for (int v = 0; v < 256; ++v) {
    float t = 0.0f;
    if (v >= 1) {
      if (static_cast<float>(v) >= static_cast<float>(SMPC_COST_INSCRIBED)) t = q.critical_cost;
      else if (!near_goal_c) t = static_cast<float>(v);
    }
    lut_cost[v] = t;
  }
}

// {Obstacles,Cost}Critic::findCircumscribedCost with InflationLayer::computeCost
// (nav2_costmap_2d, Humble): the cost at the circumscribed radius, -1 without a layer
float circumscribed_cost(const HostCostmap& map, double fp_circumscribed_radius, double fp_layer_scale)
{
  double result = -1.0;
  if (fp_layer_scale >= 0.0) {
    const double distance = fp_circumscribed_radius / map.res;
    unsigned char cost = 0;
    if (distance == 0) {
      cost = SMPC_COST_LETHAL;
    } else if (distance * map.res <= static_cast<double>(map.inscribed_radius)) {
      cost = SMPC_COST_INSCRIBED;
    } else {
      const double factor = std::exp(-1.0 * fp_layer_scale *
                                     (distance * map.res - static_cast<double>(map.inscribed_radius)));
      cost = static_cast<unsigned char>((SMPC_COST_INSCRIBED - 1) * factor);
    }
    result = cost;
  }
  return static_cast<float>(result);
}

// ---- Obstacles LUT: rebuilt and uploaded only when its inputs changed -----------
static int upload_collision_luts(smpc_ctx* c, const smpc_tick_in* in, uint32_t gates, bool near_goal_cost,
                                 const float* lut_cost)
{
  const auto& cr = c->critics;
  const double rx = in->pose_x, ry = in->pose_y, gx = in->goal_x, gy = in->goal_y;
  if (gates & (SD_OBSTACLES | SD_COST)) {
    const bool near_goal = within_tol(cr.obstacles.near_goal_distance, rx, ry, gx, gy);  // :124-127
    const bool cost_only = (gates & SD_COST) && !(gates & SD_OBSTACLES) && !(gates & (SD_FP_OBSTACLES | SD_FP_COST));
    const uint64_t key = (c->map_version << 20) ^ (c->critics_version << 4) ^ (near_goal ? 1u : 0u) ^
      ((gates & (SD_FP_OBSTACLES | SD_FP_COST)) ? 2u : 0u) ^ (cost_only ? 4u : 0u) ^ (near_goal_cost ? 8u : 0u);
    if (!c->lut_valid || key != c->lut_key) {
      build_lut(c->map, cr.obstacles, near_goal, c->h_lut.get(), false, false, cost_only ? lut_cost : nullptr);
      HIPCK(c, hipMemcpyAsync(c->d_lut.get(), c->h_lut.get(), 256 * sizeof(SmpcLut), hipMemcpyHostToDevice,
                              c->stream));
      if (gates & (SD_FP_OBSTACLES | SD_FP_COST)) {
        build_lut(c->map, cr.obstacles, near_goal, c->h_lut_fp.get(), true, false);
        build_lut(c->map, cr.obstacles, near_goal, c->h_lut_fp.get() + 256, true, true);
        HIPCK(c, hipMemcpyAsync(c->d_lut_fp.get(), c->h_lut_fp.get(), 512 * sizeof(SmpcLut), hipMemcpyHostToDevice,
                                c->stream));
      }
      c->lut_key = key;
      c->lut_valid = true;
    }
  }
  return SMPC_OK;
}

// The index this tick is first scored with (it does not depend on the launch plan), and the lane
// pass's prune table for the 16 indices around it: the batch's furthest point — what the table is
// indexed with — lands within one or two of the prediction.  O(16 P), ~0.5 us for 60 points, so:
// only where it is read — a speculating tick of a context whose LAST tick took the parking form of
// the lane pass on its own (this tick's plan is made after the block has gone to the device; a
// wrong guess costs scans or a table nobody reads, never a result) — once per plan and first index
// (a plan is handed over unchanged for several ticks), and not beyond kPruneMaxPath points.
// SMPC_FURTHEST_PRUNE=0 gets the empty table, every entry "never prune" (the same work in the
// kernel: the A/B switch); a tick that does not read the table gets only its header with no
// entries (a pass that reads it after all scans every group), and the block handed to the device
// ends behind that header: 512 bytes less through the BAR on every small tick.
// Runs after predict_hint (it reads the hint) and before plan_launch: c->plan is still the
// PREVIOUS tick's.  Returns the bytes of the block to hand over.
static size_t prune_table_for_tick(smpc_ctx* c, const TickFields& b, const TickLayout& tl, uint32_t P)
{
  const float* px = b.px;
  const float* py = b.py;
  size_t tick_bytes = tl.total;
  constexpr uint32_t kPruneMaxPath = 256;
  float* table = b.prune;
  uint32_t k0 = (c->pred.hint_valid && c->pred.hint > SMPC_PRUNE_ENTRIES / 2) ? c->pred.hint - SMPC_PRUNE_ENTRIES / 2 : 0u;
  k0 = std::min(k0, P > SMPC_PRUNE_ENTRIES ? P - SMPC_PRUNE_ENTRIES : 0u);
  const bool read = c->plan.kind == PassPlan::kLane && !c->plan.rr && !c->plan.pow && !c->in_group && c->pred.hint_valid &&
    !(c->cfg.flags & SMPC_FLAG_NO_SPECULATION);
  if (!read || P > kPruneMaxPath) {
    memset(table, 0, 16);
    tick_bytes = tl.prune + 16;
  } else if (!c->knobs.furthest_prune) {
    build_prune_table(px, py, P, k0, false, table);
  } else if (c->prune_k0 == k0 && c->prune_px.size() == P && !memcmp(c->prune_px.data(), px, P * 4) &&
             !memcmp(c->prune_py.data(), py, P * 4)) {
    memcpy(table, c->prune_table, sizeof(c->prune_table));
  } else {
    build_prune_table(px, py, P, k0, true, table);
    memcpy(c->prune_table, table, sizeof(c->prune_table));
    c->prune_px.assign(px, px + P);
    c->prune_py.assign(py, py + P);
    c->prune_k0 = k0;
  }
  return tick_bytes;
}

// how the kernels get the tick block: the base address they read it from, or inside their arguments
struct HandOver {
  const uint8_t* base;   // pinned host memory (SMPC_PINNED_TICK=1) or c->tick.d_tick
  bool inline_tick;
};
// The tick's number and canary, then the block to the device: CPU stores through the BAR, a copy
// on the stream, inside the kernel arguments (fill_dev_footprint_inline), read in place from pinned
// memory, or left to the group (defer_upload).  tick_no advances here, so also for a tick whose
// planning fails afterwards.
static int hand_over_tick_block(smpc_ctx* c, uint32_t gates, const TickLayout& tl, size_t tick_bytes, HandOver& ho)
{
  const uint32_t T = c->cfg.time_steps;
  uint8_t* h = c->tick.h_tick;
  // small ticks travel inside the kernel arguments (SmpcDev::tick_bytes) instead of a copy of
  // their own; the CostCritic table (general pass only) is not part of that
  // (contexts of the wave-per-rollout pass only: see smpc_lane.hip for why not the other)
  const bool inline_tick = !c->defer_upload && !c->noise.use_tpr && T <= 64 && tl.lut_cost - tl.px <= SMPC_INLINE_TICK_CAP &&
    !c->knobs.no_inline_tick;
  // SMPC_PINNED_TICK=1 (experiment): no copy at all — the kernels read the tick block where the
  // host assembled it, in pinned host memory.  Measured (tools/tail_ab.py SMPC_PINNED_TICK=1) and
  // not the default: every block of the grid fetches its ~2 KB across PCIe, uncached.
  const bool pinned_tick = c->knobs.pinned_tick && !c->defer_upload && !inline_tick;
  const uint8_t* const tb = pinned_tick ? h : c->tick.d_tick;
  // the tick block's number: written last, echoed by block 0 of every pass that reads the block
  // from device memory (SmpcDev::canary)
  if (++c->tick.no == 0) ++c->tick.no;
  *reinterpret_cast<uint32_t*>(h + tl.canary) = c->tick.no;
  c->tick.used = tick_bytes;
  const bool bar = c->tick.bar_tick && !c->defer_upload && !pinned_tick && !inline_tick;
  // (whoever uploads: this ctx or its group; the in-launch reduction experiment does not carry it)
  c->tick.canary_expect = (!pinned_tick && !inline_tick && !c->knobs.fused_reduce) ? c->tick.no : 0u;
  if (bar) {
    // no kernel of an earlier tick may still read the block (every tick ends with fetch_out;
    // a tick abandoned on an error does not)
    if (c->launched) {
      HIPCK(c, hipStreamSynchronize(c->stream));
      c->launched = false;
    }
    // SMPC_DEBUG_STALE_TICK=n (tests of the guard): tick n's block is NOT handed over — the pass
    // reads the previous tick's, echoes its number, and fetch_out has to fail the tick
    if (c->knobs.stale_tick && c->tick.no == c->knobs.stale_tick) {
    } else {
      bar_copy(c->tick.d_tick, h, tick_bytes);
      bar_flush(c);
    }
  } else if (!c->defer_upload && !pinned_tick) {
    if (!inline_tick)
      HIPCK(c, hipMemcpyAsync(c->tick.d_tick, h, tick_bytes, hipMemcpyHostToDevice, c->stream));
    else if (gates & SD_COST)
      HIPCK(c, hipMemcpyAsync(c->tick.d_tick + tl.lut_cost, h + tl.lut_cost, 256 * sizeof(float), hipMemcpyHostToDevice,
                              c->stream));
  }
  ho.base = tb;
  ho.inline_tick = inline_tick;
  return SMPC_OK;
}

// ---- kernel parameter block ------------------------------------------------------

// c->dev zeroed, then the tick's sizes, the robot's state, the tensors, the costmap with the wave
// pass's cell-index guard band, and the tick block's regions at the base the kernels read
static void fill_dev_state(smpc_ctx* c, const smpc_tick_in* in, uint32_t nsamp, uint32_t step, const FirstPoint& fp,
                           const TickLayout& tl, const uint8_t* tb)
{
  const uint32_t T = c->cfg.time_steps, B = c->cfg.batch_size, P = in->path_len;
  SmpcDev& d = c->dev;
  memset(&d, 0, sizeof(d));
  d.B = B; d.T = T; d.P = P; d.nsamp = nsamp; d.step = step;
  d.x0 = in->pose_x; d.y0 = in->pose_y;
  d.yaw0 = fp.yaw0; d.cos0 = fp.cos0; d.sin0 = fp.sin0;
  d.svx = fp.svx; d.svy = fp.svy; d.swz = fp.swz; d.dt = c->cfg.model_dt;
  d.nvx = c->noise.cur.nvx.get(); d.nvy = c->noise.cur.nvy.get(); d.nwz = c->noise.cur.nwz.get();
  d.tvx = c->noise.cur.tvx.get(); d.tvy = c->noise.cur.tvy; d.twz = c->noise.cur.twz;
  d.u = reinterpret_cast<const float*>(tb + tl.u);
  d.traj_x = c->d_traj[0].get(); d.traj_y = c->d_traj[1].get(); d.traj_yaw = c->d_traj[2].get();
  d.map = c->d_map.get(); d.W = c->map.W; d.H = c->map.H;
  d.ox = c->map.ox; d.oy = c->map.oy; d.res = c->map.res;
  d.cost_t0 = fp.cost_t0;
  d.x00f = fp.x00; d.y00f = fp.y00;
  {
    // fast cell index: float quotient + guard band (see cost_at in smpc_kernels.hip)
    const double rinv = 1.0 / c->map.res;
    d.oxf = static_cast<float>(c->map.ox);
    d.oyf = static_cast<float>(c->map.oy);
    d.rinvf = static_cast<float>(rinv);
    const double e_o = std::max(std::fabs(c->map.ox - static_cast<double>(d.oxf)),
                                std::fabs(c->map.oy - static_cast<double>(d.oyf)));
    const double qmax = static_cast<double>(std::max(c->map.W, c->map.H)) + 2.0;
    const double eps = 2.0 * (e_o * rinv + 3.1 * 5.9604644775390625e-08 * qmax) + 1e-7;
    d.cell_eps = static_cast<float>(std::min(eps, 0.5));
  }
  d.lut = c->d_lut.get();
  d.px = reinterpret_cast<const float*>(tb + tl.px);
  d.py = reinterpret_cast<const float*>(tb + tl.py);
  d.pyaw = reinterpret_cast<const float*>(tb + tl.pyaw);
  d.D = reinterpret_cast<const float*>(tb + tl.D);
  d.pvalid = tb + tl.pvalid;
  d.pa_active = tb + tl.pa_active;
  d.pf_idx = reinterpret_cast<const uint32_t*>(tb + tl.pf_idx);
  d.prune = reinterpret_cast<const float*>(tb + tl.prune);
  d.lut_cost = reinterpret_cast<const float*>(tb + tl.lut_cost);
  d.pang_active = tb + tl.pang_active;
  d.pal_active = tb + tl.pal_active;
  d.timeline = c->d_timeline.get();
  d.canary_echo = c->tick.canary_expect ? 1u : 0u;
  d.partials = c->d_partials.get();
  d.furthest_out = reinterpret_cast<uint32_t*>(c->d_furthest.get());
}

// the critics' parameters as the kernels take them, and the optimizer's (gamma terms, temperature)
static void fill_dev_critics(smpc_ctx* c, const smpc_tick_in* in, const float* pyaw, bool near_goal_cost,
                             bool pang_correct)
{
  const uint32_t T = c->cfg.time_steps, P = in->path_len;
  const auto& cr = c->critics;
  SmpcDev& d = c->dev;
  d.obs_critical_w = cr.obstacles.critical_weight;
  d.obs_repulsion_w = cr.obstacles.repulsion_weight;
  d.obs_collision_cost = cr.obstacles.collision_cost;
  d.obs_rep_over_T = cr.obstacles.repulsion_weight / static_cast<float>(T);
  d.obs_power = cr.obstacles.cost_power;
  d.pa_weight = cr.path_align.cost_weight; d.pa_power = cr.path_align.cost_power;
  d.pf_weight = cr.path_follow.cost_weight; d.pf_power = cr.path_follow.cost_power;
  d.ga_weight = cr.goal_angle.cost_weight; d.ga_power = cr.goal_angle.cost_power;
  d.ga_goal_yaw = P ? pyaw[P - 1] : 0.f;
  d.pfw_weight = cr.prefer_forward.cost_weight; d.pfw_power = cr.prefer_forward.cost_power;
  d.con_weight = cr.constraint.cost_weight; d.con_power = cr.constraint.cost_power;
  {
    // ConstraintCritic::initialize (constraint_critic.cpp:36-38)
    const float min_sgn = cr.constraint.vx_min > 0.0f ? 1.0f : -1.0f;
    d.con_max_vel = sqrtf(cr.constraint.vx_max * cr.constraint.vx_max + cr.constraint.vy_max * cr.constraint.vy_max);
    d.con_min_vel = min_sgn * sqrtf(cr.constraint.vx_min * cr.constraint.vx_min + cr.constraint.vy_max * cr.constraint.vy_max);
    d.con_acker_r = c->acker_r;
  }
  d.cost_w254 = cr.cost.cost_weight / 254.0f;   // cost_critic.cpp:34
  d.cost_collision_cost = cr.cost.collision_cost; d.cost_power = cr.cost.cost_power;
  d.cost_critical = cr.cost.critical_cost;
  d.cost_near_goal = near_goal_cost ? 1u : 0u;
  d.goal_x = in->goal_x; d.goal_y = in->goal_y;
  d.goal_weight = cr.goal.cost_weight; d.goal_power = cr.goal.cost_power;
  d.tw_weight = cr.twirling.cost_weight; d.tw_power = cr.twirling.cost_power;
  d.pal_weight = cr.path_align_legacy.cost_weight;
  d.pal_power = cr.path_align_legacy.cost_power;
  {
    const uint32_t lstep = cr.path_align_legacy.trajectory_point_step;
    d.pal_eval = lstep ? static_cast<float>(T / lstep) : 0.f;   // traj_pts_eval = floor(T / step) (:83)
  }
  d.pang_weight = cr.path_angle.cost_weight; d.pang_power = cr.path_angle.cost_power;
  d.pang_offset = cr.path_angle.offset_from_furthest; d.pang_correct = pang_correct ? 1 : 0;
  d.db_vx = std::fabs(static_cast<double>(cr.velocity_deadband.deadband_velocities[0]));
  // no vy term for a non-holonomic model (velocity_deadband_critic.cpp:78-97); with
  // state.vy = 0 a zero deadband contributes max(0 - 0, 0) = 0
  d.db_vy = c->holonomic ? std::fabs(static_cast<double>(cr.velocity_deadband.deadband_velocities[1])) : 0.0;
  d.db_wz = std::fabs(static_cast<double>(cr.velocity_deadband.deadband_velocities[2]));
  d.db_weight = cr.velocity_deadband.cost_weight; d.db_power = cr.velocity_deadband.cost_power;
  d.g_vx = c->cfg.gamma / powf(c->cfg.vx_std, 2);
  d.g_vy = c->holonomic ? c->cfg.gamma / powf(c->cfg.vy_std, 2) : 0.f;   // optimizer.cpp:374-380
  d.g_wz = c->cfg.gamma / powf(c->cfg.wz_std, 2);
  d.neg_inv_temp = -1 / c->cfg.temperature;
  d.k2 = d.neg_inv_temp * 1.4426950408889634f;
}

// the footprint and its circumscribed cost; for an inline tick the control sequence and the path
// block inside the arguments
static void fill_dev_footprint_inline(smpc_ctx* c, uint32_t gates, const TickLayout& tl, bool inline_tick)
{
  const uint32_t T = c->cfg.time_steps;
  const uint8_t* h = c->tick.h_tick;
  SmpcDev& d = c->dev;
  d.lut_fp = c->d_lut_fp.get();
  d.fp_n = static_cast<uint32_t>(c->fp_x.size());
  for (uint32_t i = 0; i < d.fp_n; ++i) {
    d.fp_x[i] = c->fp_x[i];
    d.fp_y[i] = c->fp_y[i];
  }
  d.fp_pic = 0.0f;
  if (gates & (SD_FP_OBSTACLES | SD_FP_COST))
    d.fp_pic = circumscribed_cost(c->map, c->fp_circumscribed_radius, c->fp_layer_scale);
  // (u_arg: copied from the block, after copy_plan zeroed the vy row of a non-holonomic model)
  if (inline_tick) memcpy(d.u_arg, h + tl.u, 3 * T * sizeof(float));
  if (inline_tick) {
    d.tick_inline = 1;
    d.u_inline = 1;
    const size_t o = tl.px;   // the path block: everything between u and the CostCritic table
    d.io_px = static_cast<uint16_t>(tl.px - o); d.io_py = static_cast<uint16_t>(tl.py - o);
    d.io_pyaw = static_cast<uint16_t>(tl.pyaw - o); d.io_D = static_cast<uint16_t>(tl.D - o);
    d.io_pf_idx = static_cast<uint16_t>(tl.pf_idx - o); d.io_pvalid = static_cast<uint16_t>(tl.pvalid - o);
    d.io_pa_active = static_cast<uint16_t>(tl.pa_active - o); d.io_pang_active = static_cast<uint16_t>(tl.pang_active - o);
    d.io_pal_active = static_cast<uint16_t>(tl.pal_active - o);
    memcpy(d.tick_bytes, h + o, tl.lut_cost - o);
  }
}

// Everything the reference's critics decide once per tick on the host, plus the
// upload of the tick block.  Leaves c->dev ready for the launches.
int prepare_tick(smpc_ctx* c, const smpc_tick_in* in, const float* u_in)
{
  int rc = check_tick(c, in);
  if (rc != SMPC_OK) return rc;
  if (!u_in) return fail(c, SMPC_ERR_INVALID, "control sequence missing");
  rc = absorb_redraw(c);   // noise drawn in the background since the last tick, if any
  if (rc != SMPC_OK) return rc;
  const uint32_t T = c->cfg.time_steps, P = in->path_len;
  const auto& cr = c->critics;
  HIPCK(c, hipSetDevice(c->device));

  const TickLayout tl = tick_layout(T, std::max(P, 1u));
  if (tl.total > c->tick.cap) return fail(c, SMPC_ERR_INVALID, "tick block overflow");
  const TickFields b = tick_block(c->tick.h_tick, tl);
  copy_plan(b, tl, in, u_in, T, c->holonomic);

  uint32_t gates = 0, nsamp = 0;
  rc = tick_gates(c, in, gates, nsamp);
  if (rc != SMPC_OK) return rc;
  const double rx = in->pose_x, ry = in->pose_y, gx = in->goal_x, gy = in->goal_y;
  // (PathAlignLegacy alone: its own step — tick_gates refuses two different ones)
  const uint32_t step = (gates & SD_PATH_ALIGN) || !(gates & SD_PATH_ALIGN_LEGACY) ? cr.path_align.trajectory_point_step
                                                                                    : cr.path_align_legacy.trajectory_point_step;
  path_tables(c->map, in, gates, b.px, b.py, b.pvalid, b.D);
  const FirstPoint fp = first_point(in, c->holonomic, c->cfg.model_dt, c->map);

  // the per-candidate-furthest-point tables; a critic past its gate gets its table, the others zeros
  const uint32_t P1 = std::max(P, 1u);
  if (gates & SD_PATH_ALIGN) occupancy_gate(b.px, b.py, b.pvalid, P, fp.x00, fp.y00, cr.path_align, b.pa_active);
  else memset(b.pa_active, 0, P1);
  if (gates & SD_PATH_ALIGN_LEGACY) occupancy_gate(b.px, b.py, b.pvalid, P, fp.x00, fp.y00, cr.path_align_legacy, b.pal_active);
  else memset(b.pal_active, 0, P1);
  if (gates & SD_PATH_FOLLOW) path_follow_targets(b.pvalid, P, cr.path_follow.offset_from_furthest, b.pf_idx);
  else memset(b.pf_idx, 0, P1 * 4);
  // (c->pang_any: cleared here for every tick, read by plan_launch below)
  PathAngleGates pang{false, false};
  if (gates & SD_PATH_ANGLE) pang = path_angle_gates(b.px, b.py, P, in, cr.path_angle, b.pang_active);
  else memset(b.pang_active, 0, P1);
  c->pang_any = pang.any_live;
  const bool near_goal_cost = (gates & SD_COST) && within_tol(cr.cost.near_goal_distance, rx, ry, gx, gy);
  if (gates & SD_COST) cost_lut(cr.cost, near_goal_cost, b.lut_cost);
  else memset(b.lut_cost, 0, 256 * 4);

  // the LUT upload is enqueued before the wait on the map upload
  rc = upload_collision_luts(c, in, gates, near_goal_cost, b.lut_cost);
  if (rc != SMPC_OK) return rc;
  rc = wait_map_upload(c);
  if (rc != SMPC_OK) return rc;
  // after wait_map_upload and before the prune table, which is indexed around the hint; the prune
  // table before plan_launch, which overwrites the c->plan of the previous tick it looks at
  predict_hint(c, in, u_in);
  const size_t tick_bytes = prune_table_for_tick(c, b, tl, P);
  // (the profile's first event: between the prune table and the hand-over)
  if (c->cfg.flags & SMPC_FLAG_PROFILE) HIPCK(c, hipEventRecord(c->ev0.get(), c->stream));
  HandOver ho{};
  rc = hand_over_tick_block(c, gates, tl, tick_bytes, ho);
  if (rc != SMPC_OK) return rc;

  // c->dev is zeroed and filled before plan_launch, which writes the window, wxf / cxf and
  // cell_eps_w into it
  fill_dev_state(c, in, nsamp, step, fp, tl, ho.base);
  fill_dev_critics(c, in, b.pyaw, near_goal_cost, pang.correct);
  fill_dev_footprint_inline(c, gates, tl, ho.inline_tick);
  int mode_now = 0;
  rc = plan_launch(c, in, gates, nsamp, mode_now);
  if (rc != SMPC_OK) return rc;

  // written only after everything succeeded
  c->gate_flags = gates;
  // with a footprint the two collision critics no longer see the same set of colliding rollouts,
  // and a pass reports one non-colliding count (CostCritic's, scored first): smpc_optimize counts
  // ObstaclesCritic's with a pass of its own; the sharded tick and the grouped launch do not
  c->two_coll_fp = (gates & SD_OBSTACLES) && (gates & SD_COST) && (gates & (SD_FP_OBSTACLES | SD_FP_COST));
  c->score_mode = mode_now;
  c->fail_in = in->fail_flag_in != 0;
  c->P = P;
  c->tick_ready = true;
  begin_limit_iteration(c, nullptr);   // iteration 0 limits against the uploaded u
  return SMPC_OK;
}

}  // namespace smpc_impl
