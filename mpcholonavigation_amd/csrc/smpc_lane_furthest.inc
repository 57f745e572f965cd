// smpc_lane_furthest.inc — the furthest-point section of the lane pass's group body (lane = rollout,
// x and y hold the rollout's endpoint).  Included by smpc_lane_pass.inc at one of two places, with
// LANE_FURTHEST_PRUNE defined:
//   false  in front of the per-rollout costs, every group scans (the GoalAngle, deployed-list,
//          grouped, re-read and cost-power instances: they have no registers for anything else);
//   true   at the END of the group body, behind the wz walk, where the parked registers are dead,
//          with the prune test in front of the scan (the plain instances).
// One text, included twice, and not a lambda: lambdas have spilled here before.
    // nearest path point of the endpoint (utils.hpp:292-319): first minimum wins
    if (want_local_furthest) {
      // Only the batch-wide MAXIMUM of F over the live rollouts is consumed, and after a wave's first
      // group nearly every rollout is below a value already attained.  theta is such a value: the
      // larger of this wave's F_local and one LDS word that holds the largest m a wave of this block
      // has formed so far (zeroed by the staging, raised with an LDS atomic maximum on the float's
      // bits — F >= 0, so the bit order is the float order — and read with a plain load: a stale value
      // is a weaker bound, never a wrong one).  Both are F values of live rollouts that went through
      // the scan, so theta <= the true maximum and leaving out rollouts with F <= theta cannot
      // change it.  The per-lane test "F <= theta" against the host's table entry for K = rint(theta)
      // is derived, with its margins, at build_prune_table (smpc_prepare.cpp); a group none of whose
      // live lanes fails it skips the scan altogether.  K outside the table: the group scans.
      //
      // A wave's FIRST group has no bound: the eight waves of a block start together and reach this
      // point within a microsecond of each other.  So only wave 0 scans its first group; every other
      // wave that has a second group to come leaves its first group's endpoints in the four unused
      // floats at the end of its parked-wz rows (LANE_PARK_STRIDE 68) and judges them behind its
      // second group, one group-time later, when wave 0's maximum is in the block's word: the loop
      // below then runs twice, the second time on the endpoints left behind (a first group that
      // another follows is a full one: all 64 lanes live).
      int reps = 1;
      if constexpr (LANE_FURTHEST_PRUNE) {
        if (furthest_pending) {
          reps = 2;
        } else if (wave != 0 && grp == gw && grp + nW < ngroups &&
                   __builtin_amdgcn_readfirstlane((int)__float_as_uint(fmaxf(F_local, s_prune[2]))) == 0) {
          park[lane * LANE_PARK_STRIDE + 64] = x;
          park[lane * LANE_PARK_STRIDE + 65] = y;
          furthest_pending = true;
          reps = 0;
        }
      }
      for (int rep = 0; rep < reps; ++rep) {
      bool flive = live;
      if constexpr (LANE_FURTHEST_PRUNE) {
        if (rep == 1) {
          x = park[lane * LANE_PARK_STRIDE + 64];
          y = park[lane * LANE_PARK_STRIDE + 65];
          flive = true;
          furthest_pending = false;
        }
      }
      bool scan = true;
      if constexpr (LANE_FURTHEST_PRUNE) {
        const uint32_t* s_prune_u = reinterpret_cast<const uint32_t*>(s_prune);
        const float theta = __uint_as_float((uint32_t)__builtin_amdgcn_readfirstlane(
            (int)__float_as_uint(fmaxf(F_local, s_prune[2]))));
        const float Kf = rintf(theta);
        const uint32_t ent = (uint32_t)(int)Kf - s_prune_u[0];
        bool may_raise = flive;
        if (ent < s_prune_u[1]) {
          const f32x4 ea = reinterpret_cast<const f32x4*>(s_prune + 4)[2 * ent];
          const f32x4 eb = reinterpret_cast<const f32x4*>(s_prune + 4)[2 * ent + 1];
          const float ex = x - ea[0], ey = y - ea[1];
          const float ps = ea[2] * ex + ea[3] * ey, pt = ea[2] * ey - ea[3] * ex;
          // (every compare is false for a NaN: such a lane scans)
          const bool prunable = (fmaxf(fabsf(ps), fabsf(pt)) <= 1.0f) && (ps + eb[0] * fabsf(pt) <= eb[1]) &&
                                (Kf + fmaxf(ps * eb[2] + eb[3], -0.45f) <= theta);
          may_raise = flive && !prunable;
        }
        scan = __any(may_raise);
      }
      if (scan) {
      // Four path points per pair of LDS broadcast reads (the arrays are padded to a multiple
      // of four with far-away points that never win).  The strict "<" scan runs over the
      // MINIMUM of each block of four — the first block that holds the overall minimum wins —
      // and the first point of that block that attains it is found afterwards, from the same
      // arithmetic: the reference's first minimum at a third of the compare/select work.
      auto block_d2 = [&](const float* bx, const float* by, float (&dd)[4]) {
        const f32x4 qx = *reinterpret_cast<const f32x4*>(bx);
        const f32x4 qy = *reinterpret_cast<const f32x4*>(by);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float ex = qx[e] - x, ey = qy[e] - y;
          dd[e] = ex * ex + ey * ey;
        }
      };
      float best = 3.4028234663852886e38f;
      uint32_t bj = 0;
      const uint32_t P4 = (p.P + 3u) & ~3u;
      // The scan is 15 blocks for a 60-point path and only its batch-wide MAXIMUM is consumed.  So
      // it starts three blocks below the block of the index this tick is scored with (where the
      // maximum has been every tick so far) and runs to the path's end; what that leaves out is
      // checked for the ONE lane that ends up holding the wave's maximum (below).  (The plain
      // instances only: in the GoalAngle, deployed-list and grouped ones the extra code costs
      // 16-48 bytes of scratch.)
      constexpr bool kWindow = !GA && !DEP && !MANY;
      const uint32_t j_lo = (kWindow && (S >> 2) > 3u) ? ((S >> 2) - 3u) << 2 : 0u;
      for (uint32_t j = j_lo; j < P4; j += 4) {
        float dd[4];
        block_d2(s_px + j, s_py + j, dd);
        const float mn = fminf(fminf(dd[0], dd[1]), fminf(dd[2], dd[3]));
        if (mn < best) {      // a NaN or infinite distance never wins, as in the plain scan
          best = mn;
          bj = j;
        }
      }
      // index + how far the endpoint sits towards the next point, in segment lengths (what the
      // host predicts the next tick's index from; smpc_dev.h)
      auto point_F = [&]() -> float {
        float dd[4];
        block_d2(s_px + bj, s_py + bj, dd);
        const uint32_t bi = bj + (dd[0] == best ? 0u : dd[1] == best ? 1u : dd[2] == best ? 2u : dd[3] == best ? 3u : 0u);
        float F = (float)bi;
        if (bi + 1 < p.P) {
          const float nx = s_px[bi + 1], ny = s_py[bi + 1];
          const float sgx = nx - s_px[bi], sgy = ny - s_py[bi];
          const float d_next = (nx - x) * (nx - x) + (ny - y) * (ny - y);
          const float seg2 = sgx * sgx + sgy * sgy;
          const float tt = seg2 > 0.f ? 0.5f + 0.5f * (best - d_next) * fast_rcp(seg2) : 0.f;
          F = fmaxf(F + fminf(fmaxf(tt, -0.45f), 0.45f), 0.f);
        }
        return F;
      };
      float F = point_F();
      float m = flive ? F : 0.f;
      for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, WAVE));
      if (kWindow && j_lo) {
        // A lane whose true nearest point lies BELOW the window holds a value that is too high,
        // never too low: max over the lanes of the windowed values >= the true maximum, with
        // equality as soon as ONE lane that attains it is exact.  So: take a lane holding the
        // maximum and test every point below the window against its endpoint — one point per
        // lane of the wave, "<=" because an equal distance at a lower index wins the reference's
        // strict scan.  If one of them beats it (a path that doubles back under the endpoint),
        // every lane scans the lower blocks after all and the maximum is formed again.
        const unsigned long long holders = __ballot(flive && F == m);
        bool below = false;
        if (holders) {
          const int wl = __builtin_ctzll(holders);
          const float wx = __shfl(x, wl, WAVE), wy = __shfl(y, wl, WAVE), wbest = __shfl(best, wl, WAVE);
          for (uint32_t k = (uint32_t)lane; k < j_lo; k += WAVE) {
            const float ex = s_px[k] - wx, ey = s_py[k] - wy;
            below = below || (ex * ex + ey * ey <= wbest);
          }
        }
        if (__builtin_expect(__any(below), 0)) {
          for (uint32_t jj = j_lo; jj > 0; jj -= 4) {      // downwards: ties go to the lower block
            const uint32_t j = jj - 4;
            float dd[4];
            block_d2(s_px + j, s_py + j, dd);
            const float mn = fminf(fminf(dd[0], dd[1]), fminf(dd[2], dd[3]));
            if (mn <= best) {
              best = mn;
              bj = j;
            }
          }
          F = point_F();
          m = flive ? F : 0.f;
          for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, WAVE));
        }
      }
      F_local = fmaxf(F_local, m);
      if constexpr (LANE_FURTHEST_PRUNE) {
        // m is the exact maximum of the lanes that scanned (the check above): raise the block's word
        if (lane == 0)
          (void)__hip_atomic_fetch_max(reinterpret_cast<uint32_t*>(s_prune) + 2, __float_as_uint(m), __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_WORKGROUP);
        // developer aid: how many of this wave's groups took the scan (tools/lane_timeline.py)
        if (__builtin_expect(p.timeline != nullptr, 0) && lane == 0)
          p.timeline[SMPC_SCAN_COUNT_AT + blockIdx.x * 8 + wave] += 1ull;
      }
      }
      }
    }
