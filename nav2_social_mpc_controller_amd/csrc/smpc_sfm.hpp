// smpc_sfm.hpp — pieces of the Social Force Model (include/nav2_social_mpc_controller/sfm.hpp) that the people projection
// (smpc_project.hpp) and the crowd step (smpc_crowd.hpp) share: the angle wrap, the nearest-obstacle lookup of
// computeObstacle (src/optimizer.cpp:673-728) and one partner's term of computeSocialForce in table math.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/smpc.h"
#include "smpc_math.hpp"

namespace smpc {

// The reference normalises angles by repeated +-2 pi (sfm angle.hpp); every argument on this path is a difference of
// atan2 results except `yaw - init_yaw` at step 0, where init_yaw is caller data. A wave must terminate whatever the
// input: beyond 8 pi the value is pre-reduced with fmod (non-finite input comes back as NaN), within it the loop is the
// reference's own arithmetic.
__device__ inline double proj_wrap(double a) {
  if (!(fabs(a) <= 8.0 * M_PI)) a = fmod(a, 2 * M_PI);
  while (a <= -M_PI) a += 2 * M_PI;
  while (a > M_PI) a -= 2 * M_PI;
  return a;
}

// computeObstacle (src/optimizer.cpp:673-728): nearest-obstacle lookup, float arithmetic as in the reference; the
// result is agent - obstacle (the reference stores this DIFFERENCE where the SFM expects a position). In two parts so
// that the grid load of a step is in flight during the next step's desired and social forces: `issue` finds the cell
// and loads its entry, `finish` (called where the obstacle force needs it) turns the entry into the difference.
template <typename PP>
__device__ inline int proj_obstacle_issue(const PP& p, const uint32_t* idx, double ox, double oy, double px, double py,
                                          unsigned int& ob) {
  const double res = (double)p.od_resolution;
  const unsigned int xcell = (unsigned int)(long long)floor((px - ox) / res);
  const unsigned int ycell = (unsigned int)(long long)floor((py - oy) / res);
  ob = 0;
  if (xcell >= (unsigned int)p.od_width || ycell >= (unsigned int)p.od_height) return SMPC_PROJ_CELL_OUT_OF_BOUNDS;
  ob = idx[xcell + ycell * (unsigned int)p.od_width];
  return SMPC_PROJ_OK;
}
template <typename PP>
__device__ inline int proj_obstacle_finish(const PP& p, unsigned int ob, double ox, double oy, double px, double py,
                                           double& dx, double& dy) {
  if (ob >= (unsigned int)p.od_width * (unsigned int)p.od_height) return SMPC_PROJ_INDEX_OUT_OF_BOUNDS;
  const unsigned int oyc = ob / (unsigned int)p.od_width, oxc = ob % (unsigned int)p.od_width;
  const float x = (float)((double)((float)oxc * p.od_resolution) + ox);
  const float y = (float)((double)((float)oyc * p.od_resolution) + oy);
  dx = px - (double)x;
  dy = py - (double)y;
  return SMPC_PROJ_OK;
}

// sqrt(z) for z >= 0 through the refined reciprocal square root (1-2 ulp; 0 stays 0)
__device__ inline double proj_sqrt(double z) { return z > 0.0 ? z * rsqrt_pos(z) : 0.0; }

// computeSocialForce's term of one partner (sfm.hpp:237-281): diff = partner - self, dv = own velocity - partner's.
// Constants of the reference's defaults (forceFactorSocial 2.1, lambda 2, gamma 0.35, n 2, n' 3). Two phases, so that
// a caller with several partners in flight keeps their arithmetic in straight-line code and visits the rare
// two-arctangent form once for all of them.
struct ProjPair {
  double ex, ey, ix, iy, il, earg, theta;
  bool same_vel, near_axis;
};
__device__ inline void proj_pair_begin(MathTabP mt, double dfx, double dfy, double dvx, double dvy, ProjPair& q) {
  const double kLam = 2.0, kGam = 0.35;
  const double z = dfx * dfx + dfy * dfy;
  const double inv_nd = rsqrt_pos(fmax(z, 1e-300));
  const double nd = z * inv_nd;
  q.ex = z > 0 ? dfx * inv_nd : dfx; q.ey = z > 0 ? dfy * inv_nd : dfy;
  const double ivx = kLam * dvx + q.ex, ivy = kLam * dvy + q.ey;
  const double inv_il = rsqrt_pos(ivx * ivx + ivy * ivy);
  q.il = (ivx * ivx + ivy * ivy) * inv_il;
  q.ix = ivx * inv_il; q.iy = ivy * inv_il;
  // equal velocities (two standing people): theta is mathematically 0 and the reference gets its libm's last-bit
  // noise (its thetaSign is then 0 or +-1 by chance); take exactly 0, the convention of the hot path
  q.same_vel = (kLam * dvx == 0.0) && (kLam * dvy == 0.0);
  // theta = wrap(atan2(e) - atan2(i)) is the angle from i to e = atan2(i x e, i . e): one table arctangent away from
  // theta = 0 and |theta| = pi, the reference's own two-atan2 form next to them (its last bits decide thetaSign)
  const double cross = q.ix * q.ey - q.iy * q.ex, dot = q.ix * q.ex + q.iy * q.ey;
  q.theta = atan2_dir(mt, cross, dot);
  q.near_axis = !q.same_vel && !(fabs(cross) >= 1e-6);  // (equal velocities: i = e, cross = 0, theta := 0 anyway)
  q.earg = -nd * inv_il * (1.0 / kGam);  // -|diff| / B
}
__device__ inline void proj_pair_exact_theta(ProjPair& q) {
  if (q.near_axis) q.theta = proj_wrap(proj_wrap(atan2(q.ey, q.ex)) - proj_wrap(atan2(q.iy, q.ix)));
}
__device__ inline void proj_pair_end(MathTabP mt, const ProjPair& q, double& sfx, double& sfy) {
  const double kFs = 2.1, kGam = 0.35, kN = 2.0, kNp = 3.0;
  const double theta = q.same_vel ? 0.0 : q.theta;
  const double Bq = kGam * q.il;
  const double a1 = kNp * Bq * theta, a2 = kN * Bq * theta;
  const double fv = -exp_tab(mt, fma(-a1, a1, q.earg));
  const double sgn = (theta == 0) ? 0.0 : ((theta > 0) ? 1.0 : -1.0);  // sfm.hpp:265-270
  const double fa = -sgn * exp_tab(mt, fma(-a2, a2, q.earg));
  sfx = kFs * (fv * q.ix + fa * (-q.iy));
  sfy = kFs * (fv * q.iy + fa * q.ix);
}

}  // namespace smpc
