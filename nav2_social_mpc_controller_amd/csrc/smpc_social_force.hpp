// smpc_social_force.hpp — the social force between one (me, other) pair with its derivatives, as the social-work critic
// needs it: the general form that follows the reference case by case (social_force_general) and the branch-free form
// of the agent loop for a regular pair (pair_force).
#pragma once

#include <hip/hip_runtime.h>

#include "smpc_math.hpp"

namespace smpc {

__device__ inline double wrap_to_pi(double a) {  // critics/social_work_cost_function.hpp:39-46
  // only ever called on a difference of two atan2 results (|a| <= 2 pi, or NaN): at most one trip per loop; the guard
  // keeps the wave finite should that ever change
  if (!(fabs(a) <= 8.0 * M_PI)) a = fmod(a, 2.0 * M_PI);
  while (a > M_PI) a -= 2.0 * M_PI;
  while (a <= -M_PI) a += 2.0 * M_PI;
  return a;
}

// ------------------------------------------------------------------------------------------------
// Social force between one (me, other) pair and its derivatives with respect to diff = me_pos - other_pos and
// u = me_vel - other_vel. Restates computeSocialForce (critics/social_work_cost_function.hpp:164-228) for a
// single "other"; constants from src/critics/social_work_cost_function.cpp:38-43. F = k (fv i + fa i_perp).
// ------------------------------------------------------------------------------------------------
struct Force {
  double fx, fy;
  double dfx_dx, dfy_dx, dfx_dy, dfy_dy;      // wrt diff
  double dfx_dux, dfy_dux, dfx_duy, dfy_duy;  // wrt u
  bool special;  // pair_force() only: this pair needs social_force_general() (theta within 1e-6 of 0 or pi)
};

// 1/sqrt(x) for a normal positive x: hardware estimate + one cubic correction (what the library routine does, without
// its zero / infinity / denormal cases, which cannot occur here: d2 >= 1e-12 after the coincident-pair clamp, and a
// vanishing interaction vector is a singular configuration for the reference as well).
__device__ inline double fast_rsqrt(double x) {
  const double y = __builtin_amdgcn_rsq(x);
  const double e = fma(-x * y, y, 1.0);
  return fma(y * e, fma(e, 0.375, 0.5), y);
}

__device__ inline Force social_force_general(double dx, double dy, double ux, double uy) {
  const double lambda = 2.0, gamma = 0.35, nPrime = 3.0, nn = 2.0, k = 2.1;
  Force R;
  double d2 = dx * dx + dy * dy;
  const bool degenerate = d2 < 1e-12;  // |diff| < 1e-6 (:181-184): diff := (1e-6, 0), a constant: no dependence on positions
  if (degenerate) { dx = 1e-6; dy = 0.0; d2 = 1e-12; }
  const double inv_n = fast_rsqrt(d2);
  const double n = d2 * inv_n;
  const double ex = dx * inv_n, ey = dy * inv_n;  // diffDirection :185
  const double ivx = fma(lambda, ux, ex), ivy = fma(lambda, uy, ey);  // :191-192 (lambda u is exact: lambda = 2)
  const double L2 = ivx * ivx + ivy * ivy;
  const double inv_L = fast_rsqrt(L2);
  const double L = L2 * inv_L;  // :194
  const double ix = ivx * inv_L, iy = ivy * inv_L;  // :195-196
  // theta = wrapToPi(atan2(dir) - atan2(idir)) (:198-200) is the angle from idir to dir = atan2(idir x dir, idir . dir).
  // One atan2 instead of two wherever that cannot change sign(theta): away from theta = 0 and |theta| = pi
  // (|sin theta| >= 1e-6). Closer than that the reference's own two-atan2 form is evaluated, so that the last-bit
  // behaviour next to the discontinuity of sign(theta) (:210) stays the reference's.
  // Equal velocities (robot stopped beside a standing person): theta is mathematically 0 and the reference's value is
  // 0 up to the last-bit noise of its own libm (which then decides sign(theta)). Take exactly 0.
  const double cross = ix * ey - iy * ex, dot = ix * ex + iy * ey;
  double phi;
  if (ux == 0.0 && uy == 0.0) {
    phi = 0.0;
  } else if (fabs(cross) >= 1e-6) {
    phi = atan2(cross, dot);
  } else {
    phi = wrap_to_pi(atan2(ey, ex) - atan2(iy, ix));
  }
  const double Bq = gamma * L;  // :203
  const double inv_B = inv_L * (1.0 / gamma);
  const double a1 = nPrime * Bq * phi, a2 = nn * Bq * phi;
  const double base = -n * inv_B;
  const double E1 = exp(base - a1 * a1);  // :205-207
  const double E2 = exp(base - a2 * a2);  // :212-215
  const double sgn = (phi > 0.0) ? 1.0 : -1.0;  // :210
  const double fv = -E1, fa = -sgn * E2;
  R.fx = k * (fv * ix - fa * iy);  // :218-224, i_perp = (-iy, ix)
  R.fy = k * (fv * iy + fa * ix);
  // The force depends on its inputs through (n, alpha = atan2(e), iv): dF = A_n dn + A_alpha dalpha + A_x d(iv_x) +
  // A_y d(iv_y). With dL = i . d(iv), kappa = d atan2(i) = (i_perp . d(iv)) / L, dphi = dalpha - kappa, dB = gamma dL,
  //   d(arg_m) = -dn/B + n dB/B^2 - 2 a_m c_m (dB phi + B dphi),   dF = k ((dfv - fa kappa) i + (dfa + fv kappa) i_perp),
  // the four columns are evaluated once and every direction below is a linear combination of them.
  const double nB2 = n * inv_B * inv_B;
  // A_n: dn = 1 -> d(arg) = -1/B, no rotation: -F / B
  const double anx = -inv_B * R.fx, any = -inv_B * R.fy;
  // A_alpha: dalpha = 1 -> dphi = 1, d(arg_m) = -2 a_m c_m B
  double aax, aay;
  {
    const double twoB = 2.0 * Bq;
    const double dfv = E1 * (a1 * nPrime * twoB);
    const double dfa = sgn * E2 * (a2 * nn * twoB);
    aax = k * (dfv * ix - dfa * iy);
    aay = k * (dfv * iy + dfa * ix);
  }
  // A_x, A_y: d(iv) = (1, 0) / (0, 1)
  auto column = [&](double dL, double kappa, double& ofx, double& ofy) {
    const double dB = gamma * dL;
    const double dbase = nB2 * dB;
    const double common = dB * phi - Bq * kappa;  // dphi = -kappa
    const double dfv = -E1 * (dbase - 2.0 * a1 * nPrime * common);
    const double dfa = -sgn * E2 * (dbase - 2.0 * a2 * nn * common);
    const double ci = dfv - fa * kappa, cp = dfa + fv * kappa;
    ofx = k * (ci * ix - cp * iy);
    ofy = k * (ci * iy + cp * ix);
  };
  double axx, axy, ayx, ayy;
  column(ix, -iy * inv_L, axx, axy);
  column(iy, ix * inv_L, ayx, ayy);
  R.dfx_dux = lambda * axx; R.dfy_dux = lambda * axy;  // u enters iv as lambda u
  R.dfx_duy = lambda * ayx; R.dfy_duy = lambda * ayy;
  if (degenerate) {
    R.dfx_dx = R.dfy_dx = R.dfx_dy = R.dfy_dy = 0.0;
  } else {
    // moving diff by dd: dn = e . dd, dalpha = (e_perp . dd) / n, d(iv) = de = e_perp dalpha, e_perp = (-ey, ex);
    // C = A_alpha + A_x (-ey) + A_y ex is what one unit of dalpha does in total
    const double cx = aax - ey * axx + ex * ayx, cy = aay - ey * axy + ex * ayy;
    const double da1 = -ey * inv_n, da2 = ex * inv_n;  // dd = (1, 0) / (0, 1)
    R.dfx_dx = ex * anx + da1 * cx; R.dfy_dx = ex * any + da1 * cy;
    R.dfx_dy = ey * anx + da2 * cx; R.dfy_dy = ey * any + da2 * cy;
  }
  return R;
}

// The same force for a regular pair (|diff| >= 1e-6, the overwhelmingly common case), built for instruction count:
// table-driven exp / atan2 (smpc_math.hpp), no selects for the coincident-pair clamp, no branches. Two rare shapes
// are only flagged, for the caller to redo the step's agents with social_force_general(): a coincident pair (flagged
// by the caller) and a pair whose theta is within 1e-6 of 0 or pi while the velocities differ (Force::special: next
// to the discontinuity of sign(theta) the reference's own two-atan2 form decides, :198-200).
// pair_force(-d, -u) == -pair_force(d, u) bit for bit (every intermediate flips sign or stays exactly), with equal
// derivatives: the force on an agent from the robot needs no evaluation of its own.
// The constant factors are left to the caller, who applies them once to the sums over the agents of a step instead of
// to every pair: the force and its diff-derivatives come WITHOUT the factor k (kPairForceK), the u-derivatives without
// k * lambda (kPairForceLambda; u enters the interaction vector as lambda u).
constexpr double kPairForceK = 2.1, kPairForceLambda = 2.0;
__device__ inline Force pair_force(MathTabP mt, const double* atab, double dx, double dy, double ux, double uy) {
  const double lambda = kPairForceLambda, gamma = 0.35, nPrime = 3.0, nn = 2.0;
  Force R;
  const double d2 = fma(dx, dx, dy * dy);
  const double inv_n = rsqrt_pos(d2);
  const double n = d2 * inv_n;
  const double ex = dx * inv_n, ey = dy * inv_n;  // diffDirection :185
  const double ivx = fma(lambda, ux, ex), ivy = fma(lambda, uy, ey);  // :191-192
  const double L2 = fma(ivx, ivx, ivy * ivy);
  const double inv_L = rsqrt_pos(L2);
  const double L = L2 * inv_L;  // :194
  const double ix = ivx * inv_L, iy = ivy * inv_L;  // :195-196
  const double cross = fma(ix, ey, -(iy * ex)), dot = fma(ix, ex, iy * ey);
  const bool zero_u = (ux == 0.0) & (uy == 0.0);  // equal velocities: theta := 0 (parity)
  double phi = atan2_unit(mt, atab, cross, dot);  // (cross, dot) = (sin, cos) of theta: a unit vector
  // keep the scheduler from interleaving the arctangent, the two exponentials and the derivative block: the extra
  // overlap buys nothing with two or three waves per SIMD and costs ~15 VGPRs (the stand-alone K1 kernel would drop
  // from three waves per SIMD to two)
  __builtin_amdgcn_sched_barrier(0);
  R.special = !zero_u & (fabs(cross) < 1e-6);
  phi = zero_u ? 0.0 : phi;
  const double Bq = gamma * L;  // :203
  const double inv_B = inv_L * (1.0 / gamma);
  const double a1 = nPrime * Bq * phi, a2 = nn * Bq * phi;
  const double base = -n * inv_B;
  const double E1 = exp_tab(mt, fma(-a1, a1, base));  // :205-207
  const double E2 = exp_tab(mt, fma(-a2, a2, base));  // :212-215
  __builtin_amdgcn_sched_barrier(0);
  const double fv = -E1;
  const double fa = (phi > 0.0) ? -E2 : E2;  // -sign(theta) E2, sign = -1 at theta == 0 (:210)
  R.fx = fma(fv, ix, -(fa * iy));  // :218-224 without the factor k, i_perp = (-iy, ix)
  R.fy = fma(fv, iy, fa * ix);
  // derivative: see social_force_general(); dfa = sgn E2 (...) = -fa (...)
  const double nB2 = n * inv_B * inv_B;
  const double anx = -inv_B * R.fx, any = -inv_B * R.fy;
  const double twoB = 2.0 * Bq;
  const double g1 = a1 * nPrime, g2 = a2 * nn;
  double aax, aay;
  {
    const double dfv = E1 * (g1 * twoB);
    const double dfa = -fa * (g2 * twoB);
    aax = fma(dfv, ix, -(dfa * iy));
    aay = fma(dfv, iy, dfa * ix);
  }
  auto column = [&](double dL, double kappa, double& ofx, double& ofy) {
    const double dB = gamma * dL;
    const double dbase = nB2 * dB;
    const double common = 2.0 * fma(dB, phi, -(Bq * kappa));  // dphi = -kappa
    const double dfv = fv * fma(-g1, common, dbase);
    const double dfa = fa * fma(-g2, common, dbase);
    const double ci = fma(-fa, kappa, dfv), cp = fma(fv, kappa, dfa);
    ofx = fma(ci, ix, -(cp * iy));
    ofy = fma(ci, iy, cp * ix);
  };
  double axx, axy, ayx, ayy;
  column(ix, -iy * inv_L, axx, axy);
  column(iy, ix * inv_L, ayx, ayy);
  R.dfx_dux = axx; R.dfy_dux = axy;  // without the factor k * lambda
  R.dfx_duy = ayx; R.dfy_duy = ayy;
  const double cx = aax - ey * axx + ex * ayx, cy = aay - ey * axy + ex * ayy;
  const double da1 = -ey * inv_n, da2 = ex * inv_n;
  R.dfx_dx = ex * anx + da1 * cx; R.dfy_dx = ex * any + da1 * cy;
  R.dfx_dy = ey * anx + da2 * cx; R.dfy_dy = ey * any + da2 * cy;
  return R;
}

}  // namespace smpc
