// smpc_lm.hpp — the parts of the Levenberg-Marquardt solve the solve kernel (smpc_solve_kernel.hpp) is assembled from:
// the small dense solves and polynomial root finders of the line search's interpolation, its register-resident fast
// paths, the Armijo test, and the names of the state machine's phases, scalars and registers.
// Algorithm = Ceres' trust-region minimizer with bounds as specified in SURVEY.md Appendix A (A.4 .. A.11).
#pragma once

#include <hip/hip_runtime.h>

#include "smpc_math.hpp"

namespace smpc {

#ifdef SMPC_STAMPS
// diagnostic build only: [0] bracketed_root<4> calls, [1] their iterations, [2] bracketed_root<3> calls, [3] iterations,
// [4] interpolations (cubic), [5] (quintic), [6] quintic shortcut taken, [7] generic fallback
__device__ unsigned long long g_ls_dbg[8];
#define SMPC_LS_COUNT(i, n) do { if ((threadIdx.x & 31) == 0) atomicAdd(&g_ls_dbg[i], (unsigned long long)(n)); } while (0)
#else
#define SMPC_LS_COUNT(i, n) do { } while (0)
#endif

// ---- small uniform helpers working on an LDS scratch area (dynamic indexing without private scratch) ----

// Solve A z = b with full pivoting, n <= 6, A row-major n x n in LDS (destroyed). Result in z (LDS).
__device__ inline void fullpiv_solve(double* A, double* b, int* perm, double* z, double* out, int n) {
  for (int i = 0; i < n; ++i) perm[i] = i;
  for (int kk = 0; kk < n; ++kk) {
    int pr = kk, pc = kk;
    double best = -1.0;
    for (int i = kk; i < n; ++i)
      for (int j = kk; j < n; ++j) {
        const double v = fabs(A[i * n + j]);
        if (v > best) { best = v; pr = i; pc = j; }
      }
    if (best == 0.0) { for (int i = kk; i < n; ++i) b[i] = 0.0; break; }
    if (pr != kk) {
      for (int j = 0; j < n; ++j) { const double t = A[pr * n + j]; A[pr * n + j] = A[kk * n + j]; A[kk * n + j] = t; }
      const double t = b[pr]; b[pr] = b[kk]; b[kk] = t;
    }
    if (pc != kk) {
      for (int i = 0; i < n; ++i) { const double t = A[i * n + pc]; A[i * n + pc] = A[i * n + kk]; A[i * n + kk] = t; }
      const int t = perm[pc]; perm[pc] = perm[kk]; perm[kk] = t;
    }
    for (int i = kk + 1; i < n; ++i) {
      const double f = A[i * n + kk] / A[kk * n + kk];
      for (int j = kk; j < n; ++j) A[i * n + j] -= f * A[kk * n + j];
      b[i] -= f * b[kk];
    }
  }
  for (int i = n - 1; i >= 0; --i) {
    if (A[i * n + i] == 0.0) { z[i] = 0.0; continue; }
    double v = b[i];
    for (int kk = i + 1; kk < n; ++kk) v -= A[i * n + kk] * z[kk];
    z[i] = v / A[i * n + i];
  }
  for (int i = 0; i < n; ++i) out[perm[i]] = z[i];
}

__device__ inline double eval_poly(const double* p, int ncoef, double x) {
  double v = 0.0;
  for (int i = 0; i < ncoef; ++i) v = v * x + p[i];
  return v;
}

// Real parts of all roots of the polynomial p (highest degree first, ncoef coefficients) into roots[]; returns count.
__device__ inline int poly_roots_real(const double* pin, int ncoef, double* roots, double* zr, double* zi, double* cm) {
  int lead = 0;
  while (lead + 1 < ncoef && pin[lead] == 0.0) ++lead;
  const double* p = pin + lead;
  const int deg = ncoef - lead - 1;
  if (deg <= 0) return 0;
  if (deg == 1) { roots[0] = -p[1] / p[0]; return 1; }
  if (deg == 2) {
    const double a = p[0], b = p[1], cc = p[2];
    const double D = b * b - 4 * a * cc;
    const double sD = sqrt(fabs(D));
    if (D >= 0) {
      if (b >= 0) { roots[0] = (-b - sD) / (2.0 * a); roots[1] = (2.0 * cc) / (-b - sD); }
      else { roots[0] = (2.0 * cc) / (-b + sD); roots[1] = (-b + sD) / (2.0 * a); }
    } else { roots[0] = -b / (2.0 * a); roots[1] = -b / (2.0 * a); }
    return 2;
  }
  // Aberth-Ehrlich on the monic polynomial
  double radius = 0.0;
  for (int i = 0; i <= deg; ++i) cm[i] = p[i] / p[0];
  for (int i = 1; i <= deg; ++i) radius = fmax(radius, pow(fabs(cm[i]), 1.0 / i));
  radius = fmax(2.0 * radius, 1e-300);
  for (int i = 0; i < deg; ++i) {
    double sn, cs;
    sincos(2.0 * M_PI * i / deg + 0.4, &sn, &cs);
    zr[i] = radius * cs; zi[i] = radius * sn;
  }
  for (int it = 0; it < 200; ++it) {
    double maxstep = 0.0;
    for (int i = 0; i < deg; ++i) {
      const double xr = zr[i], xi = zi[i];
      double pr = cm[0], pi = 0.0, dr = 0.0, di = 0.0;
      for (int kk = 1; kk <= deg; ++kk) {
        const double ndr = dr * xr - di * xi + pr, ndi = dr * xi + di * xr + pi;
        dr = ndr; di = ndi;
        const double npr = pr * xr - pi * xi + cm[kk], npi = pr * xi + pi * xr;
        pr = npr; pi = npi;
      }
      if (pr == 0.0 && pi == 0.0) continue;
      // ratio = p / p'
      const double dd = dr * dr + di * di;
      const double rr = (pr * dr + pi * di) / dd, ri = (pi * dr - pr * di) / dd;
      double sr = 0.0, si = 0.0;
      for (int j = 0; j < deg; ++j) {
        if (j == i) continue;
        const double er = xr - zr[j], ei = xi - zi[j];
        const double ee = er * er + ei * ei;
        sr += er / ee; si += -ei / ee;
      }
      // step = ratio / (1 - ratio * sum)
      const double qr = 1.0 - (rr * sr - ri * si), qi = -(rr * si + ri * sr);
      const double qq = qr * qr + qi * qi;
      const double str = (rr * qr + ri * qi) / qq, sti = (ri * qr - rr * qi) / qq;
      zr[i] = xr - str; zi[i] = xi - sti;
      const double mag = sqrt(zr[i] * zr[i] + zi[i] * zi[i]);
      maxstep = fmax(maxstep, sqrt(str * str + sti * sti) / fmax(1e-300, mag));
    }
    if (maxstep < 1e-15) break;
  }
  for (int i = 0; i < deg; ++i) roots[i] = zr[i];
  return deg;
}

struct Sample {
  double x, value, gradient;
  bool value_valid, gradient_valid;
};

// LineSearch::InterpolatingPolynomialMinimizingStepSize with CUBIC interpolation:
// fit a polynomial through {lowerbound, current[, previous]} (values and directional derivatives), minimise on
// [lo, hi]. scratch: >= 96 doubles of LDS.
__device__ __attribute__((always_inline)) inline double interpolate_step(const Sample& lower, const Sample& previous, const Sample& current,
                                          double lo, double hi, double* scratch) {
  if (!current.value_valid) return fmin(fmax(current.x * 0.5, lo), hi);
  double* A = scratch;          // 36
  double* b = scratch + 36;     // 6
  double* z = scratch + 42;     // 6
  double* poly = scratch + 48;  // 6
  double* dpoly = scratch + 54; // 6
  double* roots = scratch + 60; // 6
  double* zr = scratch + 66;    // 6
  double* zi = scratch + 72;    // 6
  double* cm = scratch + 78;    // 6
  int* perm = (int*)(scratch + 84);  // 6 ints
  const bool use_prev = previous.value_valid;
  int nc = (lower.value_valid ? 1 : 0) + (lower.gradient_valid ? 1 : 0) + (current.value_valid ? 1 : 0) +
           (current.gradient_valid ? 1 : 0);
  if (use_prev) nc += (previous.value_valid ? 1 : 0) + (previous.gradient_valid ? 1 : 0);
  const int degree = nc - 1;
  int row = 0;
  auto add_sample = [&](const Sample& sm) {
    if (sm.value_valid) {
      double pw = 1.0;
      for (int j = degree; j >= 0; --j) { A[row * nc + j] = pw; pw *= sm.x; }
      b[row] = sm.value; ++row;
    }
    if (sm.gradient_valid) {
      double pw = 1.0;
      A[row * nc + degree] = 0.0;
      for (int j = degree - 1; j >= 0; --j) { A[row * nc + j] = (degree - j) * pw; pw *= sm.x; }
      b[row] = sm.gradient; ++row;
    }
  };
  add_sample(lower);
  add_sample(current);
  if (use_prev) add_sample(previous);
  fullpiv_solve(A, b, perm, z, poly, nc);
  // MinimizePolynomial on [lo, hi]
  double opt_x = (lo + hi) / 2.0;
  double opt_v = eval_poly(poly, nc, opt_x);
  const double vlo = eval_poly(poly, nc, lo);
  if (vlo < opt_v) { opt_v = vlo; opt_x = lo; }
  const double vhi = eval_poly(poly, nc, hi);
  if (vhi < opt_v) { opt_v = vhi; opt_x = hi; }
  if (nc > 2) {
    for (int i = 0; i < degree; ++i) dpoly[i] = (degree - i) * poly[i];
    const int nr = poly_roots_real(dpoly, degree, roots, zr, zi, cm);
    for (int i = 0; i < nr; ++i) {
      const double rt = roots[i];
      if (rt < lo || rt > hi) continue;
      const double v = eval_poly(poly, nc, rt);
      if (v < opt_v) { opt_v = v; opt_x = rt; }
    }
  }
  auto check_sample = [&](const Sample& sm) {
    if (sm.x < lo || sm.x > hi) return;
    const double v = eval_poly(poly, nc, sm.x);
    if (v < opt_v) { opt_x = sm.x; opt_v = v; }
  };
  check_sample(lower);
  check_sample(current);
  if (use_prev) check_sample(previous);
  return opt_x;
}

// ---- register-resident fast paths of the line-search interpolation (same algorithm as above, no LDS loops) ----

template <int nc> __device__ inline double eval_poly_reg(const double (&p)[nc], double x) {
  double v = 0.0;
#pragma unroll
  for (int i = 0; i < nc; ++i) v = v * x + p[i];
  return v;
}

// 1/x to ~1e-16 relative: hardware estimate + two Newton steps (only used where a last-bit error is harmless).
__device__ inline double fast_rcp(double x) {
  double r = __builtin_amdgcn_rcp(x);
  r = r * fma(-x, r, 2.0);
  r = r * fma(-x, r, 2.0);
  return r;
}

// sqrt(x) for x >= 0 (0 stays 0) through the refined reciprocal square root: 7 instructions instead of the library's
// ~20 (1-2 ulp; used for norms that only enter tolerance tests and for discriminants of the line search).
__device__ inline double fast_sqrt(double x) { return x > 0.0 ? x * rsqrt_pos(x) : 0.0; }

// Horner value and derivative of a degree-D polynomial p[0] x^D + ... + p[D].
template <int D> __device__ inline void horner_d(const double (&p)[D + 1], double x, double& f, double& df) {
  double v = p[0], d = 0.0;
#pragma unroll
  for (int i = 1; i <= D; ++i) { d = fma(d, x, v); v = fma(v, x, p[i]); }
  f = v; df = d;
}

// The root of p inside [a, b], a <= b, given that p is monotone there: Newton from the midpoint, kept inside the
// shrinking sign-change bracket (bisection whenever a Newton step leaves it). NaN if p does not change sign on [a, b].
template <int D> __device__ inline double bracketed_root(const double (&p)[D + 1], double a, double b, int* trips = nullptr) {
  double fa, fb, t;
  horner_d<D>(p, a, fa, t);
  horner_d<D>(p, b, fb, t);
  if (fa == 0.0) return a;
  if (fb == 0.0) return b;
  if (!((fa < 0.0) != (fb < 0.0)) || !(fa == fa) || !(fb == fb)) return __builtin_nan("");
  const bool neg_lo = fa < 0.0;
  // start from the secant point of the bracket (inside it, since the signs differ); Newton from there, bisection
  // whenever a step leaves the shrinking bracket
  double xl = a, xh = b, x = a - fa * (b - a) * fast_rcp(fb - fa);
  if (!(x > a && x < b)) x = 0.5 * (a + b);
  for (int it = 0; it < 80; ++it) {
    SMPC_LS_COUNT(D == 4 ? 1 : 3, 1);
    if (trips) ++*trips;
    double fx, dfx;
    horner_d<D>(p, x, fx, dfx);
    if (fx == 0.0) break;
    if ((fx < 0.0) == neg_lo) xl = x; else xh = x;
    double xn = x - fx * fast_rcp(dfx);
    // inclusive: a converged iterate moves by less than an ulp, lands ON the bracket end it has just become, and must
    // count as a (zero-length) Newton step — with strict inequalities it was sent back to the midpoint of a still wide
    // bracket and the search started over (measured on real line searches: 11 % of the calls took 16..58 trips)
    const bool newton = xn >= xl && xn <= xh;
    if (!newton) xn = 0.5 * (xl + xh);
    // A Newton step below 1e-9 |x| leaves an error of the order of its square; waiting for the step itself to reach
    // round-off would spin on polynomials whose Horner value is noisier than that (measured: 7% of the solve kernel).
    const double dx = fabs(xn - x);
    const bool done = (newton && dx <= 1e-9 * fabs(xn)) || dx <= 4e-16 * fabs(xn);
    x = xn;
    if (done) break;
  }
  SMPC_LS_COUNT(D == 4 ? 0 : 2, 1);
  return x;
}

// Real roots of the quartic q (q[0] != 0) inside [lo, hi] — the only roots of the derivative that can win the
// minimisation of the interpolating quintic (the real part of a complex pair, which the reference's companion-matrix /
// this repository's Aberth fallback also offer as candidates, is never a critical point and so never below the minimum
// over {lo, hi, real critical points}). Isolation by monotone pieces: the roots of q'' (quadratic, closed form) cut
// [lo, hi] into <= 3 pieces on which q' is monotone; its <= 3 roots there cut [lo, hi] into <= 4 pieces on which q is
// monotone. Four neighbouring lanes take one piece each (lane & 3); roots[j] is NaN where piece j holds no root.
__device__ inline void quartic_roots_in_range_lanes(const double (&q)[5], double lo, double hi, double (&roots)[4]) {
  int lane = threadIdx.x & 63;
  asm volatile("" : "+v"(lane));  // (the masks "r == j" stay here: hoisted out of the persistent loop they were spilled SGPR pairs)
  const int r = lane & 3, base = lane & ~3;
  const double A = 12.0 * q[0], Bq = 6.0 * q[1], C = 2.0 * q[2];
  double e0 = lo, e1 = lo;
  bool inflection_inside = false;
  const double D = Bq * Bq - 4.0 * A * C;
  if (D > 0.0) {
    const double t = -0.5 * (Bq + copysign(fast_sqrt(D), Bq));
    const double x1 = t * fast_rcp(A), x2 = C * fast_rcp(t);
    inflection_inside = (x1 > lo && x1 < hi) || (x2 > lo && x2 < hi);
    e0 = fmin(fmax(fmin(x1, x2), lo), hi);
    e1 = fmax(fmin(fmax(x1, x2), hi), lo);
  }
  {
    // The common shape of a line-search interpolant (96 % of 6850 quintic fits dumped from real solves): q = p' has
    // opposite signs at the two ends and no inflection in between (q'' keeps its sign, q is convex or concave), so q
    // has exactly one root there — the only critical point of p in the interval. One bracketed iteration, the same in
    // every lane, instead of the two lane-parallel isolation stages below; and when q falls through zero the point is
    // a local maximum of p, which can never win against the interval ends: nothing to compute at all.
    double ql, qh, t;
    horner_d<4>(q, lo, ql, t);
    horner_d<4>(q, hi, qh, t);
    const bool one_root = !inflection_inside && ((ql < 0.0 && qh > 0.0) || (ql > 0.0 && qh < 0.0));
    if (one_root) SMPC_LS_COUNT(6, 1);
    if (one_root) {  // decided per slot (the value is the same in all its lanes): a result never depends on the wave's other scene
      roots[0] = (ql < 0.0) ? bracketed_root<4>(q, lo, hi) : __builtin_nan("");
      roots[1] = roots[2] = roots[3] = __builtin_nan("");
      return;
    }
  }
  const double d1[4] = {4.0 * q[0], 3.0 * q[1], 2.0 * q[2], q[3]};
  const double pa = (r == 0) ? lo : (r == 1) ? e0 : e1;
  const double pb = (r == 0) ? e0 : (r == 1) ? e1 : hi;
  const double s = bracketed_root<3>(d1, pa, pb);
  const double s0 = __shfl(s, base + 0, 64), s1 = __shfl(s, base + 1, 64), s2 = __shfl(s, base + 2, 64);
  const double b1 = (s0 == s0) ? s0 : lo;
  const double b2 = (s1 == s1) ? fmax(s1, b1) : b1;
  const double b3 = (s2 == s2) ? fmax(s2, b2) : b2;
  const double ca = (r == 0) ? lo : (r == 1) ? b1 : (r == 2) ? b2 : b3;
  const double cb = (r == 0) ? b1 : (r == 1) ? b2 : (r == 2) ? b3 : hi;
  const double root = bracketed_root<4>(q, ca, cb);
#pragma unroll
  for (int j = 0; j < 4; ++j) roots[j] = __shfl(root, base + j, 64);
}

// MinimizeInterpolatingPolynomial for the two common shapes: {lower, current} with all values and gradients valid
// (cubic) and {lower, current, previous} (quintic). The lower bound sample always sits at x = 0, so its two
// interpolation conditions fix the two lowest coefficients exactly (p(0) = f0, p'(0) = g0; in the full-pivot LU of
// FindInterpolatingPolynomial those two unit rows are never touched by an elimination step either); the remaining
// 2 / 4 coefficients come from the reduced system of the other samples. Returns false if the shape is not covered.
__device__ inline bool interpolate_step_fast(const Sample& lower, const Sample& previous, const Sample& current,
                                             double lo, double hi, double& step_size) {
  if (!(lower.value_valid && lower.gradient_valid && current.value_valid && current.gradient_valid)) return false;
  if (lower.x != 0.0) return false;
  const bool use_prev = previous.value_valid;
  if (use_prev && !previous.gradient_valid) return false;
  const double f0 = lower.value, g0 = lower.gradient;
  double opt_x = (lo + hi) / 2.0, opt_v;
  SMPC_LS_COUNT(use_prev ? 5 : 4, 1);
  if (!use_prev) {
    constexpr int nc = 4;
    // a x1^3 + b x1^2 = f1 - g0 x1 - f0 =: A ;  3 a x1^2 + 2 b x1 = g1 - g0 =: B, solved in closed form (the reference
    // runs a full-pivot LU on the 4 x 4 Vandermonde system: the same polynomial up to its round-off)
    const double x1 = current.x;
    if (x1 == 0.0) return false;
    const double rx = fast_rcp(x1);
    const double A = current.value - g0 * x1 - f0, Bx = (current.gradient - g0) * x1;
    const double rxsq = rx * rx;
    const double poly[nc] = {(Bx - 2.0 * A) * (rxsq * rx), (3.0 * A - Bx) * rxsq, g0, f0};
    opt_v = eval_poly_reg<nc>(poly, opt_x);
    const double vlo = eval_poly_reg<nc>(poly, lo);
    if (vlo < opt_v) { opt_v = vlo; opt_x = lo; }
    const double vhi = eval_poly_reg<nc>(poly, hi);
    if (vhi < opt_v) { opt_v = vhi; opt_x = hi; }
    // derivative 3 p0 x^2 + 2 p1 x + p2, roots as poly_roots_real() finds them (leading zeros stripped)
    const double qa = 3.0 * poly[0], qb = 2.0 * poly[1], qc = poly[2];
    double r0 = 0.0, r1 = 0.0;
    int nr = 0;
    if (qa != 0.0) {
      const double D = qb * qb - 4 * qa * qc;
      const double sD = fast_sqrt(fabs(D));
      const double inv2a = fast_rcp(2.0 * qa);
      if (D >= 0) {
        // the stable pair of formulas: tq = -(qb + sign(qb) sD) is the sum without cancellation
        const double tq = (qb >= 0) ? (-qb - sD) : (-qb + sD);
        const double big = tq * inv2a, small = (2.0 * qc) * fast_rcp(tq);
        r0 = (qb >= 0) ? big : small;
        r1 = (qb >= 0) ? small : big;
      } else { r0 = -qb * inv2a; r1 = r0; }
      nr = 2;
    } else if (qb != 0.0) { r0 = -qc * fast_rcp(qb); nr = 1; }
    // Candidates: the critical points and the samples themselves, each only if it lies in [lo, hi]. In a backtracking
    // search the interval is [1e-3, 0.6] x the current step, so the samples (0, the current step, the longer previous
    // one) never do, and of the two critical points at most the minimum: every evaluation sits behind a wave-level
    // test (results unchanged: a candidate outside the interval was never taken).
    // (x >= lo && x <= hi rather than the reference's !(x < lo || x > hi): a NaN candidate, which the reference evaluates
    // to a NaN value that never wins, is simply not evaluated)
    const bool in0 = nr >= 1 && r0 >= lo && r0 <= hi, in1 = nr >= 2 && r1 >= lo && r1 <= hi;
    if (__any(in0)) { const double v = eval_poly_reg<nc>(poly, r0); if (in0 && v < opt_v) { opt_v = v; opt_x = r0; } }
    if (__any(in1)) { const double v = eval_poly_reg<nc>(poly, r1); if (in1 && v < opt_v) { opt_v = v; opt_x = r1; } }
    const bool inl = lower.x >= lo && lower.x <= hi, inc = current.x >= lo && current.x <= hi;
    if (__any(inl)) { const double v = eval_poly_reg<nc>(poly, lower.x); if (inl && v < opt_v) { opt_v = v; opt_x = lower.x; } }
    if (__any(inc)) { const double v = eval_poly_reg<nc>(poly, current.x); if (inc && v < opt_v) { opt_v = v; opt_x = current.x; } }
    step_size = opt_x;
    return true;
  }
  constexpr int nc = 6;
  // Quintic through {0: f0, g0; x1 = current; x2 = previous}: Hermite divided differences on the nodes 0, 0, x1, x1, x2, x2
  // and expansion of the Newton form. The reference solves the 6 x 6 Vandermonde system by full-pivot LU; against an
  // exact solve the divided differences are the more accurate of the two (argmin within 3e-15 vs 8e-12 relative,
  // tools/ — measured on 3000 random line searches), and they cost ~60 instructions instead of ~700 of select-based
  // pivoting.
  const double x1 = current.x, x2 = previous.x;
  if (x1 == 0.0 || x2 == 0.0 || x1 == x2) return false;
  const double r1 = fast_rcp(x1), r2 = fast_rcp(x2), r12 = fast_rcp(x2 - x1);
  const double d01 = (current.value - f0) * r1, d12 = (previous.value - current.value) * r12;
  const double e0 = (d01 - g0) * r1, e1 = (current.gradient - d01) * r1;
  const double e2 = (d12 - current.gradient) * r12, e3 = (previous.gradient - d12) * r12;
  const double h0 = (e1 - e0) * r1, h1 = (e2 - e1) * r2, h2 = (e3 - e2) * r12;
  const double k0 = (h1 - h0) * r2, k1 = (h2 - h1) * r2;
  const double m0 = (k1 - k0) * r2;
  const double x1s = x1 * x1;
  const double poly[nc] = {m0, k0 - m0 * (2.0 * x1 + x2), h0 - 2.0 * k0 * x1 + m0 * (x1s + 2.0 * x1 * x2),
                           e0 - h0 * x1 + k0 * x1s - m0 * x1s * x2, g0, f0};
  double dq[5];
#pragma unroll
  for (int i = 0; i < 5; ++i) dq[i] = (5 - i) * poly[i];
  if (dq[0] == 0.0) return false;  // degenerate leading coefficient: generic path
  opt_v = eval_poly_reg<nc>(poly, opt_x);
  const double vlo = eval_poly_reg<nc>(poly, lo);
  if (vlo < opt_v) { opt_v = vlo; opt_x = lo; }
  const double vhi = eval_poly_reg<nc>(poly, hi);
  if (vhi < opt_v) { opt_v = vhi; opt_x = hi; }
  double roots[4];
  quartic_roots_in_range_lanes(dq, lo, hi, roots);
  // (each candidate behind a wave-level test, as in the cubic case: roots[1..3] are NaN after the one-root shortcut)
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const double rt = roots[i];
    const bool in = rt >= lo && rt <= hi;
    if (__any(in)) { const double v = eval_poly_reg<nc>(poly, rt); if (in && v < opt_v) { opt_v = v; opt_x = rt; } }
  }
  const double sx[3] = {lower.x, current.x, previous.x};
#pragma unroll
  for (int smp = 0; smp < 3; ++smp) {
    const bool in = sx[smp] >= lo && sx[smp] <= hi;
    if (__any(in)) { const double v = eval_poly_reg<nc>(poly, sx[smp]); if (in && v < opt_v) { opt_v = v; opt_x = sx[smp]; } }
  }
  step_size = opt_x;
  return true;
}

// std::min(std::max(v, lo), hi) of parameter_block.h Plus(): a NaN stays a NaN (fmin / fmax alone would drop it and a
// NaN warm start would be solved from the lower bound instead of failing its initial evaluation like Ceres)
__device__ inline double clampd(double v, double lo, double hi) { return (v != v) ? v : fmin(fmax(v, lo), hi); }

// tf2 Quaternion::setRPY(0,0,yaw) followed by tf2::getYaw (x = y = 0): src/optimizer.cpp:434-439 round trips.
__device__ inline double yaw_roundtrip(double yaw) {
  double sz, cz;
  sincos(yaw * 0.5, &sz, &cz);
  return atan2(2.0 * (cz * sz), cz * cz - sz * sz);
}


// Armijo sufficient decrease of a line-search sample, the one expression both the sweep (does the
// sample need its whole Gram?) and the state machine (is the search over?) evaluate: explicit operations, so that the two
// sites cannot be contracted differently. A NaN value fails.
__device__ inline bool armijo_holds(double value, double cost, double gd0, double alpha) {
  return isfinite(value) && !(value > fma(1e-4 * gd0, alpha, cost));
}

enum Phase { PH_FETCH = 0, PH_INIT = 1, PH_LS = 2, PH_REEVAL = 3, PH_DONE = 4, PH_IDLE = 5 };

// Slot-uniform LM scalars parked in LDS (offsets into the scal[] block).
enum Scal { S_COST = 0, S_XNORM, S_GMAX, S_RADIUS, S_DECF, S_MCC, S_GD0, S_DIRMAX, S_PREV_X, S_PREV_V, S_PREV_G,
            S_CUR_X, S_CUR_V, S_CUR_G, S_INITIAL_COST, S_FIRST_V, S_COUNT };

// The state machine's flags, bits of LmRegs::flags: one word that is parked and fetched as it is (seven bools were packed
// and unpacked with shifts around every sweep).
enum LmFlag { LF_STEP_SUCCESSFUL = 1, LF_AT_LEAST_ONE = 2, LF_PREV_VV = 4, LF_PREV_GV = 8, LF_CUR_VV = 16, LF_CUR_GV = 32,
              LF_FIRST_VV = 64 };

struct LmRegs {  // slot-uniform integers / flags kept in registers
  int phase, iter, evals, num_invalid, ls_iters, n_samples, status, reason;
  int flags;  // LmFlag bits
  __device__ bool has(int f) const { return (flags & f) != 0; }
  __device__ void set(int f, bool v) { flags = v ? (flags | f) : (flags & ~f); }
  // flag `to` takes the value of flag `from`
  __device__ void copy(int to, int from) { set(to, has(from)); }
};

// 2^-e for a power of two d = 2^e within [2^-1021, 2^1022]: exact, so that x * pow2_reciprocal(d) is the correctly rounded
// x / d wherever that quotient is a normal number (the trust-region radius: within [1e-32, 1e16], divided by 2, 4, 8, ...)
__device__ inline double pow2_reciprocal(double d) {
  return __longlong_as_double(0x7fe0000000000000ll - __double_as_longlong(d));
}

}  // namespace smpc
