// smpc_collision_monitor_rule.hpp — the rule of the collision monitor (include/smpc_collision_monitor.h states the contract):
// the robot's cell, the point of a beam in the robot's frame, the two inside tests, the simulation step of the approach zones,
// the ratios and the scaled command, and the reach beyond which a point cannot matter to a zone. Plain double arithmetic with
// one rounding per operation, exact integer arithmetic for the cells; no HIP call, no include beyond <stdint.h> and, for the
// two headings, smpc_math.hpp: the kernel (smpc_collision_monitor.hpp) and a host-only program
// (tests/test_collision_monitor.py) compile the same functions.
#pragma once
#include <stdint.h>

#include "smpc_math.hpp"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SMPC_CM_HD __host__ __device__
#else
#define SMPC_CM_HD
#endif

namespace smpc {

constexpr int32_t kMonitorCircle = 0, kMonitorPolygon = 1;
constexpr int32_t kMonitorStop = 0, kMonitorSlowdown = 1, kMonitorLimit = 2, kMonitorApproach = 3;
constexpr int32_t kMonitorBadInput = 16, kMonitorNoCell = 32;  // the flags beside 1 << action of the deciding zone
constexpr int kMonitorMaxZones = 8, kMonitorMaxVertices = 16, kMonitorMaxSteps = 32;

// A zone as the kernel and the host-only program read it: the caller's smpc_monitor_zone with the circle's squared radius
// and the radius of the disc around the robot that holds the zone (cm_bound) formed once.
struct MonitorZone {
  int32_t shape, action, n, min_points;
  double radius2, slowdown_ratio, linear_limit, angular_limit, bound;
  double vx[kMonitorMaxVertices], vy[kMonitorMaxVertices];
};

SMPC_CM_HD inline bool cm_finite(double v) { return __builtin_fabs(v) <= 1.7976931348623157e308; }  // false for NaN and inf

// step 2: cosine and sine of an angle, as smpc_plant.h rule 4 obtains them (t: a MathTab)
template <class TabP>
SMPC_CM_HD inline void cm_heading(TabP t, double theta, double* c, double* s) {
  if (__builtin_expect(!(__builtin_fabs(theta) <= 1e5), 0)) {
#if defined(__HIP_DEVICE_COMPILE__)
    sincos(theta, s, c);
#else
    *s = sin(theta); *c = cos(theta);
#endif
  } else {
    sincos_tab(t, theta, s, c);
  }
}

// step 2: the angle of one simulation step, w * sim_dt
SMPC_CM_HD inline double cm_step_angle(double w, double sim_dt) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  return w * sim_dt;
}

// step 3: the robot's cell, as smpc_sensed_costmap.h rule 1; false: x or y is not finite, or |q| <= 2^30 fails on an axis
SMPC_CM_HD inline bool cm_robot_cell(double x, double y, double ox, double oy, double res, int32_t* ax, int32_t* ay) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  const double dx = x - ox, dy = y - oy;
  const double qx = __builtin_floor(dx / res), qy = __builtin_floor(dy / res);
  if (!(cm_finite(x) && cm_finite(y))) return false;
  if (!(__builtin_fabs(qx) <= 1073741824.0 && __builtin_fabs(qy) <= 1073741824.0)) return false;  // a NaN lands here too
  *ax = (int32_t)qx; *ay = (int32_t)qy;
  return true;
}

// step 3: does a beam of this kind give a point? WORLD, AGENT, CORNER_PAIR
SMPC_CM_HD inline bool cm_is_hit(uint32_t kind) { return kind >= 1u && kind <= 3u; }

// step 3, one axis: the centre of cell a + off (|a| <= 2^30, off any int32: the sum is exact) minus the robot's coordinate
SMPC_CM_HD inline double cm_rel(double origin, int32_t a, int32_t off, double res, double x) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  const double i = (double)((int64_t)a + (int64_t)off);
  const double h = i + 0.5;
  const double m = h * res;
  const double centre = origin + m;
  return centre - x;
}

// steps 3 and 5: (c * rx + s * ry, c * ry - s * rx)
SMPC_CM_HD inline void cm_to_frame(double c, double s, double rx, double ry, double* px, double* py) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  const double a = c * rx, b = s * ry, d = c * ry, e = s * rx;
  *px = a + b;
  *py = d - e;
}

// step 5: the point of step m >= 1 in the frame of the simulated pose
SMPC_CM_HD inline void cm_step_point(double px, double py, double X, double Y, double C, double S, double* qx, double* qy) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  const double dx = px - X, dy = py - Y;
  cm_to_frame(C, S, dx, dy, qx, qy);
}

// step 5: one simulation step of the pose
SMPC_CM_HD inline void cm_advance(double v, double sim_dt, double c1, double s1, double* X, double* Y, double* C, double* S) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  const double vc = v * *C, vs = v * *S;
  const double ax = vc * sim_dt, ay = vs * sim_dt;
  *X = *X + ax;
  *Y = *Y + ay;
  const double cc = *C * c1, ss = *S * s1, sc = *S * c1, cs = *C * s1;
  *C = cc - ss;
  *S = sc + cs;
}

SMPC_CM_HD inline double cm_radius2(double radius) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  return radius * radius;
}

// step 4: the circle
SMPC_CM_HD inline bool cm_in_circle(double qx, double qy, double radius2) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  const double xx = qx * qx, yy = qy * qy;
  return xx + yy < radius2;
}

// step 4: does edge (Vj -> Vi) count for the parity of q?
SMPC_CM_HD inline bool cm_edge_counts(double vix, double viy, double vjx, double vjy, double qx, double qy) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  if ((viy > qy) == (vjy > qy)) return false;
  const double dy = vjy - viy, ex = vjx - vix;
  const double a = ex * (qy - viy), b = (qx - vix) * dy;
  const double t = a - b;
  return dy > 0.0 ? t > 0.0 : (dy < 0.0 && t < 0.0);
}

// step 4: the polygon, edge after edge (the kernel walks the edges outside and its points inside: the same parities)
template <class ZoneP>
SMPC_CM_HD inline bool cm_in_polygon(ZoneP z, double qx, double qy) {
  const int n = z->n;
  bool in = false;
  double vjx = z->vx[n - 1], vjy = z->vy[n - 1];
  for (int i = 0; i < n; ++i) {
    const double vix = z->vx[i], viy = z->vy[i];
    in ^= cm_edge_counts(vix, viy, vjx, vjy, qx, qy);
    vjx = vix; vjy = viy;
  }
  return in;
}

// step 5: m / M as doubles
SMPC_CM_HD inline double cm_step_ratio(int m, int M) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  return (double)m / (double)M;
}

// step 6: a triggered LIMIT zone
SMPC_CM_HD inline double cm_limit_ratio(double v, double w, double linear_limit, double angular_limit) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  const double av = __builtin_fabs(v), aw = __builtin_fabs(w);
  double r = 1.0;
  if (av > linear_limit) { const double q = linear_limit / av; r = q < r ? q : r; }
  if (aw > angular_limit) { const double q = angular_limit / aw; r = q < r ? q : r; }
  return r;
}

// step 6: one component of the command out; ratio in [0, 1]
SMPC_CM_HD inline double cm_scale(double u, double ratio) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  if (ratio == 1.0) return u;
  if (ratio == 0.0) return 0.0;
  return u * ratio;
}

// The disc around the robot that holds a zone: the circle's radius, the largest |vertex| of a polygon (the correctly rounded
// square root of a sum that is off by two roundings: cm_reach2 adds a margin far above that).
SMPC_CM_HD inline double cm_bound(int32_t shape, double radius, int n, const double* vx, const double* vy) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  if (shape == kMonitorCircle) return radius;
  double m = 0.0;
  for (int i = 0; i < n; ++i) {
    const double xx = vx[i] * vx[i], yy = vy[i] * vy[i];
    const double d2 = xx + yy;
    m = d2 > m ? d2 : m;
  }
  return __builtin_sqrt(m);
}

// The squared reach of a zone: a point p with px^2 + py^2 above it is outside the zone at every step 0..M. At step m the
// simulated robot has moved at most m * |v| * sim_dt (up to rounding), so the point's distance from it is at least
// |p| - M |v| sim_dt, and a point inside the zone is within `bound` of it. The factor and the constant are far above every
// rounding error of steps 3 to 5 (relative 1e-14 after 32 rotations) and far below a cell.
SMPC_CM_HD inline double cm_reach2(double bound, double v, int M, double sim_dt) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  const double travel = M > 0 ? (__builtin_fabs(v) * (double)M) * sim_dt : 0.0;
  const double reach = (bound + travel) * 1.000001 + 1e-9;
  return reach * reach;
}

SMPC_CM_HD inline bool cm_within_reach(double px, double py, double reach2) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  const double xx = px * px, yy = py * py;
  return xx + yy <= reach2;  // false for a NaN: such a point is never inside either
}

}  // namespace smpc
