// smpc_scan_people_rule.hpp — the rule of the scan-based people detector (include/smpc_scan_people.h states the contract):
// the robot's cell, the foreground test of a beam, the link between neighbouring hits, the gates of a segment and the position
// of an accepted one. Exact integer arithmetic up to the position, there plain double arithmetic with one rounding per
// operation; no HIP call, no include beyond <stdint.h>: the kernel (smpc_scan_people.hpp) and a host-only program
// (tests/test_scan_people.py) compile the same functions.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SMPC_SP_HD __host__ __device__
#else
#define SMPC_SP_HD
#endif

namespace smpc {

constexpr int32_t kScanAccepted = 0, kScanByPoints = 1, kScanByWidth = 2;  // sp_gate

SMPC_SP_HD inline bool sp_finite(double v) { return __builtin_fabs(v) <= 1.7976931348623157e308; }  // false for NaN and inf

// step 1: the robot's cell, as smpc_sensed_costmap.h rule 1; false: x or y is not finite, or |q| <= 2^30 fails on an axis
SMPC_SP_HD inline bool sp_robot_cell(double x, double y, double ox, double oy, double res, int32_t* ax, int32_t* ay) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  const double dx = x - ox, dy = y - oy;
  const double qx = __builtin_floor(dx / res), qy = __builtin_floor(dy / res);
  if (!(sp_finite(x) && sp_finite(y))) return false;
  if (!(__builtin_fabs(qx) <= 1073741824.0 && __builtin_fabs(qy) <= 1073741824.0)) return false;  // a NaN lands here too
  *ax = (int32_t)qx; *ay = (int32_t)qy;
  return true;
}

// x * x + y * y of two int32, exact: at most 2^63, so unsigned
SMPC_SP_HD inline uint64_t sp_norm2(int32_t x, int32_t y) {
  const int64_t lx = x, ly = y;
  return (uint64_t)(lx * lx) + (uint64_t)(ly * ly);
}

// step 2: is this beam foreground? AGENT, CORNER_PAIR, WORLD without map subtraction; within the range
SMPC_SP_HD inline bool sp_foreground(uint32_t kind, int32_t subtract_map, int32_t ox, int32_t oy, int32_t range_d2) {
  const bool hit = kind == 2u || kind == 3u || (kind == 1u && subtract_map == 0);
  return hit && sp_norm2(ox, oy) <= (uint64_t)range_d2;
}

// steps 3 and 5: the squared cell distance of two foreground hits (|o| <= sqrt(2^31) each: the differences fit 32 bits)
SMPC_SP_HD inline int64_t sp_dist2(int32_t ax, int32_t ay, int32_t bx, int32_t by) {
  const int64_t dx = (int64_t)ax - (int64_t)bx, dy = (int64_t)ay - (int64_t)by;
  return dx * dx + dy * dy;
}

// step 3: are two foreground neighbours linked?
SMPC_SP_HD inline bool sp_linked(int32_t ox, int32_t oy, int32_t px, int32_t py, int32_t link_d2) {
  return sp_dist2(ox, oy, px, py) <= (int64_t)link_d2;
}

// step 6
SMPC_SP_HD inline int32_t sp_gate(int32_t m, int64_t chord, int32_t min_points, int32_t width_d2_min, int32_t width_d2_max) {
  if (m < min_points) return kScanByPoints;
  if (chord < (int64_t)width_d2_min || chord > (int64_t)width_d2_max) return kScanByWidth;
  return kScanAccepted;
}

// step 7, one axis: the centre of the segment's mean cell
SMPC_SP_HD inline double sp_centre(int32_t S, int32_t m, int32_t a, double origin, double res) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  const double mean = (double)S / (double)m;
  const double i = (double)a + mean;
  const double h = i + 0.5;
  const double w = h * res;
  return origin + w;
}

// step 7: the centre pushed back along the sight line
SMPC_SP_HD inline void sp_position(double cx, double cy, double x, double y, double body_offset, double* px, double* py) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  const double rx = cx - x, ry = cy - y;
  const double xx = rx * rx, yy = ry * ry;
  const double d = __builtin_sqrt(xx + yy);
  *px = cx; *py = cy;
  if (body_offset > 0.0 && sp_finite(d) && d > 0.0) {
    const double k = body_offset / d;
    const double ux = rx * k, uy = ry * k;
    *px = cx + ux; *py = cy + uy;
  }
}

}  // namespace smpc
