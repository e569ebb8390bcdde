// smpc_visibility_rule.hpp — the rule of the line-of-sight filter (include/smpc_visibility.h states the contract): the cell
// of a point, which cells occlude, the range gate, and the sight line between two cell centres over a cell accessor.
// Plain double arithmetic with one rounding per operation for the points, exact unsigned integer arithmetic for the ray;
// no HIP call, no include beyond <stdint.h>: the kernel (smpc_visibility.hpp) and a host-only program
// (tests/test_visibility.py) compile the same functions.
//
// The sight line in closed form. Let the major axis be the one with the larger cell distance M, the other distance
// m <= M, and count columns i = 0 .. M along the major axis and rows r = 0 .. m along the minor one, cell a = (0, 0),
// cell b = (M, m). The segment between the centres crosses the boundary between columns i and i + 1 at the height
// m * (2i + 1) / (2M) above a's centre, that is in row
//     r_i = (m * (2i + 1) + M) / (2M)                       (integer division; the dividend stays below 2^32 for M <= 32769)
// and, when the remainder is 0 and m > 0, exactly through the lattice corner below row r_i. Column i is entered in row
// r_(i-1) (column 0: row 0) and left in row r_i, or r_i - 1 at a corner; slope <= 1, so those are its only cells (at most
// two). At a corner the two cells that touch the segment only there are (i + 1, r_i - 1) and (i, r_i): they occlude as a
// pair. Column M holds b alone. Every column is independent of the others: that is what the kernel's lanes share out.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SMPC_VIS_HD __host__ __device__
#else
#define SMPC_VIS_HD
#endif

namespace smpc {

// seen codes (enum smpc_seen_code)
constexpr uint32_t kSeenHidden = 0u, kSeenSeen = 1u, kSeenOutOfRange = 2u, kSeenNotFinite = 3u;

struct VisOcc {
  uint32_t min_cost;  // cost >= min_cost occludes
  uint32_t unknown;   // ... 255 only when set
};

SMPC_VIS_HD inline bool vis_occludes(const VisOcc& o, uint32_t cost) { return cost >= o.min_cost && (cost != 255u || o.unknown != 0u); }

SMPC_VIS_HD inline bool vis_finite(double v) { return __builtin_fabs(v) <= 1.7976931348623157e308; }  // false for NaN and inf

// one axis: floor((p - origin) / res) as a double; a cell outside the world is legal
SMPC_VIS_HD inline double vis_cell_axis(double p, double origin, double res) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  const double d = p - origin;
  return __builtin_floor(d / res);
}

// the robot's cell; false: x or y is not finite, or |q| <= 2^30 fails on an axis (a NaN lands here too)
SMPC_VIS_HD inline bool vis_robot_cell(double rx, double ry, double ox, double oy, double res, int32_t* ax, int32_t* ay) {
  const double qx = vis_cell_axis(rx, ox, res), qy = vis_cell_axis(ry, oy, res);
  if (!(vis_finite(rx) && vis_finite(ry))) return false;
  if (!(__builtin_fabs(qx) <= 1073741824.0 && __builtin_fabs(qy) <= 1073741824.0)) return false;
  *ax = (int32_t)qx; *ay = (int32_t)qy;
  return true;
}

// ddx * ddx + ddy * ddy <= max_range * max_range: two products, a sum and a product, each rounded on its own
SMPC_VIS_HD inline bool vis_in_range(double rx, double ry, double px, double py, double max_range) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  const double ddx = px - rx, ddy = py - ry;
  const double xx = ddx * ddx, yy = ddy * ddy;
  const double d2 = xx + yy, r2 = max_range * max_range;
  return d2 <= r2;
}

// The ray from cell a to cell b: cell (column i, row r) is (ax + ux * i + vx * r, ay + uy * i + vy * r).
struct VisRay {
  int32_t ax, ay;
  int32_t ux, uy, vx, vy;
  uint32_t M, m;  // cell distance along the major and the minor axis, m <= M
};

SMPC_VIS_HD inline VisRay vis_ray(int32_t ax, int32_t ay, int32_t bx, int32_t by) {
  const int32_t ex = bx - ax, ey = by - ay;  // |cells| <= 2^30 + 32769: no overflow
  const uint32_t dx = (uint32_t)(ex < 0 ? -ex : ex), dy = (uint32_t)(ey < 0 ? -ey : ey);
  const int32_t sx = ex < 0 ? -1 : 1, sy = ey < 0 ? -1 : 1;
  VisRay r;
  r.ax = ax; r.ay = ay;
  if (dx >= dy) { r.ux = sx; r.uy = 0; r.vx = 0; r.vy = sy; r.M = dx; r.m = dy; }
  else          { r.ux = 0; r.uy = sy; r.vx = sx; r.vy = 0; r.M = dy; r.m = dx; }
  return r;
}

// Does column i (0 <= i < M) hide b: one of its cells other than a occludes, or both cells of the corner pair at its far
// boundary do. occ(x, y): does world cell (x, y) occlude (false outside the world).
template <typename Occ>
SMPC_VIS_HD inline bool vis_column(const VisRay& r, uint32_t i, Occ&& occ) {
  const uint32_t two_m = 2u * r.M;
  const uint32_t enter = i == 0u ? 0u : (r.m * (2u * i - 1u) + r.M) / two_m;
  const uint32_t t = r.m * (2u * i + 1u) + r.M;
  const uint32_t row = t / two_m;
  const bool corner = r.m != 0u && t - row * two_m == 0u;  // (then row >= 1)
  const uint32_t leave = corner ? row - 1u : row;
  const int32_t cx = r.ax + r.ux * (int32_t)i, cy = r.ay + r.uy * (int32_t)i;  // (column i, row 0)
  // `|` and `&`, not `||` and `&&`: which cells are tested depends on the ray alone, never on what a cell held (measured
  // on the MI355X: asking for all four cells unconditionally, to have their loads in flight together, was slower)
  bool hit = false;
  if (i != 0u || enter != 0u) hit = occ(cx + r.vx * (int32_t)enter, cy + r.vy * (int32_t)enter);
  if (leave != enter) hit = hit | occ(cx + r.vx * (int32_t)leave, cy + r.vy * (int32_t)leave);
  if (corner)
    hit = hit | (occ(cx + r.ux + r.vx * (int32_t)(row - 1u), cy + r.uy + r.vy * (int32_t)(row - 1u)) &
                 occ(cx + r.vx * (int32_t)row, cy + r.vy * (int32_t)row));
  return hit;
}

// the whole sight line, column after column
template <typename Occ>
SMPC_VIS_HD inline bool vis_hidden(const VisRay& r, Occ&& occ) {
  for (uint32_t i = 0u; i < r.M; ++i)
    if (vis_column(r, i, occ)) return true;
  return false;
}

}  // namespace smpc
