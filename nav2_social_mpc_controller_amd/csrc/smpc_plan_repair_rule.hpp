// smpc_plan_repair_rule.hpp — the rule of the plan repair (include/smpc_plan_repair.h states the contract): the distance
// between two points, the order of the closest-pose keys, a pose's cell in the region and what it means for the stretch in
// view, a region cell's weight, one cell's relaxation and one probe of the walk on the region's haloed arrays, and the length
// of the spliced plan. Costs, neighbour table, diagonal test, cell of a point and centre of a cell are those of
// smpc_global_plan_rule.hpp, included, not copied. Plain double arithmetic with one rounding per operation, integer
// arithmetic for the rest; no HIP call, no include beyond <stdint.h> and that header: the kernels (smpc_plan_repair.hpp) and
// a host-only program (tests/test_plan_repair.py) compile the same functions.
#pragma once
#include <stdint.h>

#include "smpc_global_plan_rule.hpp"

namespace smpc {

constexpr int kRepairMaxRadius = 63;

// enum smpc_repair_status, and the value a robot carries from the judging kernel to the field kernel
constexpr int32_t kRepairPending = -1, kRepairClear = 0, kRepairRepaired = 1, kRepairNoPlan = 2, kRepairNoCell = 3, kRepairNoRejoin = 4,
                  kRepairUnreachable = 5, kRepairTooLong = 6, kRepairInconsistent = 7;

// what a pose of the stretch in view is
constexpr int kPoseOutOfView = 0, kPoseBlocked = 1, kPosePassable = 2, kPoseOwnCell = 3;  // own cell: impassable, yet not blocked

struct PrWindow {
  double ox, oy, res;   // the window's origin and resolution
  int32_t sx, sy;       // its size in cells
};

// d2(p, q): two differences, two products, one sum
SMPC_GP_HD inline double pr_d2(double px, double py, double qx, double qy) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  const double dx = px - qx;
  const double dy = py - qy;
  const double a = dx * dx;
  const double b = dy * dy;
  return a + b;
}

SMPC_GP_HD inline bool pr_finite(double v) {
  uint64_t u;
  __builtin_memcpy(&u, &v, sizeof(u));
  return (u & 0x7FF0000000000000ull) != 0x7FF0000000000000ull;
}

// does candidate (valid a, da, ia) come before (valid b, db, ib)? The least d2 wins, then the least index; a key that is not
// valid (a d2 that is not finite, or no pose at all) never wins.
SMPC_GP_HD inline bool pr_closer(bool va, double da, int32_t ia, bool vb, double db, int32_t ib) {
  if (!va) return false;
  if (!vb) return true;
  return da < db || (da == db && ia < ib);
}

// the cell of a point, when it has one in the region around (ax, ay)
SMPC_GP_HD inline bool pr_region_cell(const PrWindow& w, double px, double py, int32_t ax, int32_t ay, int32_t R, int32_t* cx, int32_t* cy) {
  if (!gp_cell_axis(px, w.ox, w.res, w.sx, cx)) return false;
  if (!gp_cell_axis(py, w.oy, w.res, w.sy, cy)) return false;
  const int32_t dx = *cx - ax, dy = *cy - ay;
  return dx >= -R && dx <= R && dy >= -R && dy <= R;
}

// a pose of the stretch whose cell, in the region, costs v
SMPC_GP_HD inline int pr_pose_class(const GpCost& c, uint32_t v, bool own_cell) {
  if (gp_passable(c, v)) return kPosePassable;
  return own_cell ? kPoseOwnCell : kPoseBlocked;
}

// w(c) of a region cell; the robot's own cell counts as passable whatever its cost. 0: impassable.
SMPC_GP_HD inline uint32_t pr_weight(const GpCost& c, uint32_t v, bool own_cell) {
  return own_cell ? (uint32_t)c.neutral + (uint32_t)c.weight * v : gp_weight(c, v);
}

// The region lives in two arrays of (S + 2) x (S + 2) cells, `pitch` = S + 2 apart per row: potentials f and weights w, the
// rim a halo of weight 0 and potential kFieldUnreachable, so no probe needs a bounds test.
SMPC_GP_HD inline int pr_offset(int k, int pitch) { return gp_dy(k) * pitch + gp_dx(k); }

// One relaxation of cell idx: min over its allowed steps of f(n) + k w(n), when that is below what the cell holds and not
// above `cap` (the current F of the robot's cell: a cell above it cannot lie on the walk). Returns the cell's new value.
template <typename F, typename W>
SMPC_GP_HD inline uint32_t pr_relax(const F* f, const W* w, int idx, int pitch, uint32_t cap) {
  const uint32_t cur = f[idx];
  if (w[idx] == 0) return cur;
  uint32_t best = cur;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int dx = gp_dx(k), dyp = gp_dy(k) * pitch;
    const uint32_t sc = gp_step_cost(k, w[idx + dyp + dx], w[idx + dx], w[idx + dyp]);
    const uint32_t fn = f[idx + dyp + dx];
    const uint32_t cand = fn + sc;  // below the marker whenever it counts (the host's bound)
    best = (sc != 0u && fn != kFieldUnreachable && cand < best && cand <= cap) ? cand : best;
  }
  return best;
}

// Is neighbour k of cell idx the next cell of the walk?
template <typename F, typename W>
SMPC_GP_HD inline bool pr_walk_probe(const F* f, const W* w, int idx, int pitch, int k) {
  const int dx = gp_dx(k), dyp = gp_dy(k) * pitch;
  const uint32_t sc = gp_step_cost(k, w[idx + dyp + dx], w[idx + dx], w[idx + dyp]);
  const uint32_t fn = f[idx + dyp + dx];
  return sc != 0u && fn != kFieldUnreachable && fn + sc == f[idx];
}

// rule 10: what the field output holds for a cell of potential v
SMPC_GP_HD inline uint32_t pr_field_out(uint32_t v, uint32_t fa) { return v <= fa ? v : kFieldUnreachable; }

// rows of the spliced plan: i0 kept, the robot, K centres, the old rows j .. n - 1
SMPC_GP_HD inline int64_t pr_new_length(int32_t i0, int32_t K, int32_t n, int32_t j) { return (int64_t)i0 + 1 + (int64_t)K + ((int64_t)n - (int64_t)j); }

}  // namespace smpc
