// smpc_local_costmap_rule.hpp — where a robot's rolling costmap window sits: the cell rule of smpc_local_costmap_batch
// (include/smpc_local_costmap.h states the contract). Nav2's LayeredCostmap::updateMap asks for the origin
// robot - getSizeInMeters / 2 and Costmap2D::updateOrigin moves the window by the whole cells of the difference (a cast to
// int: truncation toward zero); here the window is kept as the integer world cell of its cell (0,0), so the origin is
// derived from it every time and never accumulated. Plain double arithmetic, one rounding per operation; no HIP call, no
// include beyond <stdint.h>: the kernel (smpc_local_costmap.hpp) and a host-only program (tests/test_local_costmap.py)
// compile the same function.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SMPC_LC_HD __host__ __device__
#else
#define SMPC_LC_HD
#endif

namespace smpc {

constexpr double kLcCellLimit = 1073741824.0;  // 2^30: cell + window size stays an int32_t

// origin of the window whose cell (0,0) is world cell `cell`, one axis: the product, then the sum
SMPC_LC_HD inline double lc_origin(double w0, int32_t cell, double res) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  const double m = (double)cell * res;
  return w0 + m;
}

// one axis: the cell after the update for a finite pose coordinate
SMPC_LC_HD inline int32_t lc_roll_axis(double w0, int32_t cell, double res, int32_t size, double pose) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  const double o = lc_origin(w0, cell, res);
  const double half = (((double)(size - 1) + 0.5) * res) / 2.0;
  const double want = pose - half;
  const double d = __builtin_trunc((want - o) / res);
  double c = (double)cell + d;
  c = c > kLcCellLimit ? kLcCellLimit : c;
  c = c >= -kLcCellLimit ? c : -kLcCellLimit;  // (a NaN, from an origin that is not finite, lands here too)
  return (int32_t)c;
}

struct LcRoll {
  int32_t cx, cy;  // the cell after the update
  int32_t moved;   // smpc_local_costmap_batch's moved[b]: 0 kept, 1 moved (or forced), 2 pose not finite (kept)
  bool write;      // cell, window and origin are written
};

// The update of one robot. `force`: the stored cell is taken as (0,0) and the robot is written whatever comes out.
SMPC_LC_HD inline LcRoll lc_roll(double w0x, double w0y, int32_t cell_x, int32_t cell_y, double res, int32_t size_x, int32_t size_y,
                                 double pose_x, double pose_y, bool force) {
  if (force) cell_x = cell_y = 0;
  LcRoll r;
  r.cx = cell_x; r.cy = cell_y;
  if (!(__builtin_isfinite(pose_x) && __builtin_isfinite(pose_y))) {
    r.moved = 2; r.write = force;
    return r;
  }
  r.cx = lc_roll_axis(w0x, cell_x, res, size_x, pose_x);
  r.cy = lc_roll_axis(w0y, cell_y, res, size_y, pose_y);
  r.write = force || r.cx != cell_x || r.cy != cell_y;
  r.moved = r.write ? 1 : 0;
  return r;
}

}  // namespace smpc
