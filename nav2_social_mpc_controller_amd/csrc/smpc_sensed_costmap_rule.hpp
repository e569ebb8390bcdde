// smpc_sensed_costmap_rule.hpp — the rule of the sensed local costmaps (include/smpc_sensed_costmap.h states the contract):
// which agents have a cell, one beam's first hit over a cell accessor, where a hit lands in the window, the distance to the
// nearest mark of a row from the row's bit mask, and a cell's cost. Exact integer arithmetic throughout; the cell of a point
// is smpc_visibility_rule.hpp's. No HIP call, no include beyond that header and <stdint.h>: the kernel
// (smpc_sensed_costmap.hpp) and a host-only program (tests/test_sensed_costmap.py) compile the same functions.
//
// A beam in closed form, column by column (the header of smpc_visibility_rule.hpp derives the columns): with M >= m the cell
// distances along the major and the minor axis, column i = 0 .. M - 1 is entered in row r_(i-1) (column 0: row 0, the
// robot's own cell) and left in row r_i = (m * (2i + 1) + M) / (2M), or r_i - 1 when the remainder is 0 and m > 0: the
// segment then leaves through a lattice corner, and the cells (i + 1, r_i - 1) and (i, r_i) are tested as a pair. Column M
// holds the end cell alone. The walk of the contract visits exactly these cells in exactly this order: entry cell, exit
// cell, pair, next column. r_i and the remainder are carried from column to column (one add and one compare: 2m <= 2M),
// so there is no division.
#pragma once
#include <stdint.h>

#include "smpc_visibility_rule.hpp"

namespace smpc {

// enum smpc_beam_kind
constexpr uint32_t kBeamNone = 0u, kBeamWorld = 1u, kBeamAgent = 2u, kBeamCornerPair = 3u, kBeamInvalid = 4u, kBeamNoRobot = 5u;
constexpr int32_t kSensedReach = 127;      // SMPC_SENSED_MAX_REACH
constexpr uint32_t kSensedNoGap = 255u;    // sc_row_gap: no mark within r

// agent rows: the cell of a person with finite x, y and |q| <= 2^30 on both axes (the same test as the robot's)
SMPC_VIS_HD inline bool sc_agent_cell(double px, double py, double ox, double oy, double res, int32_t* qx, int32_t* qy) {
  return vis_robot_cell(px, py, ox, oy, res, qx, qy);
}

SMPC_VIS_HD inline bool sc_beam_valid(int32_t ex, int32_t ey) {
  return ex >= -kSensedReach && ex <= kSensedReach && ey >= -kSensedReach && ey <= kSensedReach;
}

struct ScHit {
  uint32_t kind;     // NONE, WORLD, AGENT or CORNER_PAIR
  int32_t ox, oy;    // the hit's offset from a (a pair: the cell that stepped along x); NONE: the end offset
  int32_t px, py;    // CORNER_PAIR: the other hit's offset
};

// One valid beam from a to a + (ex, ey). stops(ox, oy): 0, kBeamWorld or kBeamAgent for the cell at offset (ox, oy) from a;
// it is asked for offsets within the reach square only, and never for (0, 0).
template <typename Stops>
SMPC_VIS_HD inline ScHit sc_cast(int32_t ex, int32_t ey, Stops&& stops) {
  const VisRay ray = vis_ray(0, 0, ex, ey);  // columns along the major axis: cell (i, r) is offset (ux * i + vx * r, uy * i + vy * r)
  const int32_t M = (int32_t)ray.M, m = (int32_t)ray.m;
  const bool x_major = ray.ux != 0;
  ScHit h;
  h.kind = kBeamNone; h.ox = ex; h.oy = ey; h.px = ex; h.py = ey;
  int32_t enter = 0;
  int32_t row = 0, rem = m + M;  // m * (2i + 1) + M = row * 2M + rem at i = 0
  if (rem >= 2 * M && M > 0) { rem -= 2 * M; row = 1; }
  for (int32_t i = 0; i < M; ++i) {
    const bool corner = m != 0 && rem == 0;
    const int32_t leave = corner ? row - 1 : row;
    const int32_t cx = ray.ux * i, cy = ray.uy * i;  // (column i, row 0)
    if (i != 0) {
      const uint32_t k = stops(cx + ray.vx * enter, cy + ray.vy * enter);
      if (k != 0u) { h.kind = k; h.ox = cx + ray.vx * enter; h.oy = cy + ray.vy * enter; return h; }
    }
    if (leave != enter) {
      const uint32_t k = stops(cx + ray.vx * leave, cy + ray.vy * leave);
      if (k != 0u) { h.kind = k; h.ox = cx + ray.vx * leave; h.oy = cy + ray.vy * leave; return h; }
    }
    if (corner) {
      const int32_t nx = cx + ray.ux + ray.vx * (row - 1), ny = cy + ray.uy + ray.vy * (row - 1);  // (i + 1, row - 1): stepped along the major axis
      const int32_t sx = cx + ray.vx * row, sy = cy + ray.vy * row;                                // (i, row): stepped along the minor axis
      if (stops(nx, ny) != 0u && stops(sx, sy) != 0u) {
        h.kind = kBeamCornerPair;
        h.ox = x_major ? nx : sx; h.oy = x_major ? ny : sy;
        h.px = x_major ? sx : nx; h.py = x_major ? sy : ny;
        return h;
      }
    }
    enter = row;
    rem += 2 * m;
    if (rem >= 2 * M) { rem -= 2 * M; ++row; }
  }
  if (M > 0) {
    const uint32_t k = stops(ex, ey);
    if (k != 0u) h.kind = k;
  }
  return h;
}

// the window cell of the hit at offset (ox, oy) from a; false: outside the window (64-bit: `cell` is any int32)
SMPC_VIS_HD inline bool sc_window_cell(int32_t ax, int32_t ay, int32_t ox, int32_t oy, int32_t cell_x, int32_t cell_y, int32_t size_x,
                                       int32_t size_y, int32_t* wx, int32_t* wy) {
  const int64_t x = (int64_t)ax + ox - cell_x, y = (int64_t)ay + oy - cell_y;
  if (x < 0 || x >= size_x || y < 0 || y >= size_y) return false;
  *wx = (int32_t)x; *wy = (int32_t)y;
  return true;
}

// The distance from cell x to the nearest marked cell of its row, from the row's bit mask: bit t of `v` is cell x - 32 + t
// (t = 0 .. 63) and `far` is cell x + 32. kSensedNoGap when there is none within r (r <= 32). Two bit scans, not a search.
SMPC_VIS_HD inline uint32_t sc_row_gap(uint64_t v, uint32_t far, uint32_t r) {
  const uint64_t left = v & 0x1FFFFFFFFull;                              // cells x - 32 .. x, nearest at the top
  const uint64_t right = (v >> 32) | ((uint64_t)(far & 1u) << 32);       // cells x .. x + 32, nearest at the bottom
  const uint32_t dl = left != 0ull ? (uint32_t)__builtin_clzll(left) - 31u : kSensedNoGap;
  const uint32_t dr = right != 0ull ? (uint32_t)__builtin_ctzll(right) : kSensedNoGap;
  const uint32_t g = dl < dr ? dl : dr;
  return g <= r ? g : kSensedNoGap;
}

// the least d2 over the rows so far: a row at vertical distance dy whose nearest mark is `gap` cells away along the row
SMPC_VIS_HD inline uint32_t sc_least_d2(uint32_t best, uint32_t gap, uint32_t dy2) {
  const uint32_t d2 = gap * gap + dy2;  // kSensedNoGap: 65025 + dy2, beyond every d2_max
  return d2 < best ? d2 : best;
}

constexpr uint32_t kSensedNoMark = 0xFFFFFFu;  // sc_least_d2's start value

SMPC_VIS_HD inline uint32_t sc_cost(uint32_t d2, const uint8_t* table, uint32_t d2_max) { return d2 <= d2_max ? (uint32_t)table[d2] : 0u; }

}  // namespace smpc
