// smpc_obstacle_memory_rule.hpp — the rule of the sensed local costmaps with memory (include/smpc_obstacle_memory.h states
// the contract): one beam's first hit AND the cells it passes, the roll of one word of the mark bitmap, the marking range and
// the footprint. Exact integer arithmetic throughout. No HIP call, no include beyond the existing rule headers and
// <stdint.h>: the kernel (smpc_obstacle_memory.hpp) and a host-only program (tests/test_obstacle_memory.py) compile the same
// functions. sc_cast and smpc_sensed_costmap_rule.hpp stay as they are; om_cast is sc_cast's sibling.
#pragma once
#include <stdint.h>

#include "smpc_sensed_costmap_rule.hpp"

namespace smpc {

// One valid beam from a to a + (ex, ey), column by column in sc_cast's closed form (the header of
// smpc_sensed_costmap_rule.hpp), with the same hit. pass(ox, oy) is called for every cell the beam passes (rule 3 of the
// contract): a itself, then each cell that was entered, tested and did not stop the beam, in the order of the walk. In a
// column at most two cells are entered (leave - enter <= 1); the two cells of a corner pair are tested but never passed.
// stops(ox, oy) as sc_cast's: offsets within the reach square only, never (0, 0).
template <typename Stops, typename Pass>
SMPC_VIS_HD inline ScHit om_cast(int32_t ex, int32_t ey, Stops&& stops, Pass&& pass) {
  const VisRay ray = vis_ray(0, 0, ex, ey);
  const int32_t M = (int32_t)ray.M, m = (int32_t)ray.m;
  const bool x_major = ray.ux != 0;
  ScHit h;
  h.kind = kBeamNone; h.ox = ex; h.oy = ey; h.px = ex; h.py = ey;
  pass(0, 0);
  int32_t enter = 0;
  int32_t row = 0, rem = m + M;  // m * (2i + 1) + M = row * 2M + rem at i = 0
  if (rem >= 2 * M && M > 0) { rem -= 2 * M; row = 1; }
  for (int32_t i = 0; i < M; ++i) {
    const bool corner = m != 0 && rem == 0;
    const int32_t leave = corner ? row - 1 : row;
    const int32_t cx = ray.ux * i, cy = ray.uy * i;  // (column i, row 0)
    if (i != 0) {
      const int32_t qx = cx + ray.vx * enter, qy = cy + ray.vy * enter;
      const uint32_t k = stops(qx, qy);
      if (k != 0u) { h.kind = k; h.ox = qx; h.oy = qy; return h; }
      pass(qx, qy);
    }
    if (leave != enter) {
      const int32_t qx = cx + ray.vx * leave, qy = cy + ray.vy * leave;
      const uint32_t k = stops(qx, qy);
      if (k != 0u) { h.kind = k; h.ox = qx; h.oy = qy; return h; }
      pass(qx, qy);
    }
    if (corner) {
      const int32_t nx = cx + ray.ux + ray.vx * (row - 1), ny = cy + ray.uy + ray.vy * (row - 1);  // (i + 1, row - 1)
      const int32_t sx = cx + ray.vx * row, sy = cy + ray.vy * row;                                // (i, row)
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
    else pass(ex, ey);
  }
  return h;
}

// rule 4: is a hit at offset (ox, oy) from a (|.| <= 127) within the marking range?
SMPC_VIS_HD inline bool om_in_mark_range(int32_t ox, int32_t oy, int32_t mark_d2) { return ox * ox + oy * oy <= mark_d2; }

// rule 5: does the window cell at offset (i, j) from a lie under the footprint? 64-bit offsets: `cell` is any int32. An
// offset beyond 46340 on an axis is beyond every footprint_d2 < 2^31, which keeps the squares within 64 bits.
SMPC_VIS_HD inline bool om_in_footprint(int64_t i, int64_t j, int32_t footprint_d2) {
  if (footprint_d2 < 0 || i < -46340 || i > 46340 || j < -46340 || j > 46340) return false;
  return i * i + j * j <= (int64_t)footprint_d2;
}

// the bits of word w of a bitmap row that are cells of a window size_x wide (0: the word lies beyond the row)
SMPC_VIS_HD inline uint32_t om_word_mask(int32_t size_x, int32_t w) {
  const int64_t left = (int64_t)size_x - 32 * (int64_t)w;
  return left >= 32 ? 0xFFFFFFFFu : (left <= 0 ? 0u : (1u << (uint32_t)left) - 1u);
}

// rule 2: the shift of one axis, s = old corner - new corner, compared in 64 bits before anything is formed from it: a
// shift of 256 cells or more (SMPC_SENSED_MAX_SIZE: no window is wider) drops every bit, whichever way and however far, and
// is reported as +-256; every other shift is itself. The result is a small 32-bit number.
SMPC_VIS_HD inline int32_t om_shift(int32_t old_cell, int32_t new_cell) {
  const int64_t s = (int64_t)old_cell - (int64_t)new_cell;
  return s <= -256 ? -256 : (s >= 256 ? 256 : (int32_t)s);
}

// rule 2, rows: the old window row that lands in row y under the shift sy (om_shift's); false: none does
SMPC_VIS_HD inline bool om_roll_row(int32_t sy, int32_t size_y, int32_t y, int32_t* src_y) {
  if (sy <= -size_y || sy >= size_y) return false;
  const int32_t yy = y - sy;  // |.| < 512
  if (yy < 0 || yy >= size_y) return false;
  *src_y = yy;
  return true;
}

// rule 2, columns: destination word w of a row is (src[hi] << sh) | (src[hi - 1] >> (32 - sh)) of the old row: old cell x
// lands in x + sx (om_shift's). false: |sx| >= size_x, every bit is dropped. hi and hi - 1 may lie outside the row (the
// caller reads zero there, and masks every source word with om_word_mask).
struct OmRoll {
  int32_t hi;    // index of the source word whose low bits land in the high bits of the destination
  uint32_t sh;   // 0 .. 31
};

SMPC_VIS_HD inline bool om_roll_source(int32_t sx, int32_t size_x, int32_t w, OmRoll* r) {
  if (sx <= -size_x || sx >= size_x) return false;  // size_x <= 256: |sx| < 256 from here on
  const int32_t q = (sx + 256) / 32 - 8;            // floor(sx / 32)
  r->hi = w - q;
  r->sh = (uint32_t)(sx - 32 * q);
  return true;
}

// The robot's window cell on one axis, a - cell in 64 bits (`cell` is any int32), cut to +-2^20: a window cell is
// rel + offset with |offset| <= 127, and beyond 2^20 - 127 that lies outside every window (side <= 256) either way.
SMPC_VIS_HD inline int32_t om_window_rel(int32_t a, int32_t cell) {
  const int64_t d = (int64_t)a - (int64_t)cell;
  return d < -1048576 ? -1048576 : (d > 1048576 ? 1048576 : (int32_t)d);
}

// the window cell of offset (ox, oy) from a, as sc_window_cell gives it, from om_window_rel's values; false: outside
SMPC_VIS_HD inline bool om_window_cell(int32_t rel_x, int32_t rel_y, int32_t ox, int32_t oy, int32_t size_x, int32_t size_y, int32_t* wx,
                                       int32_t* wy) {
  const int32_t x = rel_x + ox, y = rel_y + oy;
  if ((uint32_t)x >= (uint32_t)size_x || (uint32_t)y >= (uint32_t)size_y) return false;
  *wx = x; *wy = y;
  return true;
}

// no word is shifted by 32 or more
SMPC_VIS_HD inline uint32_t om_roll_join(uint32_t src_hi, uint32_t src_lo, uint32_t sh) {
  return sh != 0u ? (src_hi << sh) | (src_lo >> (32u - sh)) : src_hi;
}

}  // namespace smpc
