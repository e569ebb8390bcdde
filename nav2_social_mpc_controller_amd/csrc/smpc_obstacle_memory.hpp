// smpc_obstacle_memory.hpp — sensed local costmaps with memory (include/smpc_obstacle_memory.h; the rule:
// smpc_obstacle_memory_rule.hpp): smpc_sensed_costmap.hpp's scan with a mark bitmap that persists from call to call. One
// workgroup per robot, the same LDS rooms as the memoryless kernel (no new room: 45 KB, static, three workgroups per CU),
// and the same chain of steps with four additions. The memoryless kernel's steps are restated here, not shared: that
// kernel's machine code stays what it was.
//   * roll: after the rooms are zeroed a lane builds one word of `marks` from the two words of the old bitmap that land in
//     it (om_roll_source / om_roll_join), all loads independent of each other. The whole old bitmap is in LDS before the
//     first barrier that follows, so writing memory[b] in place at the end is safe.
//   * scan: a lane walks its beam once (om_cast). For each passed cell inside the window it reads its bit in `marks` with a
//     plain LDS read and issues an LDS atomicAnd only when the bit is set: a steady-state memory holds a fraction of a
//     percent of the cells, so almost every passed cell costs a read. The read-then-and is safe by rule 4 of the contract:
//     a passed cell is never a hit, so its bit can only have been set by the roll, which finished barriers ago; another
//     lane can at most have cleared it already, and clearing twice is clearing. Hits within mark_d2 are set by atomicOr.
//   * footprint: after a barrier the lanes share out the disc's bounding box, cut to the window, and clear the cells in it.
//   * rowany is computed from `marks` afterwards, one lane per row over its 8 words: clearing can empty a row. Then
//     memory[b] is written from `marks` by plain 4-byte vector stores (consecutive lanes, consecutive words), padding masked,
//     and memory_cell[b].
// Inflation and the window stores are the memoryless kernel's.
// Every index is bounded by construction: all that smpc_sensed_costmap.hpp lists, and: the roll compares both shifts in
// 64 bits against the largest window side before forming a row or a word index (om_shift, then om_roll_row and
// om_roll_source against the window's own sides), reads a source word only when its index lies in 0 .. W - 1 and writes
// the words 0 .. W - 1 of the rows 0 .. size_y - 1 only; a passed cell and a hit go through om_window_cell (on
// om_window_rel's 64-bit difference) before they index `marks`; the footprint's box is cut to the window in 64 bits before
// a lane indexes it; the write-back runs over t < size_y * W.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "smpc_obstacle_memory_rule.hpp"
#include "smpc_sensed_costmap.hpp"

namespace smpc {

struct ObstacleMemoryParams {
  SensedCostmapParams sc;
  int mark_d2, footprint_d2, footprint_r;  // footprint_r = isqrt(footprint_d2), -1 without a footprint
  uint32_t* memory;                        // [B][size_y][(size_x + 31) / 32], read and written
  int32_t* memory_cell;                    // [B][2], read and written
};

__global__ __launch_bounds__(kScThreads) void smpc_obstacle_memory_kernel(const ObstacleMemoryParams q) {
  SMPC_CHAIN_PRIORITY();
  __shared__ uint64_t band[kScBandRows * kScRowUnits];   // during the scan: the two occupancy bitmaps
  __shared__ uint32_t marks[kScSide * kScMarkWords];
  __shared__ uint32_t rowany[kScMarkWords];              // one bit per window row that holds a mark, a zero word to either side
  __shared__ int32_t rel[kScThreads * 2];                // a chunk of agents: their cells relative to the robot's
  __shared__ uint32_t table_words[(kScMaxD2 + 1 + 3) / 4];
  __shared__ int32_t reach;                              // the largest |dx|, |dy| of a valid beam
  const SensedCostmapParams& p = q.sc;
  uint32_t* agents = reinterpret_cast<uint32_t*>(band);  // [256][8]
  uint32_t* walls = agents + kScSide * 8;                // [256][8]
  uint8_t* table = reinterpret_cast<uint8_t*>(table_words);
  const int tid = (int)threadIdx.x;
  const uint32_t r = (uint32_t)p.r, d2_max = (uint32_t)p.d2_max;
  const int units = (p.size_x + 7) >> 3;            // 8-cell units per window row, <= 32
  const int words = (p.size_x + 31) >> 5;           // words per bitmap row, <= 8
  const uint32_t mem_words = (uint32_t)p.size_y * (uint32_t)words;  // words of one robot's bitmap, <= 2048
  const int band_out = kScBandRows - 2 * p.r;       // rows a band writes, >= 64
  const uint32_t n = (uint32_t)p.size_x * (uint32_t)p.size_y;
  const long long b = (long long)blockIdx.y * gridDim.x + blockIdx.x;
  if (b >= p.B) return;  // workgroup-uniform
  const size_t s = b, g = p.world_shared ? 0 : s;
  const uint8_t* world = p.world + g * (size_t)p.world_x * (size_t)p.world_y;
  const double ox = p.world_origin[2 * g], oy = p.world_origin[2 * g + 1];
  const int32_t cell_x = p.cell[2 * s], cell_y = p.cell[2 * s + 1];
  const int cnt = min(max(p.count[s], 0), p.Np);
  int32_t ax = 0, ay = 0;
  const bool robot_ok = vis_robot_cell(p.robot_pose[3 * s], p.robot_pose[3 * s + 1], ox, oy, p.resolution, &ax, &ay);
  for (int t = tid; t <= p.d2_max; t += kScThreads) table[t] = p.inflation_cost[t];
  for (int t = tid; t < kScSide * 16; t += kScThreads) agents[t] = 0u;  // both bitmaps
  for (int t = tid; t < kScSide * kScMarkWords; t += kScThreads) marks[t] = 0u;
  if (tid < kScMarkWords) rowany[tid] = 0u;
  if (tid == 0) reach = 0;
  __syncthreads();

  // the roll: destination word w of row y from the two words of old row y - shift_y that land in it
  {
    const int32_t shift_x = om_shift(q.memory_cell[2 * s], cell_x), shift_y = om_shift(q.memory_cell[2 * s + 1], cell_y);
    const uint32_t* memory = q.memory + s * (size_t)mem_words;
    for (uint32_t t = (uint32_t)tid; t < mem_words; t += kScThreads) {
      const int y = (int)(t / (uint32_t)words), w = (int)t - y * words;
      int32_t src_y = 0;
      OmRoll ro;
      if (!om_roll_row(shift_y, p.size_y, y, &src_y) || !om_roll_source(shift_x, p.size_x, w, &ro)) continue;
      const uint32_t* src = memory + (uint32_t)src_y * (uint32_t)words;  // row src_y < size_y
      const int lo = ro.hi - 1;
      const uint32_t hi_word = (uint32_t)ro.hi < (uint32_t)words ? src[ro.hi] & om_word_mask(p.size_x, ro.hi) : 0u;
      const uint32_t lo_word = (uint32_t)lo < (uint32_t)words ? src[lo] & om_word_mask(p.size_x, lo) : 0u;
      marks[y * kScMarkWords + 1 + w] = om_roll_join(hi_word, lo_word, ro.sh) & om_word_mask(p.size_x, w);
    }
  }

  if (robot_ok) {
    int32_t far = 0;
    for (int k = tid; k < p.n_beams; k += kScThreads) {
      const int32_t ex = p.beam_cells[2 * k], ey = p.beam_cells[2 * k + 1];
      if (sc_beam_valid(ex, ey)) far = max(far, max(abs(ex), abs(ey)));
    }
    if (far > 0) atomicMax(&reach, far);
  }

  // the agents' cells within reach, a chunk of 256 agents at a time: a lane finds its agent's cell, then the lanes share out
  // the cells of each disc's bounding box
  if (robot_ok) {
    for (int base = 0; base < cnt; base += kScThreads) {  // workgroup-uniform
      __syncthreads();  // `rel` is free
      const int j = base + tid;
      if (j < cnt) {
        const double* row = p.people + (s * (size_t)p.Np + (size_t)j) * 5;
        int32_t qx = 0, qy = 0;
        const bool has_cell = sc_agent_cell(row[0], row[1], ox, oy, p.resolution, &qx, &qy);
        // beyond 2^17 cells an agent is out of reach whatever agent_d2 (< 2^31: agent_r <= 46340) is: the clamp keeps the rest in 32 bits
        rel[2 * tid] = has_cell ? (int32_t)min(max((int64_t)qx - ax, (int64_t)-131072), (int64_t)131072) : 131072;
        rel[2 * tid + 1] = has_cell ? (int32_t)min(max((int64_t)qy - ay, (int64_t)-131072), (int64_t)131072) : 131072;
      }
      __syncthreads();
      const int chunk = min(cnt - base, kScThreads);
      for (int jj = 0; jj < chunk; ++jj) {  // workgroup-uniform
        const int32_t relx = rel[2 * jj], rely = rel[2 * jj + 1];
        const int32_t x0 = max(relx - p.agent_r, -kSensedReach), x1 = min(relx + p.agent_r, kSensedReach);
        const int32_t y0 = max(rely - p.agent_r, -kSensedReach), y1 = min(rely + p.agent_r, kSensedReach);
        if (x0 > x1 || y0 > y1) continue;
        const int w = x1 - x0 + 1, cells = w * (y1 - y0 + 1);  // <= 255 * 255
        for (int t = tid; t < cells; t += kScThreads) {
          const int ty = t / w, tx = t - ty * w;
          const int32_t cx = x0 + tx, cy = y0 + ty;  // in -127 .. 127
          const int32_t ddx = cx - relx, ddy = cy - rely;  // |.| <= agent_r: the sum of the squares is below 2^32
          if ((uint32_t)(ddx * ddx) + (uint32_t)(ddy * ddy) <= (uint32_t)p.agent_d2) {
            const uint32_t bx = (uint32_t)(cx + kSensedReach), by = (uint32_t)(cy + kSensedReach);  // 0 .. 254
            atomicOr(&agents[by * 8u + (bx >> 5)], 1u << (bx & 31u));
          }
        }
      }
    }
  }
  __syncthreads();  // `reach` is known, and the roll is in `marks`

  // the world's occluding cells within reach: a lane builds one word of the bitmap from up to 32 bytes of one world row
  if (robot_ok && reach > 0) {
    const int R = reach;                                               // <= 127
    const int w_lo = (kSensedReach - R) >> 5, n_words = ((kSensedReach + R) >> 5) - w_lo + 1;
    for (int t = tid; t < (2 * R + 1) * n_words; t += kScThreads) {
      const int ty = t / n_words, word = w_lo + (t - ty * n_words), cy = ty - R;
      const int32_t wy = ay + cy;  // |a| <= 2^30, |c| <= 127
      uint32_t bits = 0u;
      if ((uint32_t)wy < (uint32_t)p.world_y) {
        const uint8_t* row = world + (size_t)wy * (size_t)p.world_x;
        // 32 loads in flight together: a cell beyond the reach or the world reads column 0 of the row, which always exists
#pragma unroll
        for (int bit = 0; bit < 32; ++bit) {
          const int cx = word * 32 + bit - kSensedReach;
          const int32_t wx = ax + cx;
          const bool in = (cx >= -R) & (cx <= R) & ((uint32_t)wx < (uint32_t)p.world_x);
          const uint32_t cost = row[in ? wx : 0];
          bits |= (uint32_t)(in & vis_occludes(p.occ, cost)) << bit;
        }
      }
      walls[(uint32_t)(cy + kSensedReach) * 8u + (uint32_t)word] = bits;
    }
  }
  __syncthreads();

  // the scan: clears and marks in one pass (the two sets are disjoint: rule 4)
  const int32_t rel_x = om_window_rel(ax, cell_x), rel_y = om_window_rel(ay, cell_y);  // the robot's window cell, inside the window or not
  const auto stops = [&](int32_t cx, int32_t cy) -> uint32_t {
    if ((cx | cy) == 0) return 0u;
    const uint32_t bx = (uint32_t)(cx + kSensedReach), by = (uint32_t)(cy + kSensedReach);  // within the beam's reach: 0 .. 254
    const uint32_t at = by * 8u + (bx >> 5), bit = bx & 31u;
    const uint32_t wall = (walls[at] >> bit) & 1u, agent = (agents[at] >> bit) & 1u;  // both reads before either test: one wait
    return wall != 0u ? kBeamWorld : (agent != 0u ? kBeamAgent : 0u);
  };
  const auto pass = [&](int32_t cx, int32_t cy) {
    int32_t wx = 0, wy = 0;
    if (!om_window_cell(rel_x, rel_y, cx, cy, p.size_x, p.size_y, &wx, &wy)) return;
    uint32_t* word = &marks[wy * kScMarkWords + 1 + (wx >> 5)];
    const uint32_t bit = 1u << (wx & 31);
    if ((*word & bit) != 0u) atomicAnd(word, ~bit);
  };
  const auto mark = [&](int32_t cx, int32_t cy) {
    int32_t wx = 0, wy = 0;
    if (!om_in_mark_range(cx, cy, q.mark_d2)) return;
    if (!om_window_cell(rel_x, rel_y, cx, cy, p.size_x, p.size_y, &wx, &wy)) return;
    atomicOr(&marks[wy * kScMarkWords + 1 + (wx >> 5)], 1u << (wx & 31));
  };
  for (int k = tid; k < p.n_beams; k += kScThreads) {
    const int32_t ex = p.beam_cells[2 * k], ey = p.beam_cells[2 * k + 1];
    uint32_t kind = kBeamNoRobot;
    int32_t hx = ex, hy = ey;
    if (robot_ok) {
      kind = kBeamInvalid;
      if (sc_beam_valid(ex, ey)) {
        const ScHit h = om_cast(ex, ey, stops, pass);
        kind = h.kind; hx = h.ox; hy = h.oy;
        if (kind != kBeamNone) mark(h.ox, h.oy);
        if (kind == kBeamCornerPair) mark(h.px, h.py);
      }
    }
    const size_t at = s * (size_t)p.n_beams + (size_t)k;
    if (p.beam_kind) p.beam_kind[at] = (uint8_t)kind;
    if (p.beam_cell) { p.beam_cell[2 * at] = hx; p.beam_cell[2 * at + 1] = hy; }
  }
  __syncthreads();  // clears and marks are complete, and the bitmaps' room is the band's from here on

  // the footprint: the disc's bounding box, cut to the window (64 bits: `cell` is any int32), shared out over the lanes
  if (robot_ok && q.footprint_d2 >= 0) {
    const int64_t fx0 = max((int64_t)rel_x - q.footprint_r, (int64_t)0), fx1 = min((int64_t)rel_x + q.footprint_r, (int64_t)p.size_x - 1);
    const int64_t fy0 = max((int64_t)rel_y - q.footprint_r, (int64_t)0), fy1 = min((int64_t)rel_y + q.footprint_r, (int64_t)p.size_y - 1);
    if (fx0 <= fx1 && fy0 <= fy1) {
      const int w = (int)(fx1 - fx0 + 1), cells = w * (int)(fy1 - fy0 + 1);  // <= 256 * 256
      for (int t = tid; t < cells; t += kScThreads) {
        const int ty = t / w, tx = t - ty * w;
        const int wx = (int)fx0 + tx, wy = (int)fy0 + ty;  // inside the window
        if (om_in_footprint((int64_t)wx - rel_x, (int64_t)wy - rel_y, q.footprint_d2)) {
          uint32_t* word = &marks[wy * kScMarkWords + 1 + (wx >> 5)];
          const uint32_t bit = 1u << (wx & 31);
          if ((*word & bit) != 0u) atomicAnd(word, ~bit);
        }
      }
    }
    __syncthreads();  // workgroup-uniform branch
  }

  // rowany from the marks (clearing can empty a row), one lane per row, and the state back to memory
  for (int y = tid; y < p.size_y; y += kScThreads) {
    const uint32_t* line = marks + y * kScMarkWords + 1;
    uint32_t any = 0u;
#pragma unroll
    for (int w = 0; w < 8; ++w) any |= line[w];
    if (any != 0u) atomicOr(&rowany[1 + (y >> 5)], 1u << (y & 31));
  }
  uint32_t* memory = q.memory + s * (size_t)mem_words;
  for (uint32_t t = (uint32_t)tid; t < mem_words; t += kScThreads) {
    const int y = (int)(t / (uint32_t)words), w = (int)t - y * words;
    memory[t] = marks[y * kScMarkWords + 1 + w] & om_word_mask(p.size_x, w);
  }
  if (tid < 2) q.memory_cell[2 * s + (size_t)tid] = tid == 0 ? cell_x : cell_y;
  __syncthreads();  // rowany is complete

  // eight cells of window row y from column x0 (a multiple of 8): inflation (pass 2) and base
  LocalCostmapParams lp{};
  lp.world_x = p.world_x; lp.world_y = p.world_y; lp.outside = p.outside;
  uint8_t* dst = p.costmap + s * (size_t)n;
  int band_lo = 0;
  const uint64_t near_rows = r >= 32u ? ~0ull : ((1ull << (2u * r + 1u)) - 1ull) << (32u - r);  // bit t: the row at y - 32 + t is within r
  const auto half = [&](int x0, int y) -> uint64_t {
    uint32_t best[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) best[c] = kSensedNoMark;
    // the rows y - 32 .. y + 31 that hold a mark at all, from rowany (bit 0 of line[0] is row (y & ~31) - 32), and row y + 32
    const uint32_t* line = rowany + (y >> 5);
    const uint32_t sh = (uint32_t)(y & 31), w2 = line[2];
    const uint64_t w01 = ((uint64_t)line[1] << 32) | line[0];
    uint64_t rows = (sh != 0u ? (w01 >> sh) | ((uint64_t)w2 << (64u - sh)) : w01) & near_rows;
    while (rows != 0ull) {
      const int t = __builtin_ctzll(rows);
      rows &= rows - 1ull;
      const uint64_t gaps = band[(y - 32 + t - band_lo) * units + (x0 >> 3)];
      const uint32_t dy2 = (uint32_t)((t - 32) * (t - 32));
#pragma unroll
      for (int c = 0; c < 8; ++c) best[c] = sc_least_d2(best[c], (uint32_t)(gaps >> (8 * c)) & 255u, dy2);
    }
    if (r >= 32u && ((w2 >> sh) & 1u) != 0u) {
      const uint64_t gaps = band[(y + 32 - band_lo) * units + (x0 >> 3)];
#pragma unroll
      for (int c = 0; c < 8; ++c) best[c] = sc_least_d2(best[c], (uint32_t)(gaps >> (8 * c)) & 255u, 1024u);
    }
    uint64_t v = 0;
#pragma unroll
    for (int c = 0; c < 8; ++c) v |= (uint64_t)sc_cost(best[c], table, d2_max) << (8 * c);
    if (p.base) v = sc_max_bytes(v, sc_world_half(lp, world, (int64_t)cell_x + x0, (int64_t)cell_y + y));
    return v;
  };
  for (int y0 = 0; y0 < p.size_y; y0 += band_out) {  // workgroup-uniform
    const int y1 = min(y0 + band_out, p.size_y);
    band_lo = max(y0 - (int)r, 0);
    const int band_hi = min(y1 + (int)r, p.size_y);  // band_hi - band_lo <= 128
    // pass 1: the gaps of the band's rows that hold a mark
    for (int u = tid; u < (band_hi - band_lo) * units; u += kScThreads) {
      const int rr = u / units, ux = u - rr * units, y = band_lo + rr, x0 = ux * 8;
      if (((rowany[1 + (y >> 5)] >> (y & 31)) & 1u) == 0u) continue;
      const uint32_t* line = marks + y * kScMarkWords + (x0 >> 5);  // bit 0 of line[0] is cell (x0 & ~31) - 32; line[2] is word <= 9
      const uint32_t w2 = line[2];
      const uint64_t w01 = ((uint64_t)line[1] << 32) | line[0];
      uint64_t gaps = 0;
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        const uint32_t sh = (uint32_t)(x0 & 31) + (uint32_t)c;  // <= 31
        const uint64_t v = sh != 0u ? (w01 >> sh) | ((uint64_t)w2 << (64u - sh)) : w01;
        gaps |= (uint64_t)sc_row_gap(v, w2 >> sh, r) << (8 * c);
      }
      band[u] = gaps;
    }
    __syncthreads();
    if (p.wide) {
      // rows y0 .. y1 - 1 are a multiple of 16 bytes (size_x a multiple of 8, band_out even, the window a multiple of 16)
      for (uint32_t i = (uint32_t)y0 * (uint32_t)p.size_x + (uint32_t)tid * 16u; i < (uint32_t)y1 * (uint32_t)p.size_x; i += kScThreads * 16u) {
        const uint32_t y = i / (uint32_t)p.size_x, x = i - y * (uint32_t)p.size_x;  // x is a multiple of 8, <= size_x - 8
        uint32_t x2 = x + 8u, y2 = y;
        if (x2 == (uint32_t)p.size_x) { x2 = 0u; y2 = y + 1u; }  // (then y + 1 < y1: the 16 bytes lie below the band's end)
        const uint64_t h0 = half((int)x, (int)y), h1 = half((int)x2, (int)y2);
        *reinterpret_cast<uint4*>(dst + i) = make_uint4((uint32_t)h0, (uint32_t)(h0 >> 32), (uint32_t)h1, (uint32_t)(h1 >> 32));
      }
    } else {
      for (int u = tid; u < (y1 - y0) * units; u += kScThreads) {
        const int rr = u / units, x0 = (u - rr * units) * 8, y = y0 + rr;
        const uint64_t v = half(x0, y);
#pragma unroll
        for (int c = 0; c < 8; ++c)
          if (x0 + c < p.size_x) dst[(size_t)y * (size_t)p.size_x + (size_t)(x0 + c)] = (uint8_t)(v >> (8 * c));
      }
    }
    __syncthreads();  // the band is free again
  }
}

}  // namespace smpc
