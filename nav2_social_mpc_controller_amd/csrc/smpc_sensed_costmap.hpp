// smpc_sensed_costmap.hpp — sensed local costmaps (include/smpc_sensed_costmap.h; the rule: smpc_sensed_costmap_rule.hpp):
// per robot one 360-degree scan over the world map and the agents it is handed, the cells the beams stop at marked in the
// robot's window, the marks inflated, the window written. One workgroup per robot, all state in LDS (45 KB, static: three
// workgroups per CU). A workgroup is a chain of dependent steps, so the steps are shaped to cost one memory round trip each:
//   * reach: the largest |dx|, |dy| of a valid beam (the beams are shared out over the lanes, one LDS max).
//   * agents [256][8] words: which cells of the (2 * 127 + 1)^2 reach square around the robot an agent occupies. A lane finds
//     its agent's cell (256 agents per round trip), then the lanes share out the cells of each disc's bounding box, cut to
//     the square.
//   * walls  [256][8] words: which cells of the square within `reach` occlude: a lane builds one word from up to 32 bytes of
//     one world row (L2), all loads independent of each other. A beam that fetched its cells itself would wait for one
//     round trip per column, because it stops at its first hit: that chain alone took about a third of the kernel.
//   * scan: the beams are shared out over the lanes; a lane walks its beam's columns until the first hit (sc_cast) over
//     the two bitmaps. A hit inside the window sets its bit in
//   * marks  [256][10] words, one window row per line with a zero word to either side (so that the 64 cells around any
//     cell are three words, with no edge case), and its row's bit in rowany (laid out the same way). LDS integer OR: order-free.
//   * inflation, pass 1 (per row): the distance of each cell to the nearest mark of its row within r = isqrt(d2_max), from
//     the row's bit mask (sc_row_gap: a funnel shift and two bit scans), eight cells = one 8-byte LDS word, into
//   * band   [128][32] 8-byte words: the gaps of up to 128 window rows (the two bitmaps lie in the same room: they are done
//     with when the scan is). A window of more rows than 128 - 2r is done in bands of 128 - 2r rows (200 x 200 at r = 14:
//     two bands of 100); the r rows to either side of a band are computed for it again. (The gaps of a whole 256 x 256
//     window would be 64 KB: with the rest, one workgroup per CU.)
//   * pass 2 (per column): the rows within r that hold a mark at all come out of rowany as one 64-bit mask; over its set
//     bits the least gap^2 + dy^2, eight cells at a time; the cost from the table (staged in LDS: 1025 bytes at most), and
//     with base 1 the larger of it and the world row, read as smpc_local_costmap.hpp reads it (lc_half).
//   * the window is written 16 bytes per lane (two 8-cell halves, as smpc_local_costmap.hpp does and under the same
//     condition); every other size a byte at a time.
// Every index is bounded by construction: beam offsets are checked against the reach here (the table is device memory),
// `count` is clamped, agent cells are compared in 64 bits, clamped and cut to the reach square, a world byte is loaded only
// after both of its coordinates were found inside the world, hits are tested against the window in 64 bits, d2 against
// d2_max.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "smpc_local_costmap.hpp"
#include "smpc_math.hpp"
#include "smpc_sensed_costmap_rule.hpp"

namespace smpc {

constexpr int kScThreads = 256;
constexpr int kScSide = 256;        // SMPC_SENSED_MAX_SIZE, and the side of the reach square rounded up
constexpr int kScMarkWords = 10;    // a marks line: word 0 and word 9 stay zero
constexpr int kScBandRows = 128;
constexpr int kScRowUnits = kScSide / 8;
constexpr int kScMaxD2 = 1024;     // SMPC_SENSED_MAX_D2

struct SensedCostmapParams {
  int B, Np, size_x, size_y, world_x, world_y, world_shared;
  int n_beams, agent_d2, agent_r;  // agent_r = isqrt(agent_d2)
  int d2_max, r;                   // r = isqrt(d2_max) <= 32
  int base, wide;                  // wide: the 16-byte path (decided by the host: sizes and the alignment of costmap)
  uint32_t outside;                // outside_cost in every byte
  VisOcc occ;
  double resolution;
  const uint8_t* world;            // [B or 1][world_y][world_x]
  const double* world_origin;      // [B or 1][2]
  const double* robot_pose;        // [B][3]
  const double* people;            // [B][Np][5]
  const int32_t* count;            // [B]
  const int32_t* cell;             // [B][2]
  const int32_t* beam_cells;       // [n_beams][2]
  const uint8_t* inflation_cost;   // [d2_max + 1]
  uint8_t* costmap;                // [B][size_y][size_x]
  uint8_t* beam_kind;              // [B][n_beams] or null
  int32_t* beam_cell;              // [B][n_beams][2] or null
};

// the larger of every byte of a and b
__device__ inline uint64_t sc_max_bytes(uint64_t a, uint64_t b) {
  uint64_t v = 0;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const uint64_t x = (a >> (8 * c)) & 255u, y = (b >> (8 * c)) & 255u;
    v |= (x > y ? x : y) << (8 * c);
  }
  return v;
}

// 8 bytes of the world as smpc_local_costmap_batch cuts them: world row wy, columns wx .. wx + 7 (64-bit: `cell` is any int32)
__device__ inline uint64_t sc_world_half(const LocalCostmapParams& lp, const uint8_t* world, int64_t wx, int64_t wy) {
  if (wy < 0 || wy >= lp.world_y || wx <= -8 || wx >= lp.world_x) return ((uint64_t)lp.outside << 32) | lp.outside;
  const uint2 h = lc_half(lp, world, (int)wx, (int)wy);
  return ((uint64_t)h.y << 32) | h.x;
}

__global__ __launch_bounds__(kScThreads) void smpc_sensed_costmap_kernel(const SensedCostmapParams p) {
  SMPC_CHAIN_PRIORITY();
  __shared__ uint64_t band[kScBandRows * kScRowUnits];   // during the scan: the two occupancy bitmaps
  __shared__ uint32_t marks[kScSide * kScMarkWords];
  __shared__ uint32_t rowany[kScMarkWords];              // one bit per window row that holds a mark, a zero word to either side
  __shared__ int32_t rel[kScThreads * 2];                // a chunk of agents: their cells relative to the robot's
  __shared__ uint32_t table_words[(kScMaxD2 + 1 + 3) / 4];
  __shared__ int32_t reach;                              // the largest |dx|, |dy| of a valid beam
  uint32_t* agents = reinterpret_cast<uint32_t*>(band);  // [256][8]
  uint32_t* walls = agents + kScSide * 8;                // [256][8]
  uint8_t* table = reinterpret_cast<uint8_t*>(table_words);
  const int tid = (int)threadIdx.x;
  const uint32_t r = (uint32_t)p.r, d2_max = (uint32_t)p.d2_max;
  const int units = (p.size_x + 7) >> 3;            // 8-cell units per window row, <= 32
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
  __syncthreads();  // `reach` is known

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
        // 32 loads in flight together: a cell beyond the reach or the world reads column 0 of the row, which always exists,
        // so that no load waits for a branch (behind one each, they were 32 round trips one after the other)
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

  // the scan
  const auto stops = [&](int32_t cx, int32_t cy) -> uint32_t {
    if ((cx | cy) == 0) return 0u;
    const uint32_t bx = (uint32_t)(cx + kSensedReach), by = (uint32_t)(cy + kSensedReach);  // within the beam's reach: 0 .. 254
    const uint32_t at = by * 8u + (bx >> 5), bit = bx & 31u;
    const uint32_t wall = (walls[at] >> bit) & 1u, agent = (agents[at] >> bit) & 1u;  // both reads before either test: one wait
    return wall != 0u ? kBeamWorld : (agent != 0u ? kBeamAgent : 0u);
  };
  const auto mark = [&](int32_t cx, int32_t cy) {
    int32_t wx = 0, wy = 0;
    if (!sc_window_cell(ax, ay, cx, cy, cell_x, cell_y, p.size_x, p.size_y, &wx, &wy)) return;
    atomicOr(&marks[wy * kScMarkWords + 1 + (wx >> 5)], 1u << (wx & 31));
    atomicOr(&rowany[1 + (wy >> 5)], 1u << (wy & 31));
  };
  for (int k = tid; k < p.n_beams; k += kScThreads) {
    const int32_t ex = p.beam_cells[2 * k], ey = p.beam_cells[2 * k + 1];
    uint32_t kind = kBeamNoRobot;
    int32_t hx = ex, hy = ey;
    if (robot_ok) {
      kind = kBeamInvalid;
      if (sc_beam_valid(ex, ey)) {
        const ScHit h = sc_cast(ex, ey, stops);
        kind = h.kind; hx = h.ox; hy = h.oy;
        if (kind != kBeamNone) mark(h.ox, h.oy);
        if (kind == kBeamCornerPair) mark(h.px, h.py);
      }
    }
    const size_t at = s * (size_t)p.n_beams + (size_t)k;
    if (p.beam_kind) p.beam_kind[at] = (uint8_t)kind;
    if (p.beam_cell) { p.beam_cell[2 * at] = hx; p.beam_cell[2 * at + 1] = hy; }
  }
  __syncthreads();  // the marks are complete, and the bitmaps' room is the band's from here on

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
