// smpc_local_costmap.hpp — the rolling local costmaps of a closed-loop episode (include/smpc_local_costmap.h): every
// robot's window follows its pose (the cell rule: smpc_local_costmap_rule.hpp) and the windows that moved are cut out of
// the world map into costmap [B][size_y][size_x], the buffers the solve reads as they are.
// A store-bound copy: the world map is small and stays in L2, every window byte is stored once. No LDS, no atomics.
//   * The unit of work is the robot: `cell` is in-out and decides whether a robot is written at all, so ONE workgroup
//     reads a robot's cell, then (behind a barrier) writes it and copies the window; a fixed grid strides over the robots.
//     The decision is workgroup-uniform: a robot that stays costs two loads and no store.
//   * Wide path (size_x a multiple of 8, size_x * size_y a multiple of 16, a 16-byte aligned costmap: 200 x 200, 80 x 80):
//     a lane builds 16 destination bytes from two 8-byte halves and stores them in one 16-byte store, 4 KB per workgroup
//     pass. A half lies in one window row (a 16-byte piece may straddle two: 200 mod 16 = 8); its source starts at any byte
//     residue of the world row: the two or three aligned dwords around it are loaded and shifted. A half that is partly
//     outside the world is put together byte by byte, one wholly outside is the fill value.
//   * Every other size: a lane per byte.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "smpc_local_costmap_rule.hpp"
#include "smpc_math.hpp"

namespace smpc {

constexpr int kLcThreads = 256;

struct LocalCostmapParams {
  int B, size_x, size_y, world_x, world_y, world_shared;
  int wide;                    // the 16-byte path (decided by the host: sizes and the alignment of costmap)
  int force;
  uint32_t outside;            // outside_cost in every byte
  double resolution;
  const uint8_t* world;        // [B or 1][world_y][world_x]
  const double* world_origin;  // [B or 1][2]
  const double* pose;          // [B][3]
  int32_t* cell;               // [B][2] in / out
  uint8_t* costmap;            // [B][size_y][size_x]
  double* costmap_origin;      // [B][2]
  int32_t* moved;              // [B] or null
};

// 8 window bytes of one window row: world row wy, columns wx .. wx + 7 (any of them may lie outside the world)
__device__ inline uint2 lc_half(const LocalCostmapParams& p, const uint8_t* world, int wx, int wy) {
  if ((unsigned)wy >= (unsigned)p.world_y || wx <= -8 || wx >= p.world_x) return make_uint2(p.outside, p.outside);
  const uint8_t* row = world + (size_t)wy * (size_t)p.world_x;
  if (wx >= 0 && wx <= p.world_x - 8) {
    // The aligned dwords that hold the 8 bytes. The third one is read only when the run reaches into it, so no load
    // touches a dword without a byte of the world map in it.
    const uint8_t* src = row + wx;
    const unsigned mis = (unsigned)(reinterpret_cast<uintptr_t>(src) & 3u), sh = mis * 8u;
    const uint32_t* q = reinterpret_cast<const uint32_t*>(src - mis);
    const uint32_t d0 = q[0], d1 = q[1], d2 = sh ? q[2] : 0u;
    const uint64_t lo = ((uint64_t)d1 << 32) | d0, hi = ((uint64_t)d2 << 32) | d1;
    return make_uint2((uint32_t)(lo >> sh), (uint32_t)(hi >> sh));
  }
  uint64_t v = 0;
  for (int k = 0; k < 8; ++k) {
    const int x = wx + k;
    const uint32_t c = (x >= 0 && x < p.world_x) ? (uint32_t)row[x] : (p.outside & 0xFFu);
    v |= (uint64_t)c << (8 * k);
  }
  return make_uint2((uint32_t)v, (uint32_t)(v >> 32));
}

__global__ __launch_bounds__(kLcThreads) void smpc_local_costmap_kernel(const LocalCostmapParams p) {
  SMPC_CHAIN_PRIORITY();
  const uint32_t n = (uint32_t)p.size_x * (uint32_t)p.size_y;  // < 2^31, each side < 2^30 (checked by the host): cell + x is an int
  for (int b = blockIdx.x; b < p.B; b += gridDim.x) {
    const size_t s = b, g = p.world_shared ? 0 : s;
    const LcRoll r = lc_roll(p.world_origin[2 * g], p.world_origin[2 * g + 1], p.cell[2 * s], p.cell[2 * s + 1], p.resolution,
                             p.size_x, p.size_y, p.pose[3 * s], p.pose[3 * s + 1], p.force != 0);
    __syncthreads();  // every lane of the robot's only workgroup has read the stored cell
    if (threadIdx.x == 0) {
      if (p.moved) p.moved[s] = r.moved;
      if (r.write) {
        p.cell[2 * s] = r.cx; p.cell[2 * s + 1] = r.cy;
        p.costmap_origin[2 * s] = lc_origin(p.world_origin[2 * g], r.cx, p.resolution);
        p.costmap_origin[2 * s + 1] = lc_origin(p.world_origin[2 * g + 1], r.cy, p.resolution);
      }
    }
    if (!r.write) continue;  // workgroup-uniform
    const uint8_t* world = p.world + g * (size_t)p.world_x * (size_t)p.world_y;
    uint8_t* dst = p.costmap + s * (size_t)n;
    if (p.wide) {
      for (uint32_t i = threadIdx.x * 16u; i < n; i += kLcThreads * 16u) {
        const uint32_t y = i / (uint32_t)p.size_x, x = i - y * (uint32_t)p.size_x;  // x is a multiple of 8, <= size_x - 8
        uint32_t x2 = x + 8u, y2 = y;
        if (x2 == (uint32_t)p.size_x) { x2 = 0u; y2 = y + 1u; }
        const uint2 h0 = lc_half(p, world, r.cx + (int)x, r.cy + (int)y);
        const uint2 h1 = lc_half(p, world, r.cx + (int)x2, r.cy + (int)y2);
        *reinterpret_cast<uint4*>(dst + i) = make_uint4(h0.x, h0.y, h1.x, h1.y);
      }
    } else {
      for (uint32_t i = threadIdx.x; i < n; i += kLcThreads) {
        const uint32_t y = i / (uint32_t)p.size_x, x = i - y * (uint32_t)p.size_x;
        const int wx = r.cx + (int)x, wy = r.cy + (int)y;
        const bool in = (unsigned)wx < (unsigned)p.world_x && (unsigned)wy < (unsigned)p.world_y;
        dst[i] = in ? world[(size_t)wy * (size_t)p.world_x + (size_t)wx] : (uint8_t)p.outside;
      }
    }
  }
}

}  // namespace smpc
