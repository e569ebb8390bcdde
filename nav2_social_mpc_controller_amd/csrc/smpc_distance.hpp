// smpc_distance.hpp — the ObstacleDistance grid people projection reads (smpc_projection_batch.od_indexes), computed
// from each scene's costmap: an exact Euclidean nearest-obstacle transform. The reference takes this grid from another
// node over a topic and notes the gap itself (src/optimizer.cpp:597, "TODO use the costmap to compute the obstacles").
//
// Contract (include/smpc.h, smpc_obstacle_distance_batch): for every cell the obstacle cell (ox, oy) that minimises
// (dx^2 + dy^2, ox + oy * W) lexicographically, i.e. the nearest one in integer cells, ties to the smallest linear index.
//
// One workgroup per grid, two passes over bands of rows that fit in LDS:
//   column pass: one lane per column walks down the band keeping the last obstacle row at or above y and the next one at
//     or below y (carried from band to band in LDS; the look-ahead pointer only moves down, so every column is read
//     about once). g[y][x] = the nearer of the two, the upper one on a tie (same column: smaller row = smaller index).
//   row pass: one lane per cell, candidates g[y][x +- k] for k = 0, 1, ... until k^2 exceeds the best squared distance
//     found (a candidate k columns away is at least k^2 away; equality is still examined for the index tie). The
//     nearest obstacle of (x, y) in column ox is g[y][ox], so the minimum over the columns examined is the exact one.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/smpc.h"

namespace smpc {

constexpr int kOdMaxW = 4096;         // columns: carried column state in LDS (2 x 8 KiB)
constexpr int kOdMaxH = 32768;        // rows: kept in uint16 (0xFFFF = none); dx^2 + dy^2 < 2^32 for every cell pair
constexpr int kOdBandCells = 16384;   // g of one band in LDS (32 KiB): bands of kOdBandCells / W rows
constexpr uint16_t kOdNone = 0xFFFF;
constexpr int kOdThreads = 256;

struct DistParams {
  int W, H;
  int min_cost, unknown_is_obstacle;
  float resolution;  // the costmap's resolution as float (= smpc_projection_batch.od_resolution)
  const uint8_t* costmap;  // [grids][H][W]
  uint32_t* indexes;       // [grids][H][W]
  float* distances;        // [grids][H][W] or NULL
  int32_t* n_obstacles;    // [grids] or NULL
};

__device__ inline bool od_obstacle(uint8_t c, const DistParams& p) {
  return c >= p.min_cost && (c != 255 || p.unknown_is_obstacle);
}

// first obstacle row >= y of column x, kOdNone if there is none
__device__ inline int od_scan_down(const uint8_t* cm, int x, int y, const DistParams& p) {
  while (y < p.H && !od_obstacle(cm[(size_t)y * p.W + x], p)) ++y;
  return y < p.H ? y : kOdNone;
}

__global__ __launch_bounds__(kOdThreads) void smpc_obstacle_distance_kernel(const DistParams p) {
  __shared__ uint16_t g[kOdBandCells];
  __shared__ uint16_t above[kOdMaxW], below[kOdMaxW];
  __shared__ int count;
  const int W = p.W, H = p.H, tid = threadIdx.x;
  const uint32_t cells = (uint32_t)W * (uint32_t)H;  // also the "no obstacle" index
  const size_t base = (size_t)blockIdx.x * cells;
  const uint8_t* cm = p.costmap + base;
  uint32_t* idx = p.indexes + base;
  float* dist = p.distances ? p.distances + base : nullptr;
  if (tid == 0) count = 0;
  for (int x = tid; x < W; x += kOdThreads) {
    above[x] = kOdNone;
    below[x] = (uint16_t)od_scan_down(cm, x, 0, p);
  }
  const int R = H < kOdBandCells / W ? H : kOdBandCells / W;
  int nobs = 0;
  for (int y0 = 0; y0 < H; y0 += R) {
    const int rows = H - y0 < R ? H - y0 : R;
    __syncthreads();  // column state initialised / the previous band's row pass is done with g
    for (int x = tid; x < W; x += kOdThreads) {
      int a = above[x], b = below[x];
      for (int r = 0; r < rows; ++r) {
        const int y = y0 + r;
        if (b != kOdNone && b < y) b = od_scan_down(cm, x, y, p);
        if (b == y) { a = y; ++nobs; }
        int best = a;
        if (b != kOdNone && (a == kOdNone || b - y < y - a)) best = b;
        g[r * W + x] = (uint16_t)best;
      }
      above[x] = (uint16_t)a;
      below[x] = (uint16_t)b;
    }
    __syncthreads();
    for (int i = tid; i < rows * W; i += kOdThreads) {
      const int r = i / W, x = i - r * W, y = y0 + r;
      const uint16_t* gr = g + r * W;
      uint32_t bd2 = 0xFFFFFFFFu, bi = cells;
      auto consider = [&](int ox, int k) {
        const int oy = gr[ox];
        if (oy == kOdNone) return;
        const int dy = oy - y;
        const uint32_t d2 = (uint32_t)(k * k) + (uint32_t)(dy * dy);
        const uint32_t id = (uint32_t)ox + (uint32_t)oy * (uint32_t)W;
        if (d2 < bd2 || (d2 == bd2 && id < bi)) { bd2 = d2; bi = id; }
      };
      consider(x, 0);
      for (int k = 1; (uint32_t)(k * k) <= bd2; ++k) {
        const int lo = x - k, hi = x + k;
        if (lo < 0 && hi >= W) break;
        if (lo >= 0) consider(lo, k);
        if (hi < W) consider(hi, k);
      }
      const size_t c = (size_t)y * W + x;
      idx[c] = bi;
      if (dist) dist[c] = bi == cells ? __builtin_inff() : (float)(sqrt((double)bd2) * (double)p.resolution);
    }
  }
  if (nobs) atomicAdd(&count, nobs);
  __syncthreads();
  if (tid == 0 && p.n_obstacles) p.n_obstacles[blockIdx.x] = count;
}

}  // namespace smpc
