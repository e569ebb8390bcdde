// smpc_bicubic.hpp — bicubic interpolation of the u8 costmap, value and gradient (the obstacle critic): in one piece
// (bicubic) and split into the fetch of the 4 x 4 patch and its evaluation (bicubic_fetch / bicubic_eval).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace smpc {

// ------------------------------------------------------------------------------------------------
// Bicubic interpolation of the u8 costmap with clamp-to-edge, value and gradient
// (ceres::BiCubicInterpolator<Grid2D<u_char>> semantics; used by
// critics/obstacle_cost_function.hpp:161 as Evaluate(row = y_cell, col = x_cell)).
// ------------------------------------------------------------------------------------------------
__device__ inline void cubic_hermite(double p0, double p1, double p2, double p3, double x, double& f, double& df) {
  const double a = 0.5 * (-p0 + 3.0 * p1 - 3.0 * p2 + p3);
  const double b = 0.5 * (2.0 * p0 - 5.0 * p1 + 4.0 * p2 - p3);
  const double c = 0.5 * (-p0 + p2);
  f = p1 + x * (c + x * (b + x * a));
  df = c + x * (2.0 * b + 3.0 * a * x);
}

// The same interpolation split in two, so that the sweep can request the 4 x 4 patch as soon as the pose is known and
// consume it after the agent loop (the 16 dependent byte loads were 6 % of a lone solve launch): the patch is fetched
// as four unaligned dwords, one per row, starting at column clamp(col - 1, 0, size_x - 4); the byte of clamped column
// cc is then byte (cc - start) of its row's dword — also at the edges, where several taps share a cell.
struct CostPatch {
  uint32_t row[4];   // bytes start .. start + 3 of the four clamped rows
};

// Integer cell of a coordinate, kept defined for wild values (clamping below makes any far-outside index equivalent).
__device__ inline int cell_index(double v, int size) { return (int)fmin(fmax(floor(v), -4.0), (double)size + 4.0); }

// true when the whole 4 x 4 patch around (r, c) lies inside the map: no tap is clamped (NaN coordinates: false)
__device__ inline bool bicubic_interior(int size_x, int size_y, double r, double c) {
  const int row = cell_index(r, size_y), col = cell_index(c, size_x);
  return (row >= 1) & (row <= size_y - 3) & (col >= 1) & (col <= size_x - 3);
}

// kInterior: the caller has established bicubic_interior() for EVERY lane of the wave (a wave-uniform decision: the
// clamps, the per-tap bit offsets and their variable shifts — ~90 integer instructions per sweep — are then skipped;
// the taps and the arithmetic on them are the same, so the result does not depend on which path a wave takes).
template <bool kInterior>
__device__ inline void bicubic_fetch(const uint8_t* __restrict__ map, int size_x, int size_y, double r, double c, CostPatch& p) {
  const int row = cell_index(r, size_y), col = cell_index(c, size_x);
  if (kInterior) {
    const uint8_t* q = map + (size_t)(row - 1) * size_x + (col - 1);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      uint32_t v;
      __builtin_memcpy(&v, q + (size_t)i * size_x, 4);  // unaligned dword
      p.row[i] = v;
    }
    return;
  }
  const int start = min(max(col - 1, 0), size_x - 4);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int rr = min(max(row - 1 + i, 0), size_y - 1);
    uint32_t v;
    __builtin_memcpy(&v, map + (size_t)rr * size_x + start, 4);  // unaligned dword
    p.row[i] = v;
  }
}

// (r, c) must be the coordinates the patch was fetched for. The bit offsets of the clamped taps inside a row dword are
// derived here from c, not at the fetch: carried in the patch across the agent loop they were one register more than K1
// <3,32> has (one spilled VGPR).
template <bool kInterior>
__device__ inline void bicubic_eval(const CostPatch& p, int size_x, double r, double c, double& f, double& dfdr,
                                    double& dfdc) {
  const double tr = r - floor(r), tc = c - floor(c);
  uint32_t sh[4] = {0u, 8u, 16u, 24u};
  if (!kInterior) {
    const int col = cell_index(c, size_x);
    const int start = min(max(col - 1, 0), size_x - 4);
#pragma unroll
    for (int j = 0; j < 4; ++j) sh[j] = (uint32_t)(8 * (min(max(col - 1 + j, 0), size_x - 1) - start));
  }
  double fv[4], dv[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    double t[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) t[j] = (double)((p.row[i] >> sh[j]) & 0xffu);
    cubic_hermite(t[0], t[1], t[2], t[3], tc, fv[i], dv[i]);
  }
  double unused;
  cubic_hermite(fv[0], fv[1], fv[2], fv[3], tr, f, dfdr);
  cubic_hermite(dv[0], dv[1], dv[2], dv[3], tr, dfdc, unused);
}

__device__ inline void bicubic(const uint8_t* __restrict__ map, int size_x, int size_y, double r, double c,
                               double& f, double& dfdr, double& dfdc) {
  const double fr = floor(r), fc = floor(c);
  // keep the int conversion defined for wild coordinates; clamping below makes any far-outside index equivalent
  const double frc = fmin(fmax(fr, -4.0), (double)size_y + 4.0), fcc = fmin(fmax(fc, -4.0), (double)size_x + 4.0);
  const int row = (int)frc, col = (int)fcc;
  double fv[4], dv[4];
  int cc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) cc[j] = min(max(col - 1 + j, 0), size_x - 1);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int rr = min(max(row - 1 + i, 0), size_y - 1);
    const uint8_t* p = map + (size_t)rr * size_x;
    cubic_hermite((double)p[cc[0]], (double)p[cc[1]], (double)p[cc[2]], (double)p[cc[3]], c - fc, fv[i], dv[i]);
  }
  double unused;
  cubic_hermite(fv[0], fv[1], fv[2], fv[3], r - fr, f, dfdr);
  cubic_hermite(dv[0], dv[1], dv[2], dv[3], r - fr, dfdc, unused);
}

}  // namespace smpc
