// smpc_plant_rule.hpp — the rule of the robot plant (include/smpc_plant.h states the contract): the rate limits, the points
// of the period's segment, the cell of a point, which cells are walls, the footprint's offsets and the keys of the two
// clearances. Plain double arithmetic with one rounding per operation, exact integer arithmetic for the cells; no HIP call,
// no include beyond <stdint.h> and, for the heading, smpc_math.hpp: the kernel (smpc_plant.hpp) and a host-only program
// (tests/test_plant.py) compile the same functions.
#pragma once
#include <stdint.h>

#include "smpc_math.hpp"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SMPC_PL_HD __host__ __device__
#else
#define SMPC_PL_HD
#endif

namespace smpc {

constexpr int32_t kPlantBlockedByWall = 1, kPlantBlockedByAgent = 2, kPlantWallContact = 4, kPlantAgentContact = 8,
                  kPlantBadCommand = 16, kPlantBadState = 32;
constexpr int kPlantMaxSubsteps = 16, kPlantMaxLatency = 8, kPlantMaxFootprintD2 = 225;
constexpr uint32_t kPlantNoWall = ~0u;    // above every squared offset
constexpr uint64_t kPlantNoAgent = ~0ull; // above the bits of every double >= +0, +inf included

SMPC_PL_HD inline bool pl_finite(double v) { return __builtin_fabs(v) <= 1.7976931348623157e308; }  // false for NaN and inf

// lo when a < lo, else hi when a > hi, else a (a NaN stays; hi may be +inf)
SMPC_PL_HD inline double pl_clamp(double a, double lo, double hi) { return a < lo ? lo : (a > hi ? hi : a); }

// step 3, the linear axis: v1 = v + clamp(delta, -lim, lim) with lim = up when the speed moves away from zero, else down
SMPC_PL_HD inline double pl_limit_v(double v, double target, double v_min, double v_max, double up, double down) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  const double vt = pl_clamp(target, v_min, v_max);
  const double delta = vt - v;
  const double lim = ((v >= 0.0 && delta >= 0.0) || (v <= 0.0 && delta <= 0.0)) ? up : down;
  const double step = pl_clamp(delta, -lim, lim);
  return v + step;
}

// step 3, the angular axis: one limit in both directions
SMPC_PL_HD inline double pl_limit_w(double w, double target, double w_max, double dw) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  const double wt = pl_clamp(target, -w_max, w_max);
  const double delta = wt - w;
  const double step = pl_clamp(delta, -dw, dw);
  return w + step;
}

// step 4: cosine and sine of the heading, as the kernels of the tick chain obtain them (t: a MathTab)
template <class TabP>
SMPC_PL_HD inline void pl_heading(TabP t, double theta, double* c, double* s) {
  if (__builtin_expect(!(__builtin_fabs(theta) <= 1e5), 0)) {
#if defined(__HIP_DEVICE_COMPILE__)
    sincos(theta, s, c);
#else
    *s = sin(theta); *c = cos(theta);
#endif
  } else {
    sincos_tab(t, theta, s, c);
  }
}

// step 5: one axis of the period's segment, (v1 * c) * dt
SMPC_PL_HD inline double pl_length(double v1, double c, double dt) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  const double vc = v1 * c;
  return vc * dt;
}

// step 5: one axis of q_k, x + L * (k / S), 1 <= k <= S
SMPC_PL_HD inline double pl_point(double x, double L, int k, int S) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  const double f = (double)k / (double)S;
  const double d = L * f;
  return x + d;
}

// step 7: theta + w1 * dt
SMPC_PL_HD inline double pl_turn(double theta, double w1, double dt) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  const double d = w1 * dt;
  return theta + d;
}

// step 6: the cell of q; false: a coordinate is not finite or beyond 2^30 in magnitude (a NaN lands here too)
SMPC_PL_HD inline bool pl_cell(double qx, double qy, double ox, double oy, double res, int32_t* cx, int32_t* cy) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  const double dx = qx - ox, dy = qy - oy;
  const double fx = __builtin_floor(dx / res), fy = __builtin_floor(dy / res);
  if (!(__builtin_fabs(fx) <= 1073741824.0 && __builtin_fabs(fy) <= 1073741824.0)) return false;
  *cx = (int32_t)fx; *cy = (int32_t)fy;
  return true;
}

struct PlantWalls {
  const uint8_t* world;  // [Hy][Hx]; null: no walls
  int32_t Hx, Hy;
  int32_t footprint_d2;  // < 0: no walls
  int32_t r;             // floor(sqrt(footprint_d2)): the bounding square of the offsets has the side 2 r + 1
  int32_t min_cost, unknown, outside;
};

SMPC_PL_HD inline int32_t pl_isqrt(int32_t d2) {
  int32_t r = 0;
  while ((r + 1) * (r + 1) <= d2) ++r;
  return r;
}

SMPC_PL_HD inline bool pl_walls_on(const PlantWalls& w) { return w.world != nullptr && w.footprint_d2 >= 0; }

// is world cell (x, y) a wall? |x|, |y| <= 2^30 + 15
SMPC_PL_HD inline bool pl_is_wall(const PlantWalls& w, int32_t x, int32_t y) {
  if (x < 0 || y < 0 || x >= w.Hx || y >= w.Hy) return w.outside != 0;
  const int32_t cost = (int32_t)w.world[(uint64_t)y * (uint64_t)w.Hx + (uint64_t)x];
  return cost == 255 ? w.unknown != 0 : cost >= w.min_cost;
}

// step 6: offset t of the bounding square, 0 <= t < (2 r + 1)^2, row by row: its squared length when it lies within the
// footprint and its cell is a wall, else kPlantNoWall
SMPC_PL_HD inline uint32_t pl_offset_key(const PlantWalls& w, int32_t cx, int32_t cy, int32_t t) {
  const int32_t side = 2 * w.r + 1;
  const int32_t jy = t / side - w.r, jx = t - (t / side) * side - w.r;
  const int32_t d2 = jx * jx + jy * jy;
  if (d2 > w.footprint_d2) return kPlantNoWall;
  return pl_is_wall(w, cx + jx, cy + jy) ? (uint32_t)d2 : kPlantNoWall;
}

SMPC_PL_HD inline double pl_contact2(double contact_dist) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  return contact_dist * contact_dist;
}

SMPC_PL_HD inline uint64_t pl_bits(double v) {
  uint64_t b;
  __builtin_memcpy(&b, &v, sizeof(double));
  return b;
}

// step 6: the key of one agent at (px, py) seen from q: the bits of d2 when it is in contact, else kPlantNoAgent (a NaN or
// an infinite d2 never is below contact2)
SMPC_PL_HD inline uint64_t pl_agent_key(double px, double py, double qx, double qy, double contact2) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  const double ax = px - qx, ay = py - qy;
  const double xx = ax * ax, yy = ay * ay;
  const double d2 = xx + yy;
  return d2 < contact2 ? pl_bits(d2) : kPlantNoAgent;
}

}  // namespace smpc
