// smpc_global_plan_rule.hpp — the rule of the global plans (include/smpc_global_plan.h states the contract): which cells
// are passable and what entering one costs, the neighbour table, the diagonal test, the cell of a point and the centre of
// a cell. Integer arithmetic for costs, plain double arithmetic with one rounding per operation for the geometry; no HIP
// call, no include beyond <stdint.h>: the kernels (smpc_global_plan.hpp) and a host-only program
// (tests/test_global_plan.py) compile the same functions.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SMPC_GP_HD __host__ __device__
#else
#define SMPC_GP_HD
#endif

namespace smpc {

constexpr uint32_t kFieldUnreachable = 0xFFFFFFFFu;

struct GpCost {
  int32_t neutral, weight;  // w = neutral + weight * cost, 1 <= w <= 65535 (checked by the host)
  uint32_t lethal_min;      // cost >= lethal_min is impassable
  uint32_t allow_unknown;   // ... except 255 when set
};

SMPC_GP_HD inline bool gp_passable(const GpCost& c, uint32_t v) { return v < c.lethal_min || (c.allow_unknown != 0u && v == 255u); }

// w(c) of a passable cell; 0 marks an impassable one (a weight is >= 1)
SMPC_GP_HD inline uint32_t gp_weight(const GpCost& c, uint32_t v) {
  return gp_passable(c, v) ? (uint32_t)c.neutral + (uint32_t)c.weight * v : 0u;
}

// neighbour k = 0..7 as (dx, dy): (1,0) (0,1) (-1,0) (0,-1) (1,1) (-1,1) (-1,-1) (1,-1), two bits per entry (value + 1)
SMPC_GP_HD inline int gp_dx(int k) { return (int)((0x8246u >> (2 * k)) & 3u) - 1; }
SMPC_GP_HD inline int gp_dy(int k) { return (int)((0x0A19u >> (2 * k)) & 3u) - 1; }
SMPC_GP_HD inline uint32_t gp_step_factor(int k) { return k < 4 ? 5u : 7u; }

// Cost of the step into neighbour k, whose weight is wn; wa and wb are the weights of the two cells that share an edge
// with both ends of a diagonal step (ignored along an axis). 0: the step is not allowed.
SMPC_GP_HD inline uint32_t gp_step_cost(int k, uint32_t wn, uint32_t wa, uint32_t wb) {
  if (wn == 0u) return 0u;
  if (k >= 4 && (wa == 0u || wb == 0u)) return 0u;
  return gp_step_factor(k) * wn;
}

// one axis: the cell of point p; false: p is not finite or its cell lies outside 0 .. size - 1
SMPC_GP_HD inline bool gp_cell_axis(double p, double origin, double res, int32_t size, int32_t* cell) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  const double d = p - origin;
  const double q = __builtin_floor(d / res);
  if (!(q >= 0.0 && q < (double)size)) return false;  // a NaN lands here too
  *cell = (int32_t)q;
  return true;
}

// one axis: the centre of cell i: the sum i + 0.5, then the product, then the sum
SMPC_GP_HD inline double gp_centre(double origin, int32_t i, double res) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  const double s = (double)i + 0.5;
  const double m = s * res;
  return origin + m;
}

}  // namespace smpc
