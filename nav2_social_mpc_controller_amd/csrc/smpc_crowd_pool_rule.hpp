// smpc_crowd_pool_rule.hpp — the host-compilable part of the rule of the shared pool's crowd step
// (include/smpc_crowd_pool.h states the contract): who is a partner, the range gate (smpc_nearest_rule.hpp's own, reused)
// and the order-free sum of rule 4. Plain arithmetic, no HIP call, no include beyond <stdint.h> and the gather's rule: the
// kernel (smpc_crowd_pool.hpp) and a host-only program (tests/test_crowd_pool.py) compile the same functions.
#pragma once
#include <stdint.h>

#include "smpc_nearest_rule.hpp"

namespace smpc {

constexpr int kCpFractionBits = 36;
constexpr double kCpScale = 68719476736.0;            // 2^36
constexpr double kCpInvScale = 1.0 / 68719476736.0;   // 2^-36, exact
constexpr double kCpClamp = 8.0;
constexpr int64_t kCpMaxPartners = (1 << 24) - 1;     // A <= SMPC_NEAREST_MAX_ROWS, and a row is not its own partner

// rule 1: a row takes part (as a mover that moves, or as anybody's partner) when x, y, vx and vy are finite
SMPC_NN_HD inline bool cp_live(double x, double y, double vx, double vy) {
  return nn_finite(x) && nn_finite(y) && nn_finite(vx) && nn_finite(vy);
}

// rule 2: the gate of a live partner at (ax, ay) seen from a mover at (rx, ry)
SMPC_NN_HD inline bool cp_interacts(double rx, double ry, double ax, double ay, double interaction_range) {
  return nn_in_range(nn_d2(rx, ry, ax, ay), interaction_range);
}

// rule 4: one component of a pair term as an integer of 2^-36: round-to-nearest-even(clamp(t, -8, 8) * 2^36), 0 for a NaN.
// The product is exact (a power of two, no overflow); |q| <= 2^39.
SMPC_NN_HD inline int64_t cp_quantize(double t) {
  if (t != t) return 0;
  t = t < -kCpClamp ? -kCpClamp : (t > kCpClamp ? kCpClamp : t);
  return (int64_t)__builtin_rint(t * kCpScale);  // (the default rounding mode: to nearest, ties to even)
}

// rule 4: the force component of a sum of quantized terms
SMPC_NN_HD inline double cp_force(int64_t sum) { return (double)sum * kCpInvScale; }

// the worst case of rule 4's bound: every partner at the clamp
static_assert(kCpMaxPartners * ((int64_t)1 << 39) < INT64_MAX, "the sum of 2^24 - 1 clamped terms fits int64");

}  // namespace smpc
