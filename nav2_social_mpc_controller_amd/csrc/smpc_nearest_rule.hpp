// smpc_nearest_rule.hpp — the rule of the nearest-agent gather (include/smpc_nearest.h states the contract): the bin of a
// point, the squared distance with its range gate, and the order of the selection keys (d2, c). Plain double arithmetic
// with one rounding per operation; no HIP call, no include beyond <stdint.h>: the kernels (smpc_nearest.hpp) and a
// host-only program (tests/test_nearest.py) compile the same functions.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SMPC_NN_HD __host__ __device__
#else
#define SMPC_NN_HD
#endif

namespace smpc {

SMPC_NN_HD inline bool nn_finite(double v) { return __builtin_fabs(v) <= 1.7976931348623157e308; }  // false for NaN and inf

// one axis: clamp(floor((p - origin) / bin_size), 0, n - 1), clamped as a double; a NaN goes to bin 0. Monotone in p.
SMPC_NN_HD inline int32_t nn_bin_axis(double p, double origin, double bin_size, int32_t n) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  const double d = p - origin;
  const double q = __builtin_floor(d / bin_size);
  const double top = (double)(n - 1);
  if (!(q > 0.0)) return 0;
  return q >= top ? n - 1 : (int32_t)q;
}

// d2 = ddx * ddx + ddy * ddy: two products and a sum, each rounded on its own (never negative; NaN or inf when a
// coordinate is not finite or the products overflow)
SMPC_NN_HD inline double nn_d2(double rx, double ry, double ax, double ay) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  const double ddx = ax - rx, ddy = ay - ry;
  const double xx = ddx * ddx, yy = ddy * ddy;
  return xx + yy;
}

// the range gate: d2 <= max_range * max_range (false for a NaN)
SMPC_NN_HD inline bool nn_in_range(double d2, double max_range) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  const double r2 = max_range * max_range;
  return d2 <= r2;
}

// The selection key of a qualifying agent: the bit pattern of d2 (a finite double >= +0 orders as its integer), then the
// row. Keys of different rows are never equal.
struct NnKey {
  uint64_t d;
  uint32_t c;
};

SMPC_NN_HD inline NnKey nn_key(double d2, uint32_t c) {
  NnKey k;
  __builtin_memcpy(&k.d, &d2, sizeof(double));
  k.c = c;
  return k;
}

SMPC_NN_HD inline bool nn_key_less(uint64_t ad, uint32_t ac, uint64_t bd, uint32_t bc) { return ad < bd || (ad == bd && ac < bc); }

}  // namespace smpc
