// smpc_tracker_rule.hpp — the rule of the people tracker (include/smpc_tracker.h states the contract): which slots are
// live, the prediction, the gate and the association key, the alpha-beta update, the counters of a hit and of a miss, and
// the key of the output order. Plain double arithmetic with one rounding per operation; no HIP call, no include beyond
// <stdint.h>: the kernel (smpc_tracker.hpp) and a host-only program (tests/test_tracker.py) compile the same functions.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SMPC_TK_HD __host__ __device__
#else
#define SMPC_TK_HD
#endif

namespace smpc {

constexpr int32_t kTrackFree = 0, kTrackTentative = 1, kTrackConfirmed = 2;
constexpr int32_t kTrackMaxHits = 1 << 30;
constexpr uint64_t kTrackNoKey = ~0ull;  // above the bits of every double >= +0, +inf included

SMPC_TK_HD inline bool tk_finite(double v) { return __builtin_fabs(v) <= 1.7976931348623157e308; }  // false for NaN and inf

// step 0: a slot stays when its state is 1 or 2 and its four doubles are finite
SMPC_TK_HD inline bool tk_live(int32_t state, double x, double y, double vx, double vy) {
  return (state == kTrackTentative || state == kTrackConfirmed) && tk_finite(x) && tk_finite(y) && tk_finite(vx) && tk_finite(vy);
}

// step 1, one axis: xp = x + vx * dt
SMPC_TK_HD inline double tk_predict(double x, double v, double dt) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  const double step = v * dt;
  return x + step;
}

// step 3: d2 = rx * rx + ry * ry of the residual (rx, ry) = z - predicted; never negative, never -0
SMPC_TK_HD inline double tk_d2(double rx, double ry) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  const double xx = rx * rx, yy = ry * ry;
  return xx + yy;
}

SMPC_TK_HD inline double tk_gate2(double gate) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  return gate * gate;
}

SMPC_TK_HD inline uint64_t tk_bits(double v) {
  uint64_t b;
  __builtin_memcpy(&b, &v, sizeof(double));
  return b;
}

// The association key of a pair: the bit pattern of d2 when the pair qualifies (a double >= +0 orders as its integer),
// kTrackNoKey when it does not (a NaN never passes the gate). The order of the pairs is (key, slot, detection).
SMPC_TK_HD inline uint64_t tk_pair_key(double zx, double zy, double xp, double yp, double gate2) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  const double rx = zx - xp, ry = zy - yp;
  const double d2 = tk_d2(rx, ry);
  return d2 <= gate2 ? tk_bits(d2) : kTrackNoKey;
}

// step 4, one axis: the position xp + alpha * r and the velocity v + gain * r of a matched slot, r = z - xp
SMPC_TK_HD inline double tk_update(double base, double k, double r) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  const double c = k * r;
  return base + c;
}

SMPC_TK_HD inline int32_t tk_hit(int32_t hits) { return hits >= kTrackMaxHits ? kTrackMaxHits : hits + 1; }

// step 5: missed + 1 in 32-bit two's complement
SMPC_TK_HD inline int32_t tk_miss(int32_t missed) { return (int32_t)((uint32_t)missed + 1u); }

// step 5: does a slot that has just missed (its counter already incremented) stay?
SMPC_TK_HD inline bool tk_survives_miss(int32_t state, int32_t missed, int32_t max_missed) {
  return state == kTrackConfirmed && !(missed > max_missed);
}

SMPC_TK_HD inline int32_t tk_birth_state(int32_t confirm_hits) { return confirm_hits <= 1 ? kTrackConfirmed : kTrackTentative; }

// step 7: the key of the output order, (key, slot): the bits of dr2 = ddx * ddx + ddy * ddy, formed as the nearest rule
// forms it; kTrackNoKey when dr2 is not finite
SMPC_TK_HD inline uint64_t tk_out_key(double x, double y, double rx, double ry) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  const double ddx = x - rx, ddy = y - ry;
  const double dr2 = tk_d2(ddx, ddy);
  return tk_finite(dr2) ? tk_bits(dr2) : kTrackNoKey;
}

SMPC_TK_HD inline bool tk_key_less(uint64_t ad, uint32_t ai, uint64_t bd, uint32_t bi) { return ad < bd || (ad == bd && ai < bi); }

}  // namespace smpc
