// smpc_detector_rule.hpp — the rule of the people detector (include/smpc_detector.h states the contract): the generator
// (Philox4x32-10), a person's offset from the robot, the body-occlusion test, the miss test, the noise sum, scale and noisy
// coordinate, and the clutter candidates. This is the library's own rule; the reference has no counterpart. Plain integer
// and double arithmetic with one rounding per operation; no HIP call, no include beyond <stdint.h>: the kernel
// (smpc_detector.hpp) and a host-only program (tests/test_detector.py) compile the same functions.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SMPC_DT_HD __host__ __device__
#else
#define SMPC_DT_HD
#endif

namespace smpc {

constexpr uint8_t kDetectDetected = 0, kDetectBodyOccluded = 1, kDetectMissed = 2, kDetectNotFinite = 3;
// the `purpose` word of a draw's counter
constexpr uint32_t kDrawMiss = 0u, kDrawNoiseX = 1u, kDrawNoiseY = 2u, kDrawClutter = 3u;

struct DtWords { uint32_t w[4]; };

// Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11) with the published
// constants: ten rounds, the key bumped between rounds. draw(t, s, i, purpose) = dt_philox(t, s, i, purpose, seed_lo, seed_hi).
SMPC_DT_HD inline DtWords dt_philox(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
  for (int round = 0; round < 10; ++round) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1; c3 = (uint32_t)p0; c0 = n0; c2 = n2;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  return DtWords{{c0, c1, c2, c3}};
}

SMPC_DT_HD inline bool dt_finite(double v) { return __builtin_fabs(v) <= 1.7976931348623157e308; }  // false for NaN and inf

// step 2, one axis: a person's offset from the robot
SMPC_DT_HD inline double dt_offset(double p, double r) { return p - r; }

// step 2: dd = dx * dx + dy * dy
SMPC_DT_HD inline double dt_dd(double dx, double dy) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  const double xx = dx * dx, yy = dy * dy;
  return xx + yy;
}

SMPC_DT_HD inline double dt_r2(double body_radius) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  return body_radius * body_radius;
}

// step 2: does the person at offset e hide the person at offset d (dd = dt_dd(d)) from the robot? e's centre projects
// strictly inside the sight segment (0 < tk < dd) and lies within the body radius of its line (cr^2 <= r2 * dd). The round
// caps beyond the segment's ends are not tested. Every comparison with a NaN is false: an overflowed product hides nobody.
SMPC_DT_HD inline bool dt_occludes(double dx, double dy, double dd, double ex, double ey, double r2) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  const double txx = ex * dx, tyy = ey * dy;
  const double tk = txx + tyy;
  const double cxy = ex * dy, cyx = ey * dx;
  const double cr = cxy - cyx;
  const double cr2 = cr * cr;
  const double lim = r2 * dd;
  return tk > 0.0 && tk < dd && cr2 <= lim;
}

// step 3
SMPC_DT_HD inline bool dt_missed(uint32_t w0, uint32_t miss_threshold) { return w0 < miss_threshold; }

// step 4: the four words' sum, centred: an exact integer in [-(2^33 - 2), 2^33 - 2], symmetric about 0
SMPC_DT_HD inline int64_t dt_noise_sum(const DtWords& d) {
  return (int64_t)((uint64_t)d.w[0] + (uint64_t)d.w[1] + (uint64_t)d.w[2] + (uint64_t)d.w[3]) - (int64_t)((1ull << 33) - 2ull);
}

// step 4: scale = noise_scale + noise_growth * dd
SMPC_DT_HD inline double dt_scale(double noise_scale, double noise_growth, double dd) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  const double g = noise_growth * dd;
  return noise_scale + g;
}

// step 4, one axis: z = p + (double)s * scale
SMPC_DT_HD inline double dt_noisy(double p, int64_t s, double scale) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  const double e = (double)s * scale;
  return p + e;
}

// step 5
SMPC_DT_HD inline bool dt_clutter_exists(uint32_t w0, uint32_t clutter_threshold) { return w0 < clutter_threshold; }

// step 5, one axis: r + (double)(int32_t)w * clutter_scale
SMPC_DT_HD inline double dt_clutter_xy(double r, uint32_t w, double clutter_scale) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  const double e = (double)(int32_t)w * clutter_scale;
  return r + e;
}

}  // namespace smpc
