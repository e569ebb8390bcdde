// smpc_detector.hpp — people detections (include/smpc_detector.h; the rule: smpc_detector_rule.hpp): per robot, the persons
// it was handed become what a detector would report of them: persons hidden behind another person's body and persons the
// detector misses leave, the others are reported with a position noise that grows with range, and clutter candidates that
// exist this tick are appended. Every random number is Philox4x32-10 at the counter (tick, stream id, row, purpose).
//   One wavefront per robot, four robots per workgroup, no s_barrier. Lane j owns person j and later clutter candidate j.
//   * Lane j writes its offset (dx, dy) from the robot into the wave's own 64 + 64 doubles of LDS (zeros where the person is
//     not usable, so no word of it is read unwritten); a ballot of the usable lanes is the wave-uniform mask.
//   * Occlusion: the set bits of that mask are walked with broadcast LDS reads, each step a few FP64 operations; the loop
//     ends early when every lane of the wave is hidden or unusable. Skipped altogether when body_radius == 0.
//   * Draws: at most four Philox calls per lane (miss, noise x, noise y, clutter), each 40 32-bit multiplies. The miss draw
//     is skipped when miss_threshold == 0 and the clutter draw when clutter_threshold == 0 (a draw is never below 0), the
//     noise draws by every lane that is not detected or whose scale is 0.
//   * Output rows by ballot ranks: the rank of a detected lane is the number of detected lanes below it; the clutter ranks
//     start at the number of detected persons.
//   Bounds: the entry point admits 1 <= Np, Nd <= 64 and 0 <= Kc <= 64 only. Every LDS index is a lane number or a bit
//   number of a 64-bit mask masked with 63; global rows are lane < clamp(count, 0, Np) of people and outcome, rank < Nd of
//   detections and det_source (from lanes < n or lanes < Kc), of robot b < B; lane 0 alone writes det_count[b] and
//   draw_state[b][1].
// Plain vector loads and stores, no atomics.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "smpc_math.hpp"
#include "smpc_detector_rule.hpp"

namespace smpc {

constexpr int kDtThreads = 256;  // four wavefronts = four robots

struct DetectorParams {
  int B, Np, Nd, Kc;
  uint32_t seed_lo, seed_hi, miss_threshold, clutter_threshold;
  double body_radius, noise_scale, noise_growth, clutter_scale;
  const double* people;      // [B][Np][5]
  const int32_t* count;      // [B]
  const double* robot_pose;  // [B][3]
  uint32_t* draw_state;      // [B][2]
  double* detections;        // [B][Nd][5]
  int32_t* det_count;        // [B]
  int32_t* det_source;       // [B][Nd] or null
  uint8_t* outcome;          // [B][Np] or null
};

__global__ __launch_bounds__(kDtThreads) void smpc_detect_people_kernel(const DetectorParams p) {
  SMPC_CHAIN_PRIORITY();
  __shared__ double off_x[kDtThreads / 64][64];
  __shared__ double off_y[kDtThreads / 64][64];
  const int lane = (int)(threadIdx.x & 63u);
  const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const long long b = (long long)blockIdx.x * (kDtThreads / 64) + w;
  if (b >= p.B) return;  // wave-uniform
  const size_t s = (size_t)b;
  const int Np = p.Np, Nd = p.Nd;
  const uint64_t below = (1ull << lane) - 1ull;  // the lanes before this one

  // step 0: the state; the counter advances whatever happens (lane 0's store, at either exit)
  const uint32_t stream = p.draw_state[2 * s], tick = p.draw_state[2 * s + 1];
  const int n = min(max(p.count[s], 0), Np);
  const bool mine = lane < n;
  uint8_t* const outcome = p.outcome ? p.outcome + s * (size_t)Np + (size_t)(mine ? lane : 0) : nullptr;

  // step 1
  const double rx = p.robot_pose[3 * s], ry = p.robot_pose[3 * s + 1];
  if (!(dt_finite(rx) && dt_finite(ry))) {  // wave-uniform
    if (mine && outcome) *outcome = kDetectNotFinite;
    if (lane == 0) { p.det_count[s] = 0; p.draw_state[2 * s + 1] = tick + 1u; }
    return;
  }
  double row[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  if (mine) {
    const double* src = p.people + (s * (size_t)Np + (size_t)lane) * 5;
    for (int c = 0; c < 5; ++c) row[c] = src[c];
  }
  const bool usable = mine && dt_finite(row[0]) && dt_finite(row[1]);

  // step 2: offsets into the wave's LDS, then the walk over the usable persons
  const double dx = usable ? dt_offset(row[0], rx) : 0.0, dy = usable ? dt_offset(row[1], ry) : 0.0;
  const double dd = dt_dd(dx, dy);
  bool hidden = false;
  if (p.body_radius > 0.0) {  // wave-uniform
    off_x[w][lane] = dx;
    off_y[w][lane] = dy;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const double r2 = dt_r2(p.body_radius);
    for (uint64_t m = __ballot(usable); m != 0ull; m &= m - 1ull) {
      const int k = __builtin_amdgcn_readfirstlane(__builtin_ctzll(m)) & 63;
      const bool hides = dt_occludes(dx, dy, dd, off_x[w][k], off_y[w][k], r2);
      hidden = hidden || (k != lane && hides);
      if (__ballot(usable && !hidden) == 0ull) break;  // wave-uniform: nobody is left to hide
    }
  }

  // step 3
  bool detected = usable && !hidden;
  uint8_t code = !usable ? kDetectNotFinite : hidden ? kDetectBodyOccluded : kDetectDetected;
  if (detected && p.miss_threshold != 0u &&
      dt_missed(dt_philox(tick, stream, (uint32_t)lane, kDrawMiss, p.seed_lo, p.seed_hi).w[0], p.miss_threshold)) {
    detected = false;
    code = kDetectMissed;
  }
  if (mine && outcome) *outcome = code;

  // step 4
  const double scale = dt_scale(p.noise_scale, p.noise_growth, dd);
  if (detected && scale != 0.0) {
    row[0] = dt_noisy(row[0], dt_noise_sum(dt_philox(tick, stream, (uint32_t)lane, kDrawNoiseX, p.seed_lo, p.seed_hi)), scale);
    row[1] = dt_noisy(row[1], dt_noise_sum(dt_philox(tick, stream, (uint32_t)lane, kDrawNoiseY, p.seed_lo, p.seed_hi)), scale);
  }

  // step 6, the persons
  const uint64_t det_mask = __ballot(detected);
  const int n_det = (int)__builtin_popcountll(det_mask);
  const int rank = (int)__builtin_popcountll(det_mask & below);
  if (detected && rank < Nd) {
    double* dst = p.detections + (s * (size_t)Nd + (size_t)rank) * 5;
    for (int c = 0; c < 5; ++c) dst[c] = row[c];
    if (p.det_source) p.det_source[s * (size_t)Nd + (size_t)rank] = lane;
  }

  // step 5 and the rest of step 6: the clutter
  bool exists = false;
  double cx = 0.0, cy = 0.0;
  if (lane < p.Kc && p.clutter_threshold != 0u) {
    const DtWords d = dt_philox(tick, stream, (uint32_t)lane, kDrawClutter, p.seed_lo, p.seed_hi);
    exists = dt_clutter_exists(d.w[0], p.clutter_threshold);
    cx = dt_clutter_xy(rx, d.w[1], p.clutter_scale);
    cy = dt_clutter_xy(ry, d.w[2], p.clutter_scale);
  }
  const uint64_t clutter_mask = __ballot(exists);
  const int crank = n_det + (int)__builtin_popcountll(clutter_mask & below);
  if (exists && crank < Nd) {
    double* dst = p.detections + (s * (size_t)Nd + (size_t)crank) * 5;
    dst[0] = cx; dst[1] = cy; dst[2] = 0.0; dst[3] = 0.0; dst[4] = 0.0;
    if (p.det_source) p.det_source[s * (size_t)Nd + (size_t)crank] = -1 - lane;
  }
  if (lane == 0) {
    p.det_count[s] = min(Nd, n_det + (int)__builtin_popcountll(clutter_mask));
    p.draw_state[2 * s + 1] = tick + 1u;
  }
}

}  // namespace smpc
