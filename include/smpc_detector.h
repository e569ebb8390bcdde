/* smpc_detector.h — people detections: a detector model between the line-of-sight filter and the tracker, beside
 * include/smpc.h (whose list of structs and functions is unchanged, as is SMPC_ABI_VERSION). Same library, same handle,
 * same error codes, same staging of host-pointer calls, smpc_last_kernel_ms() covers the call's kernel.
 * This is the library's own rule: the reference controller has no counterpart (it is handed people_msgs::People by a
 * perception stack of the deployment's own). The rows the world map lets a robot see are ground truth: everybody detected
 * every tick, at the exact position, nobody invented, and a person seen through the person in front. This call turns them
 * into what a detector would report: occlusion by other people's bodies, missed detections, position noise that grows with
 * range, and clutter (false detections). All randomness comes from a counter-based generator, so the result is a pure
 * function of (seed, the robot's stream id, the robot's tick counter, the row index): no lane, batch position, stream,
 * shard or graph replay enters it. `detections` / `det_count` go straight into smpc_tracker_in.detections / det_count, or
 * into smpc_people_batch.people / count when there is no tracker. */
#ifndef SMPC_DETECTOR_H
#define SMPC_DETECTOR_H

#include "smpc.h"

#ifdef __cplusplus
extern "C" {
#endif

/* outcome[b][j] */
enum smpc_detect_outcome {
  SMPC_DETECT_DETECTED = 0,
  SMPC_DETECT_BODY_OCCLUDED = 1,
  SMPC_DETECT_MISSED = 2,
  SMPC_DETECT_NOT_FINITE = 3
};

typedef struct smpc_detector_in {
  int32_t B;
  int32_t Np;                  /* row stride of people, 1..SMPC_MAX_AGENTS */
  int32_t Nd;                  /* row stride of detections, 1..SMPC_MAX_AGENTS */
  int32_t Kc;                  /* clutter candidates per robot and tick, 0..SMPC_MAX_AGENTS */
  int32_t on_device;
  int32_t reserved;
  uint32_t seed_lo;            /* the generator's key */
  uint32_t seed_hi;
  uint32_t miss_threshold;     /* a usable person is missed when its draw < this: p_miss = threshold / 2^32 */
  uint32_t clutter_threshold;  /* candidate c exists when its draw < this */
  double body_radius;          /* >= 0; 0 disables body occlusion */
  double noise_scale;          /* >= 0; sigma0 * sqrt(3) / 2^32, formed by the caller */
  double noise_growth;         /* >= 0; added per m^2 of squared range, same unit as noise_scale */
  double clutter_scale;        /* >= 0; clutter_range / 2^31, formed by the caller */
  const double*  people;       /* [B][Np][5] smpc_people_batch.people rows */
  const int32_t* count;        /* [B], clamped to 0..Np */
  const double*  robot_pose;   /* [B][3]; x, y are read */
} smpc_detector_in;

/* ---- The rule (csrc/smpc_detector_rule.hpp; the kernel: csrc/smpc_detector.hpp) -------------------------------------------
 * Every floating-point operation is rounded on its own (no fused multiply-add).
 * The generator is Philox4x32-10 with the published constants (multipliers 0xD2511F53 and 0xCD9E8D57, key increments
 * 0x9E3779B9 and 0xBB67AE85, ten rounds, the key bumped between rounds). draw(t, s, i, purpose) is the four 32-bit words
 * of Philox with counter (t, s, i, purpose) and key (seed_lo, seed_hi).
 * Per robot b:
 * 0. State. s = draw_state[b][0], t = draw_state[b][1], n = clamp(count[b], 0, Np). After the call draw_state[b][1] = t + 1
 *    in unsigned 32-bit arithmetic, whatever else happens to the robot; draw_state[b][0] is never written. All zero is a
 *    valid state.
 * 1. Finite. If the robot's x or y is not finite: det_count[b] = 0, no row is written and outcome[b][j] = NOT_FINITE for
 *    j < n. Otherwise person j < n is usable when its x and y are finite; an unusable person gets NOT_FINITE, is not
 *    reported and occludes nobody.
 * 2. Body occlusion. For usable j: dx = px - rx, dy = py - ry, dd = dx * dx + dy * dy. j is BODY_OCCLUDED when
 *    body_radius > 0 and some usable k != j, with e its offset from the robot formed like d, satisfies all of
 *    tk = ex * dx + ey * dy > 0, tk < dd, and cr * cr <= (body_radius * body_radius) * dd with cr = ex * dy - ey * dx:
 *    k's centre projects strictly inside the sight segment and lies within body_radius of its line. The round caps beyond
 *    the segment's two ends are NOT tested: a body whose centre projects behind the robot or beyond the person hides
 *    nobody, however near the end it stands. A comparison with a NaN is false, so an overflowed product hides nobody. The
 *    result does not depend on the order in which k is visited.
 * 3. Miss. A usable, unoccluded j is MISSED when draw(t, s, j, 0)[0] < miss_threshold. Draws are addressed by j, so
 *    whether one person is missed never depends on another.
 * 4. Noise. For each detected j: sx = (int64)(w0 + w1 + w2 + w3) - (2^33 - 2) with w = draw(t, s, j, 1); sy the same with
 *    purpose 2. An exact integer, symmetric about 0, |s| < 2^34, of standard deviation sqrt((2^64 - 1) / 3).
 *    scale = noise_scale + noise_growth * dd. If scale == 0 the row is the person's, all five doubles bit for bit.
 *    Otherwise zx = px + (double)sx * scale, zy = py + (double)sy * scale, and columns 2 to 4 are copied bit for bit
 *    (without a tracker smpc_people_to_status_batch still reads the velocities as before; the tracker never reads them).
 *    A z that is not finite is written as it is; the tracker's step 2 discards it. That includes a scale that is a NaN
 *    (noise_growth = 0 times a dd that overflowed to infinity): a NaN is not 0.
 * 5. Clutter. Candidate c < Kc exists when w0 < clutter_threshold with w = draw(t, s, c, 3). Its row is
 *    rx + (double)(int32_t)w1 * clutter_scale, ry + (double)(int32_t)w2 * clutter_scale, +0.0, +0.0, +0.0: uniform in a
 *    square of half-side clutter_range around the robot.
 * 6. Output. Detected persons first in ascending j, then the existing clutter candidates in ascending c. The first
 *    det_count[b] = min(Nd, their number) rows are written, with det_source = j of the person, or -1 - c for clutter
 *    candidate c. Rows from det_count[b] on are NOT written; outcome[b][j] is not written for j >= n.
 * 7. Independence. A robot's state and outputs depend on that robot's inputs and draw_state[b] alone: not on B, its place
 *    in the batch, the stream or timing.
 *
 * SMPC_ERR_INVALID_ARG (nothing launched, every buffer left alone, draw_state included): a NULL handle, input, draw_state,
 * detections, det_count, people, count or robot_pose; B < 0; Np or Nd < 1; Kc < 0; a body_radius, noise_scale,
 * noise_growth or clutter_scale that is not finite or is negative. SMPC_ERR_UNSUPPORTED: Np, Nd or Kc above
 * SMPC_MAX_AGENTS. B == 0 succeeds and writes nothing. For device pointers one kernel on the handle's stream, no
 * allocation and no host synchronisation (capturable in a HIP graph); host pointers are staged like everywhere,
 * draw_state both ways. */
int smpc_detect_people_batch(smpc_handle* h, const smpc_detector_in* in,
                             uint32_t* draw_state  /* [B][2] stream id, tick counter — state of the caller's, in place */,
                             double*   detections  /* [B][Nd][5] out */,
                             int32_t*  det_count   /* [B] out */,
                             int32_t*  det_source  /* [B][Nd] out or NULL: j of the person, or -1 - c for clutter candidate c */,
                             uint8_t*  outcome     /* [B][Np] out or NULL */);

#ifdef __cplusplus
}
#endif

#endif
