/* smpc_tracker.h — people tracks: a per-robot tracker between detection and smpc_people_to_status_batch, beside
 * include/smpc.h (whose list of structs and functions is unchanged, as is SMPC_ABI_VERSION). Same library, same handle,
 * same error codes, same staging of host-pointer calls, smpc_last_kernel_ms() covers the call's kernel.
 * This is the library's own rule: the reference controller has no counterpart (it is handed people_msgs::People by a
 * tracker of the deployment's own). The simulator's rows carry the true velocity, and a person who steps out of sight is
 * gone from the rows within one control period. This call associates each tick's detections with tracks by position alone,
 * estimates the velocity with an alpha-beta filter, and coasts a track for a bounded time when its person is not detected.
 * It runs behind the line-of-sight filter (or whatever produces the tick's detections) and in front of
 * smpc_people_to_status_batch, which reads `people` / `count`. The state belongs to the caller, as the obstacle memory's
 * does: all zero means "no tracks", so an episode starts from zeroed buffers and there is no reset flag. */
#ifndef SMPC_TRACKER_H
#define SMPC_TRACKER_H

#include "smpc.h"

#ifdef __cplusplus
extern "C" {
#endif

/* track_meta[b][i][0] */
enum smpc_track_state {
  SMPC_TRACK_FREE = 0,
  SMPC_TRACK_TENTATIVE = 1,
  SMPC_TRACK_CONFIRMED = 2
};

typedef struct smpc_tracker_in {
  int32_t B;
  int32_t Nd;            /* row stride of detections, 1..SMPC_MAX_AGENTS */
  int32_t Nt;            /* track slots per robot, 1..SMPC_MAX_AGENTS */
  int32_t Np;            /* row stride of the outputs, 1..SMPC_MAX_AGENTS */
  int32_t on_device;
  int32_t confirm_hits;  /* >= 1 */
  int32_t max_missed;    /* >= 0 */
  int32_t reserved;
  double dt, alpha, gain, gate;   /* gain = beta / dt, formed by the caller; all finite, dt > 0, gate > 0, alpha and gain >= 0 */
  const double*  detections;  /* [B][Nd][5] smpc_people_batch.people rows; ONLY x and y are read */
  const int32_t* det_count;   /* [B], clamped to 0..Nd */
  const double*  robot_pose;  /* [B][3]; x, y are read */
} smpc_tracker_in;

/* ---- The rule (csrc/smpc_tracker_rule.hpp; the kernel: csrc/smpc_tracker.hpp) ---------------------------------------------
 * Per robot b, in this order; every floating-point operation is rounded on its own (no fused multiply-add). A slot is
 * tracks[b][i] = x, y, vx, vy with track_meta[b][i] = state, hits, missed, id; it is live when its state is 1 or 2.
 * 0. Sanitise. A slot whose state is not 1 or 2, or whose x, y, vx or vy is not finite, is freed. Freeing a slot writes its
 *    four doubles as +0.0 and its four ints as 0.
 * 1. Predict every live slot: xp = x + vx * dt, yp = y + vy * dt.
 * 2. Detections. Detection j < clamp(det_count[b], 0, Nd) is used when its x and y are finite. Columns 2 to 4 are never
 *    examined.
 * 3. Associate. A pair (live slot i, used detection j) qualifies when d2 = rx * rx + ry * ry <= gate * gate with
 *    rx = zx - xp, ry = zy - yp. Qualifying pairs are taken in ascending lexicographic order of (d2, i, j); a pair is
 *    accepted when neither its slot nor its detection has been accepted yet. (d2, i, j) is a total order, so the matching is
 *    unique and depends on no lane, atomic or memory space.
 * 4. Update every matched slot: x = xp + alpha * rx, vx = vx + gain * rx, the same for y; hits = min(hits + 1, 2^30),
 *    missed = 0; a tentative slot with hits >= confirm_hits becomes confirmed.
 * 5. Coast every unmatched live slot: x = xp, y = yp, velocity kept, missed += 1 (in 32-bit two's complement). A tentative
 *    slot that misses once is freed; a confirmed slot with missed > max_missed is freed.
 * 6. Birth. The unmatched used detections, in ascending j, each take the lowest slot that is free at this point (slots freed
 *    in steps 0 and 5 count). The new slot gets x, y = z, v = +0.0, hits = 1, missed = 0, id = next_id[b], and next_id[b] is
 *    incremented in unsigned 32-bit arithmetic; its state is confirmed when confirm_hits <= 1, else tentative. A detection
 *    that finds no free slot is dropped.
 * 7. Output. If the robot's x or y is not finite, count[b] = 0 and no row is written; steps 0 to 6 still ran. Otherwise the
 *    confirmed slots after steps 4 to 6 are ordered ascending by (dr2, slot), dr2 = ddx * ddx + ddy * ddy with
 *    ddx = x - robot x, ddy = y - robot y (two differences, two products, one sum, as in smpc_nearest.h); a dr2 that is not
 *    finite (a position that overflowed in this very call; step 0 frees the slot in the next) orders behind every finite one.
 *    The first count[b] = min(Np, their number) are written to people[b] as x, y, vx, vy, +0.0, with (slot, id) in
 *    out_track[b]; rows from count[b] on are NOT written. Nearest first keeps the truncation to N agents in
 *    smpc_people_to_status_batch meaningful, as in the shared world.
 * 8. Independence. A robot's state and outputs depend on that robot's inputs alone: not on B, its place in the batch, the
 *    stream or timing. tracks, track_meta and next_id are read and written in place; a robot's state is read only by the
 *    wavefront that writes it.
 *
 * SMPC_ERR_INVALID_ARG (nothing launched, every buffer left alone): a NULL handle, input, tracks, track_meta, next_id,
 * people, count, detections, det_count or robot_pose; B < 0; Nd, Nt or Np < 1; confirm_hits < 1; max_missed < 0; a dt,
 * alpha, gain or gate that is not finite; dt <= 0; gate <= 0; alpha < 0; gain < 0. SMPC_ERR_UNSUPPORTED: Nd, Nt or Np above
 * SMPC_MAX_AGENTS. B == 0 succeeds and writes nothing. For device pointers one kernel on the handle's stream, no allocation
 * and no host synchronisation (capturable in a HIP graph); host pointers are staged like everywhere, the state both ways. */
int smpc_track_people_batch(smpc_handle* h, const smpc_tracker_in* in,
                            double*  tracks      /* [B][Nt][4] x, y, vx, vy — state, read and written in place */,
                            int32_t* track_meta  /* [B][Nt][4] state, hits, missed, id — state, in place */,
                            int32_t* next_id     /* [B] — state, in place */,
                            double*  people      /* [B][Np][5] out */,
                            int32_t* count       /* [B] out */,
                            int32_t* out_track   /* [B][Np][2] slot, id of each output row; or NULL */);

#ifdef __cplusplus
}
#endif

#endif
