/* smpc_scan_people.h — people detections from the scan: a per-robot detector between the tick's laser scan and the tracker,
 * beside include/smpc.h (whose list of structs and functions is unchanged, as is SMPC_ABI_VERSION). Same library, same handle,
 * same error codes, same staging of host-pointer calls, smpc_last_kernel_ms() covers the call's kernel.
 * This is the library's own rule for the "leg detector" of a deployment's perception stack; the reference controller has no
 * counterpart (it is handed people). The call looks at the raw scan alone: the cells the tick's beams stopped at (beam_kind /
 * beam_cell as smpc_sensed_costmap_batch and smpc_obstacle_memory_batch write them). Neighbouring beams whose hits lie close
 * together form a segment, a segment of a person's size is a detection, and its centre, pushed back along the sight line by
 * the body's radius, goes into smpc_tracker_in.detections as it is. smpc_visible_people_batch and smpc_detect_people_batch,
 * which start from the simulator's own person rows, are the ground-truth alternative. The call has no state. */
#ifndef SMPC_SCAN_PEOPLE_H
#define SMPC_SCAN_PEOPLE_H

#include "smpc.h"
#include "smpc_sensed_costmap.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct smpc_scan_people_in {
  int32_t B;
  int32_t n_beams;          /* 1..SMPC_SENSED_MAX_BEAMS */
  int32_t Nd;               /* row stride of detections, 1..SMPC_MAX_AGENTS */
  int32_t on_device;
  int32_t subtract_map;     /* 0: WORLD hits are foreground too; 1: they are background (static-map subtraction) */
  int32_t min_points;       /* >= 1: a segment of fewer beams is rejected */
  int32_t link_d2;          /* >= 0: neighbouring hits within this squared cell distance are linked */
  int32_t width_d2_min;     /* >= 0: squared cell distance between a segment's first and last hit, lower gate */
  int32_t width_d2_max;     /* >= width_d2_min: upper gate */
  int32_t range_d2;         /* >= 0: a hit beyond this squared cell distance of the robot's cell is background */
  double resolution;        /* finite, > 0 */
  double world_origin[2];   /* finite */
  double body_offset;       /* finite, >= 0, metres: how far the centre is pushed away from the robot; 0: not at all */
  const double*  robot_pose;      /* [B][3]; x, y are read */
  const uint8_t* beam_kind;       /* [B][n_beams] enum smpc_beam_kind */
  const int32_t* beam_cell;       /* [B][n_beams][2] offsets from the robot's cell */
} smpc_scan_people_in;

/* ---- The rule (csrc/smpc_scan_people_rule.hpp; the kernel: csrc/smpc_scan_people.hpp) ---------------------------------------
 * Per robot b, with n = n_beams, (x, y) of robot_pose[b] and o_k = beam_cell[b][k] (ox, oy). Everything up to the position is
 * exact integer arithmetic.
 * 1. Cell. The robot's cell a is that of smpc_sensed_costmap.h rule 1 (per axis q = floor((p - origin) / resolution), every
 *    operation rounded on its own, finite x and y, |q| <= 2^30). A robot without a cell (a non-finite x or y included) gets
 *    det_count[b] = 0 and seg_stats[b] = (0, 0, 0, 0); no row is written, and the call is over for this robot.
 * 2. Foreground. Beam k is foreground when beam_kind[b][k] is AGENT or CORNER_PAIR, or WORLD when subtract_map == 0, and
 *    ox * ox + oy * oy <= range_d2 (the sum exact, in 64 bits). WORLD is by the scan's rule 2 exactly "the hit is an occluding
 *    cell of the map", so subtract_map = 1 is a deployment's static-map subtraction. Every other kind value (NONE, INVALID,
 *    NO_ROBOT, and the values above 5) is background, as is every beam beyond the range.
 * 3. Links. For n >= 2, beam k is linked to its predecessor (k - 1 + n) mod n when both are foreground and
 *    (ox_k - ox_pred)^2 + (oy_k - oy_pred)^2 <= link_d2. With n == 1 nothing is linked.
 * 4. Segments. A start is a foreground beam that is not linked to its predecessor. Its segment runs s, s + 1, .. (mod n) for
 *    as long as the next beam is linked to its predecessor; it may wrap from beam n - 1 to beam 0. If there are foreground
 *    beams but no start (every beam is linked to its predecessor: the robot is enclosed), there is one segment with s = 0 and
 *    m = n.
 * 5. Features. m: the segment's number of beams. S = (Sx, Sy): the sum of o_k over the segment's beams, duplicated cells as
 *    often as they occur. chord = (ox_first - ox_last)^2 + (oy_first - oy_last)^2 with first = s and last = (s + m - 1) mod n.
 * 6. Gates. A segment is rejected "by points" when m < min_points; otherwise "by width" when chord < width_d2_min or
 *    chord > width_d2_max; otherwise it is accepted.
 * 7. Position of an accepted segment; every floating-point operation is rounded on its own (no fused multiply-add), division
 *    and square root correctly rounded as IEEE 754 defines them. Per axis, with a the robot's cell on that axis:
 *    mean = (double)S / (double)m, c = origin + (((double)a + mean) + 0.5) * resolution, r = c - pose.
 *    d = sqrt(rx * rx + ry * ry). If body_offset > 0 and d is finite and > 0: k = body_offset / d, and per axis
 *    p = c + r * k (the centroid of the visible arc lies in front of the body's centre; the offset pushes it back along the
 *    sight line). Otherwise p = c.
 * 8. Output. The accepted segments in ascending s, the first det_count[b] = min(Nd, accepted) of them: detections row
 *    (px, py, +0.0, +0.0, +0.0) and det_segment row (s, m, Sx, Sy). Rows from det_count[b] on are NOT written.
 *    seg_stats[b] = (segments, rejected by points, rejected by width, accepted) counts all segments, whatever Nd.
 * 9. Independence. A robot's outputs depend on that robot's inputs alone: not on B, its place in the batch, the memory space,
 *    the stream or timing.
 *
 * SMPC_ERR_INVALID_ARG (nothing launched, every buffer left alone): a NULL handle, input, detections, det_count, robot_pose,
 * beam_kind or beam_cell; B < 0; n_beams < 1; Nd < 1; min_points < 1; a negative link_d2, width_d2_min, width_d2_max or
 * range_d2; width_d2_min > width_d2_max; subtract_map outside 0..1; a resolution that is not finite or not > 0; an origin
 * that is not finite; a body_offset that is negative or not finite. SMPC_ERR_UNSUPPORTED: n_beams above
 * SMPC_SENSED_MAX_BEAMS or Nd above SMPC_MAX_AGENTS. B == 0 succeeds and writes nothing. For device pointers one kernel on the
 * handle's stream, no allocation and no host synchronisation (capturable in a HIP graph); host pointers are staged like
 * everywhere. */
int smpc_scan_people_batch(smpc_handle* h, const smpc_scan_people_in* in,
                           double*  detections   /* [B][Nd][5] out: x, y, +0, +0, +0 — goes straight into smpc_tracker_in.detections */,
                           int32_t* det_count    /* [B] out */,
                           int32_t* det_segment  /* [B][Nd][4] out or NULL: start beam s, beams m, Sx, Sy */,
                           int32_t* seg_stats    /* [B][4] out or NULL: segments, rejected by points, rejected by width, accepted */);

#ifdef __cplusplus
}
#endif

#endif
