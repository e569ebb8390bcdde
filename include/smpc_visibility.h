/* smpc_visibility.h — the line-of-sight filter of the people a robot perceives on a world map, beside include/smpc.h (whose
 * list of structs and functions is unchanged, as is SMPC_ABI_VERSION). Same library, same handle, same error codes, same
 * staging of host-pointer calls, smpc_last_kernel_ms() covers the call's kernel.
 * This is the library's own rule: the reference controller has no counterpart (it takes every person of people_msgs::People
 * that its field-of-view cone lets through). It runs in front of smpc_people_to_status_batch. */
#ifndef SMPC_VISIBILITY_H
#define SMPC_VISIBILITY_H

#include "smpc.h"

#ifdef __cplusplus
extern "C" {
#endif

/* seen[b][j] */
enum smpc_seen_code {
  SMPC_SEEN_HIDDEN = 0,         /* an occluding cell lies on the sight line */
  SMPC_SEEN_SEEN = 1,
  SMPC_SEEN_OUT_OF_RANGE = 2,   /* farther than max_range */
  SMPC_SEEN_NOT_FINITE = 3      /* the robot or the person has no cell */
};

typedef struct smpc_visibility_in {
  int32_t B, Np;                /* Np: row stride of people, >= 1 */
  int32_t on_device;
  int32_t world_x, world_y;     /* >= 1, world_x * world_y < 2^31 */
  int32_t world_shared;         /* 1: one world map and origin for all robots */
  uint8_t occlusion_min_cost;   /* a cell with cost >= this blocks sight (default 254) */
  uint8_t unknown_occludes;     /* 0: cost 255 never blocks sight */
  uint8_t reserved[2];
  double resolution;            /* finite, > 0 */
  double max_range;             /* detector range in metres, finite, > 0 */
  const uint8_t* world;         /* [B or 1][world_y][world_x] */
  const double* world_origin;   /* [B or 1][2] */
  const double* robot_pose;     /* [B][3]; x, y are read */
  const double* people;         /* [B][Np][5] as smpc_people_batch.people */
  const int32_t* count;         /* [B], clamped to 0..Np as people_to_status does */
} smpc_visibility_in;

/* ---- The rule (csrc/smpc_visibility_rule.hpp; the kernel: csrc/smpc_visibility.hpp) --------------------------------------
 * Per person j < count[b], in this order:
 * 1. Cells. The cell of a point on one axis is q = floor((p - origin) / resolution), computed in double, every operation
 *    rounded on its own; a cell outside the world is legal here. If the robot's x or y is not finite, or |q| <= 2^30 does
 *    not hold for one of the robot's two q (a NaN among them), every person of that robot gets NOT_FINITE. A person whose x
 *    or y is not finite gets NOT_FINITE.
 * 2. Range. ddx = px - rx, ddy = py - ry; the person passes when ddx * ddx + ddy * ddy <= max_range * max_range (two
 *    products, a sum and a product, each rounded on its own), else OUT_OF_RANGE.
 * 3. Sight line: exact integer geometry on the segment between the CENTRES of the robot's cell a and the person's cell b.
 *    A cell occludes when it lies inside the world and cost >= occlusion_min_cost && (cost != 255 || unknown_occludes);
 *    cells outside the world are transparent, and a and b themselves never occlude. The person is HIDDEN when some cell
 *    whose open interior the segment meets occludes, and also when the segment passes exactly through a lattice corner and
 *    BOTH cells that touch it only at that corner occlude (one alone does not: sight passes a corner). a == b: SEEN.
 *    As a walk: dx = |bx - ax|, dy = |by - ay|, unit steps sx, sy, i = j = 0; until (i, j) == (dx, dy) compare
 *    A = (2i + 1) * dy with Bv = (2j + 1) * dx: A < Bv step i, A > Bv step j, equal: test the cells (i + 1, j) and (i, j + 1)
 *    as a pair, then step both; after each step test the new cell unless it is b. The rule is symmetric in a and b.
 * 4. Outputs. SEEN persons are copied, all five doubles bit for bit, to visible[b][0 .. visible_count[b] - 1] in their
 *    original order; rows from visible_count[b] on are NOT written, nor is seen[b][j] for j >= count[b]. A robot's outputs
 *    depend on that robot's inputs alone. visible / visible_count go straight into smpc_people_batch.people / count: the
 *    field-of-view filter and the truncation to N agents come after, and since all three keep the order, the result is
 *    that of any order of the filters.
 *
 * SMPC_ERR_INVALID_ARG (nothing launched, nothing written): a NULL handle, input, visible, visible_count, world,
 * world_origin, robot_pose, people or count; B < 0; Np < 1; world_x or world_y < 1; a resolution or max_range that is not
 * finite or not > 0. SMPC_ERR_UNSUPPORTED: max_range / resolution > 32768 (a ray then spans at most 32769 cells per axis
 * and every product of the walk fits 32 unsigned bits), world_x * world_y >= 2^31.
 * For device pointers one kernel on the handle's stream, no allocation and no host synchronisation (capturable in a HIP
 * graph). */
int smpc_visible_people_batch(smpc_handle* h, const smpc_visibility_in* in,
                              double* visible        /* [B][Np][5] */,
                              int32_t* visible_count /* [B] */,
                              uint8_t* seen          /* [B][Np] or NULL */);

#ifdef __cplusplus
}
#endif

#endif
