/* smpc_nearest.h — the nearest-agent gather of a shared world, beside include/smpc.h (whose list of structs and functions is
 * unchanged, as is SMPC_ABI_VERSION). Same library, same handle, same error codes, same staging of host-pointer calls,
 * smpc_last_kernel_ms() covers the call's kernels.
 * This is the library's own rule: the reference controller has no counterpart (it takes what people_msgs::People carries).
 * Every robot takes its at most Np nearest neighbours within the detector's range out of ONE table of agents (the shared
 * pedestrians, followed by the robots themselves), nearest first, as the rows smpc_visible_people_batch,
 * smpc_people_to_status_batch and smpc_episode_metrics_batch read. */
#ifndef SMPC_NEAREST_H
#define SMPC_NEAREST_H

#include "smpc.h"

#ifdef __cplusplus
extern "C" {
#endif

/* bin_size >= max_range * SMPC_NEAREST_BIN_MARGIN (the product of the two doubles): 1 + 2^-20 */
#define SMPC_NEAREST_BIN_MARGIN 1.00000095367431640625
#define SMPC_NEAREST_MAX_BINS 65536    /* grid_x * grid_y */
#define SMPC_NEAREST_MAX_ROWS 16777216 /* A <= 2^24 */

typedef struct smpc_nearest_in {
  int32_t B, Np;            /* robots; Np: row stride of the outputs, 1..SMPC_MAX_AGENTS */
  int32_t A;                /* rows of `agents`, >= 0 */
  int32_t on_device;
  int32_t grid_x, grid_y;   /* bins, >= 1 each, grid_x * grid_y <= 65536 */
  double grid_origin[2];    /* finite */
  double bin_size;          /* finite, >= max_range * SMPC_NEAREST_BIN_MARGIN */
  double max_range;         /* finite, > 0 */
  const double* agents;     /* [A][5] smpc_people_batch.people rows: x, y, vx, vy, vz (NULL only with A == 0) */
  const double* robot_pose; /* [B][3]; x, y are read */
  const int32_t* self;      /* [B] the row of `agents` that IS robot b and is skipped, or < 0; NULL: none */
  void* workspace;          /* device memory, smpc_nearest_workspace_bytes(A, grid_x, grid_y); may be NULL with on_device == 0 */
  uint64_t workspace_bytes;
} smpc_nearest_in;

/* ---- The rule (csrc/smpc_nearest_rule.hpp; the kernels: csrc/smpc_nearest.hpp) --------------------------------------------
 * Per robot b:
 * 1. If the robot's x or y is not finite, count[b] = 0 and nothing else of b is written.
 * 2. Agent c qualifies when c != self[b] (no self, or self[b] < 0: nobody is skipped), its x and y are finite, and
 *    ddx * ddx + ddy * ddy <= max_range * max_range with ddx = ax - rx, ddy = ay - ry: two products, a sum and a product,
 *    each rounded on its own (the range gate of include/smpc_visibility.h). Call the left side d2.
 * 3. The velocity columns are never examined.
 * 4. Chosen are the min(Np, number qualifying) smallest agents by the pair (d2, c), lexicographic: equal distances go to
 *    the lower row. (d2, c) is a total order, so the choice and its order are unique.
 * 5. They are written in that order: people[b][k] gets all five doubles of the row, bit for bit, source[b][k] gets c,
 *    count[b] their number.
 * 6. Rows and sources from count[b] on are NOT written.
 * 7. A robot's outputs depend on `agents`, its own pose and its own `self` alone: not on B, its place in the batch, the
 *    memory space, the stream, timing, or the bins.
 *
 * The bins are an accelerator and do not show in the result. The bin of a point on one axis is
 *     clamp(floor((p - grid_origin) / bin_size), 0, grid - 1)
 * computed in double, every operation rounded on its own, clamped before the conversion to an integer (a NaN goes to bin 0);
 * points outside the grid land in the border bins, and the function is monotone in p. Bins are row-major in x.
 * Why the 3 x 3 bins around the robot's bin hold every qualifying agent: d2 <= fl(R^2) gives |ax - rx| <= R (1 + 2^-51), so
 * with s = bin_size >= R (1 + 2^-20) the exact quotients (ax - o) / s and (rx - o) / s differ by at most 1 - 2^-21. If both
 * lie beyond the same end of the grid, the clamp gives both the border bin. Otherwise both lie within 65537 bins of the
 * origin, where each computed quotient is off by at most 2^-35 (a rounding of the difference, 2^17 s 2^-53, divided by s,
 * and a rounding of the quotient), so the computed ones differ by less than 1 and their floors by at most one.
 *
 * SMPC_ERR_INVALID_ARG (nothing launched, nothing written): a NULL handle, input, people, count or robot_pose; NULL agents
 * with A > 0; B < 0, A < 0, Np < 1, grid_x < 1 or grid_y < 1; a grid_origin that is not finite; a bin_size or max_range that
 * is not finite or not > 0; bin_size < max_range * SMPC_NEAREST_BIN_MARGIN; with on_device, a NULL workspace or
 * workspace_bytes < smpc_nearest_workspace_bytes(A, grid_x, grid_y). SMPC_ERR_UNSUPPORTED: Np > SMPC_MAX_AGENTS,
 * grid_x * grid_y > 65536, A > 2^24. B == 0 succeeds, launches nothing and writes nothing.
 * Device pointers: a fixed sequence of one asynchronous memset and four kernels (three with A == 0) on the handle's stream,
 * no allocation and no host synchronisation (capturable in a HIP graph). The workspace holds, in this order, int32
 * offsets [grid_x * grid_y + 1] (exclusive prefix sums of the bins' populations), int32 cursors [grid_x * grid_y] and
 * int32 rows [A] (the rows of `agents` with finite x and y, sorted by bin); its contents before the call do not matter and
 * after it they are valid until `agents` changes. Host pointers: staged, and the library provides the workspace. */

/* 4 * (2 * grid_x * grid_y + 1 + A) rounded up to a multiple of 256; 0 for arguments the call refuses */
uint64_t smpc_nearest_workspace_bytes(int32_t A, int32_t grid_x, int32_t grid_y);

int smpc_nearest_people_batch(smpc_handle* h, const smpc_nearest_in* in,
                              double* people  /* [B][Np][5] */,
                              int32_t* count  /* [B] */,
                              int32_t* source /* [B][Np] row of `agents`, or NULL */);

#ifdef __cplusplus
}
#endif

#endif
