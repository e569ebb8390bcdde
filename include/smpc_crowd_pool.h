/* smpc_crowd_pool.h — the reactive Social-Force step of a shared world's pedestrians, beside include/smpc.h (whose list of
 * structs and functions is unchanged, as is SMPC_ABI_VERSION). Same library, same handle, same error codes, same staging of
 * host-pointer calls, smpc_last_kernel_ms() covers the call's kernels.
 * smpc_crowd_step_batch moves private per-robot rows; this call moves ONE table of agents, the one smpc_nearest_people_batch
 * gathers from (include/smpc_nearest.h): rows 0 .. M-1 are pedestrians that move ("movers"), rows M .. A-1 are partners that
 * do not (in an episode: the robots). A mover gives way to every row within interaction_range; the cut-off is the library's
 * own rule (include/nav2_social_mpc_controller/sfm.hpp:237-281 sums over every agent). With a range that covers the whole
 * table the step is the reference's computeForces + updatePosition on all agents, up to the rounding of rule 4. */
#ifndef SMPC_CROWD_POOL_H
#define SMPC_CROWD_POOL_H

#include "smpc_nearest.h"

#ifdef __cplusplus
extern "C" {
#endif

/* rule 4: a component of a pair term is summed as round-to-nearest-even(t * 2^36), t clamped to [-8, 8] */
#define SMPC_CROWD_POOL_FRACTION_BITS 36
#define SMPC_CROWD_POOL_TERM_CLAMP 8.0

typedef struct smpc_crowd_pool_in {
  int32_t M;                      /* movers: rows 0 .. M-1 of `agents`, 0 <= M <= A */
  int32_t A;                      /* rows of `agents` */
  int32_t K;                      /* waypoint slots per mover, 1..SMPC_MAX_WAYPOINTS */
  int32_t on_device;
  int32_t cyclic;                 /* a mover past its last waypoint heads for the first again */
  int32_t bins_ready;             /* device pointers only: `workspace` already holds the bins of this very table (below) */
  int32_t grid_x, grid_y;         /* bins, >= 1 each, grid_x * grid_y <= 65536 */
  double grid_origin[2];          /* finite */
  double bin_size;                /* finite, >= interaction_range * SMPC_NEAREST_BIN_MARGIN */
  double interaction_range;       /* finite, > 0 */
  double dt;                      /* finite, > 0 */
  double goal_radius, person_radius, desired_speed; /* as smpc_crowd_batch */
  const double* agents;           /* [A][5] x, y, vx, vy, vz; never written */
  const double* waypoints;        /* [M][K][2] */
  const int32_t* n_waypoints;     /* [M] */
  const double* desired_speeds;   /* [M], or NULL: desired_speed for everybody */
  const uint32_t* od_indexes;     /* [od_height][od_width] ONE ObstacleDistance grid (smpc_crowd_batch with od_shared), or NULL */
  const double* od_origin;        /* [2] */
  int32_t od_width, od_height;
  float od_resolution;
  int32_t reserved0;
  void* workspace;                /* device memory, smpc_nearest_workspace_bytes(A, grid_x, grid_y); may be NULL with on_device == 0 */
  uint64_t workspace_bytes;
} smpc_crowd_pool_in;

/* ---- The rule (csrc/smpc_crowd_pool_rule.hpp; the kernel: csrc/smpc_crowd_pool.hpp) ---------------------------------------
 * Per mover i < M:
 * 1. Inert rows. A mover whose x, y, vx or vy is not finite is inert: next[i] is its row, all five doubles bit for bit,
 *    and cursor[i] is not written. Row c is a partner of i only when c != i and its x, y, vx and vy are all finite.
 * 2. Range gate. Partner c interacts when d2 <= interaction_range * interaction_range, with d2 and the comparison exactly
 *    those of include/smpc_nearest.h rule 2 (nn_d2 / nn_in_range of csrc/smpc_nearest_rule.hpp).
 * 3. Pair term. The term of one partner is smpc_crowd_step_batch's (include/smpc.h, computeSocialForce sfm.hpp:237-281 with
 *    the constants of csrc/smpc_sfm.hpp): diff = partner - mover, dv = the mover's velocity - the partner's; a pair closer
 *    than 1e-6 m takes diff = (1e-6, 0), on both sides; equal velocities take theta = 0.
 * 4. Order-free sum. Each component t of a term becomes the integer q = round-to-nearest-even(t * 2^36): 0 for a NaN,
 *    otherwise after t is clamped to [-8, 8]. The social force is (double)(sum of the q in int64) * 2^-36 per component.
 *    Integer addition is associative: the force does not depend on the order the partners are met in, hence not on the
 *    bins, the grid, the place of a row in the table or the arrival order of any atomic. A component is at most
 *    2.1 * sqrt(2) < 8 in magnitude and a mover has at most A - 1 <= 2^24 - 1 partners, so |sum| <= (2^24 - 1) * 2^39 < 2^63.
 * 5. Forces and update. Desired force (sfm.hpp:188-203), += social force, += obstacle force (sfm.hpp:205-222) from the
 *    nearest obstacle of the mover's grid cell; none when od_indexes is NULL, the cell lies off the grid or its entry is
 *    not a cell of the grid. Then updatePosition (sfm.hpp:525-572) exactly as smpc_crowd_step_batch does it: velocity,
 *    speed cap at the mover's desired speed, vz = wrap(new heading - old heading) / dt, position, and the cursor:
 *    a mover with a goal (0 <= cursor < min(max(n_waypoints, 0), K)) within goal_radius of it after the move advances,
 *    and with `cyclic` a cursor at or past the end goes back to 0.
 * 6. Synchronous update. `next` is written from the old table alone: rows of `agents` are never written, and a `next`
 *    that overlaps agents[0 .. A) is refused.
 * 7. Independence. A mover's next row and cursor depend on the table, its own waypoints / speed / cursor and the
 *    parameters alone: not on M, its place in the table, the memory space, the stream, timing, or the bins.
 *
 * Bins are the gather's (include/smpc_nearest.h): the bin of a point, row-major in x, and the 3 x 3 block around the mover's
 * bin. bin_size >= interaction_range * SMPC_NEAREST_BIN_MARGIN; the proof there carries over word for word with
 * R = interaction_range (a mover takes the robot's place).
 * bins_ready == 0: the call bins the table itself (the gather's memset + count + scan + scatter) and then steps.
 * bins_ready == 1 (device pointers): the caller vouches that `workspace` was filled by a smpc_nearest_people_batch, or by an
 * earlier step, on this very agents, A, grid_x, grid_y, grid_origin and bin_size, and that `agents` has not changed since;
 * the call launches the step kernel alone.
 *
 * SMPC_ERR_INVALID_ARG (nothing launched, nothing written): a NULL handle or input; NULL agents with A > 0; NULL next,
 * cursor, waypoints or n_waypoints with M > 0; M < 0, M > A, A < 0, K < 1, grid_x < 1 or grid_y < 1; a grid_origin that is
 * not finite; bin_size, interaction_range or dt not finite or not > 0; bin_size < interaction_range *
 * SMPC_NEAREST_BIN_MARGIN; goal_radius or person_radius negative or NaN; desired_speed not > 0; od_indexes without
 * od_origin or with od_width < 1, od_height < 1 or od_resolution not > 0; `next` overlapping agents; with on_device, a NULL
 * workspace or workspace_bytes < smpc_nearest_workspace_bytes(A, grid_x, grid_y). SMPC_ERR_UNSUPPORTED: K >
 * SMPC_MAX_WAYPOINTS, grid_x * grid_y > 65536, A > 2^24. M == 0 succeeds, launches nothing and writes nothing.
 * Device pointers: a fixed sequence on the handle's stream (bins_ready == 0: one asynchronous memset and four kernels;
 * bins_ready == 1: one kernel), no allocation and no host synchronisation (capturable in a HIP graph). Host pointers:
 * staged like the gather; the library provides the workspace and ignores bins_ready. */

int smpc_crowd_pool_step_batch(smpc_handle* h, const smpc_crowd_pool_in* in,
                               double* next    /* [M][5] */,
                               int32_t* cursor /* [M], in/out */);

#ifdef __cplusplus
}
#endif

#endif
