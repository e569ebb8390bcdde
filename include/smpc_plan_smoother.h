/* smpc_plan_smoother.h — plan smoothing: the grid paths of the global plans are relaxed before the controller reads them,
 * beside include/smpc.h (whose list of structs and functions is unchanged, as is SMPC_ABI_VERSION). Same library, same handle,
 * same error codes, same staging of host-pointer calls, smpc_last_kernel_ms() covers the call's kernel.
 * The global plans (include/smpc_global_plan.h) are 8-connected walks down an integer field: over free floor an octile
 * staircase, and a zigzag that turns at every cell where inflation gradients tilt the field. The plan window, the
 * trajectorizer, the path-align critic, the goal heading and the plan repair's closest-pose search all read those rows as they
 * are. This call moves the inner rows of every plan towards the mean of their neighbours while a data term holds them to where
 * they started, and never moves a row into a cell that is not passable. It takes the place Nav2's smoother server has between
 * the planner and the controller. The rule is the library's own, modelled on Nav2's simple smoother as recalled (a data
 * weight, a smoothness weight, a tolerance, an iteration cap and refinement rounds; its defaults as recalled: 0.2, 0.3, 1e-10,
 * 1000, 2): recalled, not restated from its source. It departs from it on purpose where a sequential sweep and a summed change
 * would make the result depend on the order of the rows: a sweep here is a Jacobi sweep, and its change is a maximum. The call
 * has no state. Not covered: pose orientations, and the segments between two poses — only the cells of the poses are tested. */
#ifndef SMPC_PLAN_SMOOTHER_H
#define SMPC_PLAN_SMOOTHER_H

#include "smpc.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SMPC_SMOOTH_MAX_POSES 1024
#define SMPC_SMOOTH_MAX_ITS 100000
#define SMPC_SMOOTH_MAX_REFINEMENTS 8

enum smpc_smooth_status {
  SMPC_SMOOTH_CONVERGED = 0,       /* every round ended with a sweep whose change was <= tolerance */
  SMPC_SMOOTH_REACHED_MAX_ITS = 1, /* MAX_ITS: a round ran max_its sweeps; its last iterate is kept, no further round */
  SMPC_SMOOTH_TOO_SHORT = 2,       /* no movable row: nothing written to the plan */
  SMPC_SMOOTH_BAD_PLAN = 3         /* a coordinate that is not finite among the first n rows: nothing written to the plan */
};

typedef struct smpc_plan_smoother_in {
  int32_t B;                    /* robots, >= 0 */
  int32_t L;                    /* rows of a plan, 2 .. SMPC_SMOOTH_MAX_POSES */
  int32_t on_device;            /* 0 host pointers, 1 device pointers (outputs follow) */
  int32_t world_x, world_y;     /* cells of a map, >= 1 */
  int32_t world_shared;         /* 1: one map and origin for all robots; 0: one per robot (e.g. the robots' own windows) */
  int32_t max_its;              /* sweeps of a round at the most, 1 .. SMPC_SMOOTH_MAX_ITS */
  int32_t refinement_num;       /* rounds after the first, 0 .. SMPC_SMOOTH_MAX_REFINEMENTS */
  int32_t lethal_min_cost;      /* a cell of cost >= lethal_min_cost is impassable ... */
  int32_t allow_unknown;        /* ... except, when != 0, a cell of exactly 255 */
  double resolution;            /* finite and > 0 */
  double w_data;                /* finite and > 0 */
  double w_smooth;              /* finite and >= 0; w_data + 4 * w_smooth < 2 */
  double tolerance;             /* >= 0 (+inf allowed) */
  const uint8_t* world;         /* [B or 1][world_y][world_x] */
  const double* world_origin;   /* [B or 1][2] */
  const int32_t* plan_len;      /* [B] */
  const int32_t* range;         /* [B][2] or NULL: the first and the last row that may move */
} smpc_plan_smoother_in;

/* ---- The rule (csrc/smpc_plan_smoother_rule.hpp; the kernel: csrc/smpc_plan_smoother.hpp) ---------------------------------
 * Per robot b, with its rows plan[b] and its map M (world, origin, size). Every double operation is rounded on its own (no
 * fused multiply-add), in the order written.
 * 1. Row count and status. n = min(max(plan_len[b], 0), L). A coordinate that is not finite among rows 0 .. n - 1: BAD_PLAN
 *    (checked first). Otherwise first = max(range[b][0], 1) and last = min(range[b][1], n - 2), without range first = 1 and
 *    last = n - 2; n < 3 or first > last: TOO_SHORT. In both cases none of the robot's plan rows is written, info[b] =
 *    (0, 0, 0, n) and change[b] = +0.0.
 * 2. Fixed rows. The movable rows are first .. last. Every other row (0, n - 1, the rows from n on, the rows outside range)
 *    never changes, bit for bit; the rows from n on are not even read. A fixed row is a neighbour like any other.
 * 3. One sweep (Jacobi: every candidate is formed from the previous iterate y; p are the rows the round started from). For a
 *    movable row i, per axis:
 *        a = p_i - y_i;  b = w_data * a;  s = y_(i+1) + y_(i-1);  d = y_i + y_i;  e = s - d;  f = w_smooth * e;  g = b + f;
 *        c = y_i + g.
 *    The candidate (c_x, c_y) is accepted when it has a cell in M and that cell is passable. The cell of a point is that of
 *    smpc_global_plan.h, per axis: floor((c - origin) / resolution); a coordinate that is not finite, or a cell outside
 *    0 .. world_x - 1 (0 .. world_y - 1), is no cell. Passable: cost < lethal_min_cost, or cost == 255 when allow_unknown is
 *    set. An accepted row becomes the candidate; a rejected row keeps y_i for this sweep. The sweep's change is the largest
 *    |h|, h = c - y_i, over the accepted rows and both axes: a maximum, so the order of the rows does not matter; +0.0 when
 *    no row was accepted.
 * 4. Rounds. The first round starts with p = y = the plan's rows. A round ends at the first sweep whose change is <=
 *    tolerance (that sweep's rows are kept); a round that has run max_its sweeps without such a sweep ends there, its last
 *    iterate is kept, and the status is MAX_ITS: no further round. After a round that converged, while fewer than
 *    refinement_num refinements have run, the next round (a refinement) starts with p := y. When no round is left the
 *    status is CONVERGED.
 * 5. Outputs. status[b]; info[b] = (sweeps over all rounds, rounds ended — the MAX_ITS round counts —, rejected candidates
 *    summed over all sweeps and saturating at INT32_MAX, n); change[b]: the change of the last sweep.
 * 6. Independence. A robot's outputs depend on that robot's rows, plan_len, range and map alone: not on B, its place in the
 *    batch, the memory space or timing.
 * Why w_data + 4 * w_smooth < 2: on an unobstructed plan the sweep multiplies the error mode of angle t by
 * 1 - w_data - 2 * w_smooth * (1 - cos t), which lies inside (-1, 1) for every t exactly under this condition and w_data > 0.
 *
 * SMPC_ERR_INVALID_ARG (nothing launched, nothing written): a NULL handle, input, world, world_origin, plan_len, plan or
 * status; B < 0; L < 2; world_x or world_y < 1; a resolution that is not finite or not > 0; w_data not finite or <= 0;
 * w_smooth not finite or < 0; w_data + 4 * w_smooth >= 2 (the sum of the double product and w_data); a tolerance that is NaN
 * or < 0; max_its < 1; refinement_num < 0. SMPC_ERR_UNSUPPORTED: L > SMPC_SMOOTH_MAX_POSES, max_its > SMPC_SMOOTH_MAX_ITS,
 * refinement_num > SMPC_SMOOTH_MAX_REFINEMENTS, or world_x * world_y >= 2^31. B == 0 succeeds and writes nothing.
 * With device pointers one kernel on the handle's stream, no allocation and no host synchronisation (capturable in a HIP
 * graph); every loop of the kernel is bounded by max_its * (refinement_num + 1). Host pointers are staged like everywhere. */
int smpc_smooth_plan_batch(smpc_handle* h, const smpc_plan_smoother_in* in,
                           double*  plan    /* [B][L][2] in / out: smoothed in place */,
                           int32_t* status  /* [B] out: enum smpc_smooth_status */,
                           int32_t* info    /* [B][4] out or NULL: sweeps, rounds, rejected, n */,
                           double*  change  /* [B] out or NULL */);

#ifdef __cplusplus
}
#endif

#endif
