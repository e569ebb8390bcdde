/* smpc_plan_repair.h — plan repair: detours around the impassable cells a robot's own window shows on its plan, beside
 * include/smpc.h (whose list of structs and functions is unchanged, as is SMPC_ABI_VERSION). Same library, same handle, same
 * error codes, same staging of host-pointer calls, smpc_last_kernel_ms() covers the call's kernels.
 * The global plans (include/smpc_global_plan.h) are made once over the static world map; the windows of a tick hold what the
 * scan marked (smpc_sensed_costmap_batch, smpc_obstacle_memory_batch). Every tick, a robot whose plan runs into impassable
 * cells of its window gets the least-cost detour inside a square region of the window around itself, spliced into its plan:
 * the integer step costs and the walk rule of the global plans, restricted to the region. This is the library's own rule,
 * the place a deployment's planner server takes (about 1 Hz on a costmap with an obstacle layer); the reference controller has
 * no counterpart. The call has no state. Not covered: restoring the first plan once the obstacle has left, regions beyond
 * SMPC_REPAIR_MAX_RADIUS, and the segments between two poses — only the cells of the poses are tested. */
#ifndef SMPC_PLAN_REPAIR_H
#define SMPC_PLAN_REPAIR_H

#include "smpc.h"
#include "smpc_global_plan.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SMPC_REPAIR_MAX_RADIUS 63

enum smpc_repair_status {
  SMPC_REPAIR_CLEAR = 0,               /* no blocked pose in view: nothing to do */
  SMPC_REPAIR_REPAIRED = 1,            /* the detour is spliced in, plan_len is the new length */
  SMPC_REPAIR_NO_PLAN = 2,             /* rule 1, or no pose with a finite distance (rule 3) */
  SMPC_REPAIR_NO_CELL = 3,             /* the robot has no cell in its window */
  SMPC_REPAIR_NO_REJOIN = 4,           /* no pose behind the blocked stretch, in view, to come back to */
  SMPC_REPAIR_UNREACHABLE = 5,         /* no path inside the region */
  SMPC_REPAIR_TOO_LONG = 6,            /* the repaired plan would have more than L rows */
  SMPC_REPAIR_INCONSISTENT_FIELD = 7   /* a bug: the field did not settle, or the walk found no next cell */
};

typedef struct smpc_plan_repair_in {
  int32_t B;                    /* robots, >= 0 */
  int32_t L;                    /* rows of a plan, >= 2 */
  int32_t on_device;            /* 0 host pointers, 1 device pointers (outputs follow) */
  int32_t size_x, size_y;       /* the window, as smpc_scene_batch reads it: cells, >= 1 */
  int32_t costmap_shared;       /* 1: one costmap and origin for all robots */
  int32_t radius;               /* R: the region's half side in cells, 1..SMPC_REPAIR_MAX_RADIUS */
  int32_t stride;               /* every stride-th cell of the detour becomes a pose, >= 1 */
  double resolution;            /* finite and > 0 */
  double clearance_d2;          /* finite and >= 0: squared rejoin clearance, metres^2 */
  smpc_plan_cost_params cost;
  const uint8_t* costmap;       /* [B or 1][size_y][size_x] */
  const double* costmap_origin; /* [B or 1][2] */
  const double* robot_pose;     /* [B][3]; x, y are read */
  const int32_t* plan_start;    /* [B] or NULL (0 for every robot): the path handler's erased prefix */
} smpc_plan_repair_in;

/* ---- The rule (csrc/smpc_plan_repair_rule.hpp; the kernels: csrc/smpc_plan_repair.hpp) --------------------------------------
 * Per robot b, with (x, y) of robot_pose[b], its window W (costmap, origin, size) and S = 2 R + 1. Every double operation is
 * rounded on its own (no fused multiply-add). The cell of a point and the centre of a cell are those of
 * smpc_global_plan.h, per axis, with the window's origin and size; passable(c), w(c), the step costs, the diagonal rule
 * and the neighbour order are that header's too. d2(p, q) = (px - qx) * (px - qx) + (py - qy) * (py - qy): two products and
 * one sum. The steps are checked in this order.
 * 1. Plan. n = plan_len[b], s = plan_start[b] (0 without plan_start). n < 2, n > L, s < 0 or s >= n: NO_PLAN.
 * 2. Robot cell. a is the cell of (x, y); none: NO_CELL. The region is the set of window cells c with
 *    max(|cx - ax|, |cy - ay|) <= R.
 * 3. Closest pose. i0 is the least i in [s, n) that minimises d2(plan[i], (x, y)). A d2 that is not finite never wins; none
 *    finite: NO_PLAN.
 * 4. The stretch in view. e is the least i >= i0 whose pose has no cell in the region, or n. A pose i in [i0, e) is blocked
 *    when its cell is not passable and is not a. No blocked pose (e == i0 included): CLEAR. i1 and i2 are the least and
 *    the greatest blocked index.
 * 5. Rejoin. j is the least index in (i2, e) whose cell is passable and with d2(plan[j], plan[i2]) >= clearance_d2: the
 *    clearance keeps the rejoin out of the unseen back of the obstacle. None: NO_REJOIN. t is the cell of pose j.
 * 6. Field. F is the fixed point of the global plans' rule restricted to the region: F(t) = 0; a step from c into an
 *    8-neighbour d costs 5 w(d) along an axis and 7 w(d) along a diagonal, a diagonal step only when both cells sharing an
 *    edge with c and d are passable; cell a counts as passable whatever its cost, with w(a) = neutral_cost + cost_weight *
 *    cost(a); cells outside the region or the window do not exist. F(a) unreachable: UNREACHABLE.
 * 7. Walk. From c = a, while F(c) != 0, go to the first neighbour d in the neighbour order that is passable (or a), allowed
 *    by the diagonal rule and has F(d) + k w(d) == F(c) exactly. The cells are c0 = a .. cm. No such neighbour, more than
 *    S * S steps, or a field that has not settled within S * S sweeps: INCONSISTENT_FIELD (a bug; reported per robot, no host
 *    read-back).
 * 8. Splice. Rows 0 .. i0 - 1 stay; row i0 becomes (x, y); then the centres of c[k * stride], k = 1, 2, .. while
 *    k * stride < m; then the old rows j .. n - 1. The new length n' > L: TOO_LONG. Otherwise REPAIRED and plan_len[b] = n';
 *    rows from n' on are not written.
 * 9. Untouched rows. With any status but REPAIRED not one byte of the robot's plan rows or of plan_len[b] changes. A robot's
 *    outputs depend on that robot's inputs alone: not on B, its place in the batch, the memory space or timing.
 * 10. field, when given, for the robots that reached step 6 (UNREACHABLE, INCONSISTENT_FIELD, TOO_LONG, REPAIRED): cell
 *    (fx, fy) of the row is window cell a - (R, R) + (fx, fy) and holds F(c) where F(c) <= F(a), taking the marker of an
 *    unreachable F(a) as the largest value, and SMPC_FIELD_UNREACHABLE everywhere else (cells outside the window or
 *    impassable included). A cell with F(c) > F(a) cannot lie on the walk, so the kernel stops relaxing such cells. After
 *    a field that did not settle (INCONSISTENT_FIELD by sweeps) the row's contents are unspecified. Other robots' rows are
 *    not written.
 * info[b] = (i0, i1, j, m), each -1 where the robot's status left it undetermined: CLEAR knows i0; NO_REJOIN i0 and i1;
 * UNREACHABLE and INCONSISTENT_FIELD i0, i1 and j; TOO_LONG and REPAIRED all four.
 *
 * SMPC_ERR_INVALID_ARG (nothing launched, nothing written): a NULL handle, input, costmap, costmap_origin, robot_pose, plan,
 * plan_len, workspace or status; B < 0; L < 2; size_x or size_y < 1; radius < 1; stride < 1; a resolution or clearance_d2
 * that is not finite; resolution <= 0; clearance_d2 < 0; neutral_cost < 1; cost_weight < 0; neutral_cost + 255 * cost_weight
 * > 65535. SMPC_ERR_UNSUPPORTED: radius > SMPC_REPAIR_MAX_RADIUS, or S * S * 7 * (neutral_cost + 255 * cost_weight) >=
 * 2^32 - 1 (no potential can then overflow or collide with the marker). B == 0 succeeds and writes nothing.
 * With device pointers two kernels on the handle's stream, no allocation and no host synchronisation (capturable in a HIP
 * graph); host pointers are staged like everywhere (the host workspace is then not touched). */
int smpc_repair_plan_batch(smpc_handle* h, const smpc_plan_repair_in* in,
                           double*   plan       /* [B][L][2] in / out */,
                           int32_t*  plan_len   /* [B] in / out */,
                           double*   workspace  /* [B][L][2]; contents unspecified afterwards */,
                           int32_t*  status     /* [B] out: enum smpc_repair_status */,
                           int32_t*  info       /* [B][4] out or NULL: i0, i1, j, m */,
                           uint32_t* field      /* [B][S][S] out or NULL, S = 2 * radius + 1 */);

#ifdef __cplusplus
}
#endif

#endif
