/* smpc_global_plan.h — global plans on a world map: goal fields and plan extraction, beside include/smpc.h (whose list of
 * structs and functions is unchanged, as is SMPC_ABI_VERSION). Same library, same handle, same error codes, same staging
 * of host-pointer calls, smpc_last_kernel_ms() covers each call's kernel. */
#ifndef SMPC_GLOBAL_PLAN_H
#define SMPC_GLOBAL_PLAN_H

#include "smpc.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- The rule (csrc/smpc_global_plan_rule.hpp; the kernels: csrc/smpc_global_plan.hpp) ----------------------------------
 * The costs are this library's own integer rule, not a restatement of NavFn: every cost and potential is an integer, so a
 * field is the unique fixed point of its world and goal and can be compared bit for bit, whatever order it was relaxed in.
 *   passable(c):  world[c] < lethal_min_cost, or world[c] == 255 when allow_unknown is set.
 *   w(c) = neutral_cost + cost_weight * world[c]                              (passable cells only)
 *   a step from cell a into an 8-neighbour b costs 5 * w(b) along an axis and 7 * w(b) along a diagonal;
 *   a diagonal step is allowed only when both cells that share an edge with a and b are passable (no corner cutting).
 *   Neighbour order, wherever an order matters, as (dx, dy): (1,0) (0,1) (-1,0) (0,-1) (1,1) (-1,1) (-1,-1) (1,-1).
 *   Cell of a point, per axis: floor((p - origin) / resolution), every operation an IEEE double operation rounded on its
 *   own; a point that is not finite, or whose cell lies outside the world, has no cell.
 *   Centre of cell i, per axis: origin + (i + 0.5) * resolution (the sum i + 0.5, the product, the sum), derived from the
 *   integer cell every time. */
#define SMPC_FIELD_UNREACHABLE 0xFFFFFFFFu

typedef struct smpc_plan_cost_params {
  int32_t neutral_cost;         /* >= 1; 50 is the customary value */
  int32_t cost_weight;          /* >= 0; customary 1. neutral_cost + 255 * cost_weight <= 65535 */
  uint8_t lethal_min_cost;      /* customary 253 */
  uint8_t allow_unknown;        /* != 0: a cell of exactly 255 is passable as well; customary 0 */
  uint8_t reserved[6];
} smpc_plan_cost_params;

typedef struct smpc_goal_field_in {
  int32_t G;                    /* goals, >= 0 */
  int32_t on_device;            /* 0 host pointers, 1 device pointers (outputs follow) */
  int32_t world_x, world_y;     /* world cells, >= 1 */
  int32_t world_shared;         /* 1: one world map and origin for all goals */
  int32_t reserved;
  double resolution;            /* finite and > 0 */
  smpc_plan_cost_params cost;
  const uint8_t* world;         /* [G or 1][world_y][world_x] */
  const double* world_origin;   /* [G or 1][2] */
  const double* goal;           /* [G][2] */
} smpc_goal_field_in;

/* field[g][c]: the least total step cost of any allowed path from cell c to the cell of goal g; 0 at the goal's cell,
 * SMPC_FIELD_UNREACHABLE for impassable cells and cells without a path. status[g]: 0 ok, 1 the goal has no cell, 2 the
 * goal's cell is impassable (1 and 2: the whole field is unreachable).
 * One workgroup per goal relaxes its field tile by tile until nothing changes; every loop is bounded, and a field that
 * has not settled within world_x * world_y sweeps (a bug) comes back as SMPC_ERR_DEVICE. To find that out the call reads
 * one word back after its kernel, so it WAITS FOR THE STREAM also with device pointers: keep it out of captured graphs.
 * No allocation after a handle's first call.
 * SMPC_ERR_INVALID_ARG (nothing launched, nothing written): a NULL handle, input, field, world, world_origin or goal;
 * G < 0; world_x or world_y < 1; a resolution that is not finite or not > 0; neutral_cost < 1; cost_weight < 0;
 * neutral_cost + 255 * cost_weight > 65535.
 * SMPC_ERR_UNSUPPORTED: world_x * world_y >= 2^31, or world_x * world_y * 7 * (neutral_cost + 255 * cost_weight) >=
 * 2^32 - 1 (computed in 64 bits: no potential can then overflow or collide with the marker). */
int smpc_goal_field_batch(smpc_handle* h, const smpc_goal_field_in* in,
                          uint32_t* field   /* [G][world_y][world_x] */,
                          int32_t* status   /* [G] or NULL */);

enum smpc_plan_error {
  SMPC_PLAN_OK = 0,
  SMPC_PLAN_START_OUTSIDE = 1,       /* the pose has no cell */
  SMPC_PLAN_START_BLOCKED = 2,       /* the start cell is impassable */
  SMPC_PLAN_UNREACHABLE = 3,         /* no path from the start cell */
  SMPC_PLAN_TRUNCATED = 4,           /* more than L poses: the first L are written */
  SMPC_PLAN_BAD_GOAL_INDEX = 5,      /* robot_goal outside 0..G-1 */
  SMPC_PLAN_INCONSISTENT_FIELD = 6   /* no neighbour satisfies the equality, or more than world_x * world_y steps */
};

typedef struct smpc_extract_plan_in {
  int32_t B;                    /* robots, >= 0 */
  int32_t G;                    /* fields, >= 0 */
  int32_t L;                    /* rows of a plan, >= 2 */
  int32_t stride;               /* every stride-th path cell becomes a pose, >= 1 */
  int32_t on_device;
  int32_t world_x, world_y;
  int32_t world_shared;
  double resolution;
  smpc_plan_cost_params cost;
  const uint8_t* world;         /* [G or 1][world_y][world_x] */
  const double* world_origin;   /* [G or 1][2] */
  const uint32_t* field;        /* [G][world_y][world_x] */
  const double* goal;           /* [G][2] */
  const int32_t* robot_goal;    /* [B]: the field of each robot */
  const double* pose;           /* [B][3]; x, y are read */
} smpc_extract_plan_in;

/* Per robot, with g = robot_goal[b], checked in this order: g outside 0..G-1: BAD_GOAL_INDEX; the pose has no cell:
 * START_OUTSIDE; its cell c0 is impassable: START_BLOCKED; field[g][c0] is the marker: UNREACHABLE.
 * Walk: from c = c0, while field[c] != 0, go to the first neighbour n in the order above that is passable, reachable,
 * allowed by the diagonal rule and has field[n] + k * w(n) == field[c] exactly (k = 5 or 7); none, or more than
 * world_x * world_y steps: INCONSISTENT_FIELD. That gives cells c0 .. cn.
 * Plan: pose 0 is the robot's (x, y); then the centres of c[j * stride] for j = 1, 2, .. while j * stride < n; last the
 * goal point goal[g] itself (n = 0: [pose, goal]). More than L poses: the first L are written, plan_len = L, TRUNCATED.
 * Rows of plan beyond plan_len are not written. With any error but TRUNCATED plan_len = 0 and none of the robot's rows is
 * written (the walk is therefore made twice: once to judge it, once to write). A robot's outputs depend on that robot's
 * inputs and its field alone.
 * For device pointers one kernel on the handle's stream, no allocation and no host synchronisation (capturable in a HIP
 * graph). Refusals as for smpc_goal_field_batch (with field, robot_goal, pose, plan and plan_len among the pointers and
 * B < 0 or G < 0), plus L < 2 and stride < 1 (SMPC_ERR_INVALID_ARG). */
int smpc_extract_plan_batch(smpc_handle* h, const smpc_extract_plan_in* in,
                            double* plan        /* [B][L][2] */,
                            int32_t* plan_len   /* [B] */,
                            int32_t* error      /* [B] or NULL: enum smpc_plan_error */);

#ifdef __cplusplus
}
#endif

#endif
