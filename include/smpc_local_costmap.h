/* smpc_local_costmap.h — rolling local costmaps of a closed-loop episode, beside include/smpc.h (whose list of structs
 * and functions is unchanged, as is SMPC_ABI_VERSION). Same library, same handle, same error codes, same staging of
 * host-pointer calls. */
#ifndef SMPC_LOCAL_COSTMAP_H
#define SMPC_LOCAL_COSTMAP_H

#include "smpc.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- Rolling local costmaps (csrc/smpc_local_costmap.hpp, the cell rule: csrc/smpc_local_costmap_rule.hpp) ------------
 * The reference controller runs on Nav2's rolling local costmap: a window of the world that follows the robot. One call
 * moves every robot's window to its pose and cuts the windows that moved out of the world map, into the buffers
 * smpc_scene_batch reads (costmap [B][size_y][size_x] with costmap_origin [B][2], costmap_shared = 0). */
typedef struct smpc_local_costmap_in {
  int32_t B;
  int32_t on_device;            /* 0 host pointers, 1 device pointers (outputs follow) */
  int32_t size_x, size_y;       /* window cells = smpc_scene_batch.size_x / size_y, >= 1 */
  int32_t world_x, world_y;     /* world cells, >= 1, world_x * world_y < 2^31 */
  int32_t world_shared;         /* 1: one world map and origin for all robots */
  uint8_t outside_cost;         /* value of window cells that lie outside the world */
  uint8_t force;                /* != 0: stored cells are taken as (0,0) and every window is rewritten */
  uint8_t reserved[2];
  double resolution;            /* of the world and of the windows, finite and > 0 */
  const uint8_t* world;         /* [B or 1][world_y][world_x] */
  const double* world_origin;   /* [B or 1][2], finite */
  const double* pose;           /* [B][3]; x, y are read */
} smpc_local_costmap_in;

/* Contract, per robot b and per axis (x shown; w0 = the world origin, res = resolution), every operation an IEEE double
 * operation rounded on its own (no fused multiply-add):
 *   o    = w0 + cell * res                                  (the product, then the sum; cell is (0,0) under `force`)
 *   want = pose_x - ((size_x - 1 + 0.5) * res) / 2          (LayeredCostmap::updateMap with Costmap2D::getSizeInMetersX)
 *   d    = trunc((want - o) / res)                          (Costmap2D::updateOrigin: a cast to int)
 *   cell' = clamp(cell + d, -2^30, 2^30), the sum and the clamp in double, then the conversion.
 * A robot whose pose x or y is not finite keeps its cell (both axes) and gets moved[b] = 2.
 *   costmap_origin[b] = w0 + cell' * res (the same two roundings: derived from the integer cell every time, never
 *     accumulated, so it cannot drift);
 *   costmap[b][y][x]  = world[cell'_y + y][cell'_x + x] where that world cell exists, else outside_cost (partial overlap,
 *     no overlap and a window larger than the world are all legal).
 * A robot is WRITTEN (cell, window and origin) when `force` is set or cell' != cell, with moved[b] = 1 for a finite pose;
 * otherwise moved[b] = 0 (or 2) and neither its window nor its origin is touched, bit for bit. Under `force` a robot
 * without a finite pose is written too, at cell (0,0), and keeps moved[b] = 2. The decision is per robot: a robot's
 * outputs depend on that robot's inputs alone, not on B, its place in the batch, the memory space or timing.
 * For device pointers the call is one kernel on the handle's stream, no allocation and no host synchronisation
 * (capturable in a HIP graph); host pointers are staged like everywhere (costmap and costmap_origin both ways, so what
 * the kernel leaves alone comes back as it went). smpc_last_kernel_ms() covers the kernel.
 * SMPC_ERR_INVALID_ARG (nothing launched, nothing written): a NULL handle, input, cell, costmap, costmap_origin, world,
 * world_origin or pose; B < 0; size_x, size_y, world_x or world_y < 1; a resolution that is not finite or not > 0.
 * SMPC_ERR_UNSUPPORTED: world_x * world_y >= 2^31, size_x * size_y >= 2^31, or size_x or size_y >= 2^30. */
int smpc_local_costmap_batch(smpc_handle* h, const smpc_local_costmap_in* in,
                             int32_t* cell           /* [B][2] in-out: world cell (x, y) of window cell (0,0) */,
                             uint8_t* costmap        /* [B][size_y][size_x] */,
                             double* costmap_origin  /* [B][2] */,
                             int32_t* moved          /* [B] or NULL */);

#ifdef __cplusplus
}
#endif

#endif
