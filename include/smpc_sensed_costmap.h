/* smpc_sensed_costmap.h — sensed local costmaps: each robot's window as one laser scan marks it, inflated, beside
 * include/smpc.h (whose list of structs and functions is unchanged, as is SMPC_ABI_VERSION). Same library, same handle,
 * same error codes, same staging of host-pointer calls, smpc_last_kernel_ms() covers the call's kernel.
 * The reference controller is deployed on a rolling local costmap of two layers, an ObstacleLayer fed by one laser scan and
 * an InflationLayer, with no static layer: its costmap holds what the scanner hits, walls and legs alike, inflated. This
 * call is the library's own rule for that: a MEMORYLESS scan, rebuilt every tick from the world map and the agents it is
 * handed. Nav2's persistent marking and its ray-trace clearing over several scans are smpc_obstacle_memory_batch
 * (include/smpc_obstacle_memory.h), which adds a state to this rule. It runs behind
 * smpc_local_costmap_batch, whose `cell` it reads, and writes the windows smpc_scene_batch reads. */
#ifndef SMPC_SENSED_COSTMAP_H
#define SMPC_SENSED_COSTMAP_H

#include "smpc.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SMPC_SENSED_MAX_REACH 127    /* largest |dx|, |dy| of a beam's end offset, in cells */
#define SMPC_SENSED_MAX_SIZE 256     /* largest window side */
#define SMPC_SENSED_MAX_D2 1024      /* largest d2_max (an inflation radius of 32 cells) */
#define SMPC_SENSED_MAX_BEAMS 4096

/* beam_kind[b][k] */
enum smpc_beam_kind {
  SMPC_BEAM_NONE = 0,          /* nothing stops the beam up to and including its end cell */
  SMPC_BEAM_WORLD = 1,         /* the hit is an occluding cell of the world map */
  SMPC_BEAM_AGENT = 2,         /* the hit is a cell an agent occupies (and no occluding world cell) */
  SMPC_BEAM_CORNER_PAIR = 3,   /* the beam ends on a lattice corner between two cells that both stop it: two hits */
  SMPC_BEAM_INVALID = 4,       /* |dx| or |dy| of the end offset exceeds SMPC_SENSED_MAX_REACH: nothing is cast */
  SMPC_BEAM_NO_ROBOT = 5       /* the robot has no cell: nothing is cast */
};

typedef struct smpc_sensed_costmap_in {
  int32_t B, Np;                /* Np: row stride of people, >= 1 */
  int32_t on_device;
  int32_t size_x, size_y;       /* window cells, 1 .. SMPC_SENSED_MAX_SIZE */
  int32_t world_x, world_y;     /* >= 1, world_x * world_y < 2^31 */
  int32_t world_shared;         /* 1: one world map and origin for all robots */
  int32_t n_beams;              /* 1 .. SMPC_SENSED_MAX_BEAMS */
  int32_t agent_d2;             /* >= 0: an agent occupies the cells within this squared cell distance of its own */
  int32_t d2_max;               /* 0 .. SMPC_SENSED_MAX_D2: the last entry of inflation_cost */
  uint8_t occlusion_min_cost;   /* a world cell with cost >= this stops a beam (default 254) */
  uint8_t unknown_occludes;     /* 0: cost 255 never stops a beam */
  uint8_t base;                 /* 0: the window starts free; 1: from the world map, as smpc_local_costmap_batch cuts it */
  uint8_t outside_cost;         /* base 1: value of window cells that lie outside the world */
  double resolution;            /* finite, > 0 */
  const uint8_t* world;         /* [B or 1][world_y][world_x] */
  const double* world_origin;   /* [B or 1][2] */
  const double* robot_pose;     /* [B][3]; x, y are read */
  const double* people;         /* [B][Np][5] as smpc_people_batch.people; x, y are read */
  const int32_t* count;         /* [B], clamped to 0..Np as people_to_status does */
  const int32_t* cell;          /* [B][2] world cell (x, y) of window cell (0,0): smpc_local_costmap_batch's, read only */
  const int32_t* beam_cells;    /* [n_beams][2] end-cell offsets (dx, dy) from the robot's cell, shared by all robots */
  const uint8_t* inflation_cost;/* [d2_max + 1] cost by squared cell distance to the nearest mark */
} smpc_sensed_costmap_in;

/* ---- The rule (csrc/smpc_sensed_costmap_rule.hpp; the kernel: csrc/smpc_sensed_costmap.hpp) -----------------------------
 * Everything about a ray is exact integer arithmetic; the only doubles are the cell of a point,
 * q = floor((p - origin) / resolution) per axis as in smpc_visibility.h rule 1 (every operation rounded on its own).
 * 1. Cells. The robot's cell a is that of (x, y) of robot_pose[b]; a robot whose x or y is not finite, or for which
 *    |q| <= 2^30 fails on an axis, has no cell: it casts nothing and every beam of it has kind NO_ROBOT. Agent
 *    j < clamp(count[b], 0, Np) with finite x and y and |q| <= 2^30 on both axes has the cell q and occupies the cells
 *    q + (i, j) with i * i + j * j <= agent_d2; every other row occupies nothing.
 * 2. What stops a beam. A world cell that lies inside the world and has cost >= occlusion_min_cost && (cost != 255 ||
 *    unknown_occludes): kind WORLD. A cell an agent occupies, inside the world or not: kind AGENT; WORLD wins when both
 *    hold. Cells outside the world are transparent unless occupied. a itself never stops a beam.
 * 3. One beam k runs from the centre of a to the centre of e = a + beam_cells[k], along the walk of smpc_visibility.h
 *    rule 3: dx = |ex - ax|, dy = |ey - ay|, unit steps sx, sy, i = j = 0; until (i, j) == (dx, dy) compare
 *    A = (2i + 1) * dy with Bv = (2j + 1) * dx: A < Bv step i, A > Bv step j; equal (a lattice corner): the cells
 *    (i + 1, j) and (i, j + 1), which touch the segment only there, are tested as a pair: when BOTH stop the beam it ends
 *    there with kind CORNER_PAIR and both are hits (one alone does not stop it), else step both. After each step the new
 *    cell is tested, e included; the first cell that stops the beam is the hit, with its kind. No hit: NONE. A beam with
 *    |dx| or |dy| > SMPC_SENSED_MAX_REACH has kind INVALID and casts nothing (the kernel checks this itself: the table is
 *    device memory). beam_cell[b][k] is the hit's offset from a: for a pair the cell that stepped along x, (i + 1, j); for
 *    NONE, INVALID and NO_ROBOT the end offset beam_cells[k].
 * 4. Marks. A hit cell that lies inside the robot's window (window cell = world cell - cell[b], 0 <= . < size) is marked;
 *    hits outside the window are dropped.
 * 5. Inflation. For every window cell, d2 is the least dx * dx + dy * dy (integers) to a marked cell of the same window;
 *    its cost is inflation_cost[d2] when d2 <= d2_max, else (and without any mark) 0. The table need not be monotone.
 * 6. Base. base 0: that cost is the cell. base 1: the cell is the larger of that cost and what smpc_local_costmap_batch
 *    puts there: world[cell[b].y + y][cell[b].x + x] where that world cell exists, else outside_cost.
 * 7. Every window, and every beam_kind / beam_cell entry when the arrays are given, is written every call. A robot's
 *    outputs depend on that robot's inputs alone: not on B, its place in the batch, the memory space, timing or the order
 *    of any atomic.
 *
 * SMPC_ERR_INVALID_ARG (nothing launched, nothing written): a NULL handle, input, costmap, world, world_origin,
 * robot_pose, people, count, cell, beam_cells or inflation_cost; B < 0; Np < 1; size_x, size_y, world_x or world_y < 1; a
 * resolution that is not finite or not > 0; n_beams < 1; agent_d2 < 0; d2_max < 0; base > 1.
 * SMPC_ERR_UNSUPPORTED: size_x or size_y > SMPC_SENSED_MAX_SIZE, d2_max > SMPC_SENSED_MAX_D2,
 * n_beams > SMPC_SENSED_MAX_BEAMS, world_x * world_y >= 2^31. B == 0 succeeds and launches nothing.
 * For device pointers one kernel on the handle's stream, no allocation and no host synchronisation (capturable in a HIP
 * graph); host pointers are staged like everywhere. */
int smpc_sensed_costmap_batch(smpc_handle* h, const smpc_sensed_costmap_in* in,
                              uint8_t* costmap    /* [B][size_y][size_x] */,
                              uint8_t* beam_kind  /* [B][n_beams] enum smpc_beam_kind, or NULL */,
                              int32_t* beam_cell  /* [B][n_beams][2], or NULL */);

#ifdef __cplusplus
}
#endif

#endif
