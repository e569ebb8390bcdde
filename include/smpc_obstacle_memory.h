/* smpc_obstacle_memory.h — sensed local costmaps with memory: a mark persists in the robot's rolling window until a later
 * beam passes through its cell, beside include/smpc.h and include/smpc_sensed_costmap.h (whose lists of structs and
 * functions are unchanged, as is SMPC_ABI_VERSION). Same library, same handle, same error codes, same staging of
 * host-pointer calls, smpc_last_kernel_ms() covers the call's kernel.
 * smpc_sensed_costmap_batch rebuilds the window from one scan and forgets it. Nav2's ObstacleLayer, which the reference
 * controller is deployed on (marking and clearing both on, obstacle_max_range 2.5 m, raytrace_max_range 3.0 m,
 * footprint_clearing_enabled), keeps a mark until a ray passes through its cell: a person who steps behind a pillar leaves
 * lethal cells where they were last seen, a hit beyond the marking range stops the ray without marking, and the cells under
 * the robot are always free. This call is the library's own rule for that. The state is one bit per window cell and the
 * world cell of the window's corner, both owned by the caller and read and written by the call. It runs where
 * smpc_sensed_costmap_batch runs: behind smpc_local_costmap_batch, whose `cell` it reads, and before smpc_scene_batch. */
#ifndef SMPC_OBSTACLE_MEMORY_H
#define SMPC_OBSTACLE_MEMORY_H

#include "smpc_sensed_costmap.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct smpc_obstacle_memory_in {
  smpc_sensed_costmap_in scan;   /* every field as smpc_sensed_costmap.h states it; beam_cells reach out to the clearing range */
  int32_t mark_d2;               /* >= 0: a hit is marked only when ox*ox + oy*oy <= mark_d2 (its offset from the robot's cell) */
  int32_t footprint_d2;          /* >= -1: cells within this squared cell distance of the robot's cell are cleared; -1: none */
} smpc_obstacle_memory_in;

/* ---- The rule (csrc/smpc_obstacle_memory_rule.hpp; the kernel: csrc/smpc_obstacle_memory.hpp) -----------------------------
 * "Rule n there" is rule n of smpc_sensed_costmap.h. memory[b] holds one bit per window cell: bit (x & 31) of word (x >> 5)
 * of row y is window cell (x, y); a row is W = (size_x + 31) / 32 words. memory_cell[b] is the world cell of window cell
 * (0, 0) at the time memory[b] was last written.
 * 1. Cells, stoppers, beams, kinds, beam_kind, beam_cell: exactly rules 1 - 3 there. The two beam outputs of this call equal
 *    those of smpc_sensed_costmap_batch on in->scan, always.
 * 2. Roll. Per axis s = memory_cell[b] - cell[b], computed in 64 bits. A set bit at old window cell (x, y) moves to
 *    (x + s.x, y + s.y) when that cell lies in the window and is dropped otherwise; cells that enter the window are unmarked.
 *    Input bits of columns >= size_x in a row's last word are ignored. (Nav2's updateOrigin.)
 * 3. Passed cells. In the walk of rule 3 there, the robot's cell a and every cell (i, j) the walk steps into and tests
 *    without being stopped are passed by that beam. At a lattice corner the two cells that only touch the segment are not
 *    passed. A beam of kind NONE passes its end cell; a hit cell is not passed; INVALID and NO_ROBOT beams pass nothing.
 *    Passed cells inside the window are cleared.
 * 4. Marks. A hit cell (both cells of a corner pair, each judged on its own offset (ox, oy) from a) is marked when it lies
 *    inside the window and ox * ox + oy * oy <= mark_d2. Any other hit leaves its cell's bit as the roll left it.
 *    A cell that stops a beam stops every beam, so it is never passed by any beam, and a passed cell is never a hit: within
 *    one call the cleared set and the marked set are disjoint, and the result depends neither on the order of the beams
 *    nor on that of any atomic. (This is what lets the kernel clear and mark in one pass over the beams.)
 * 5. Footprint. After marks and clears, every window cell whose offset (i, j) from a has i * i + j * j <= footprint_d2 is
 *    cleared, marks of this call included (Nav2 applies footprint_clearing_enabled after marking). Nothing is cleared when
 *    the robot has no cell or footprint_d2 == -1.
 * 6. Outputs. The resulting bitmap is written to memory[b], padding bits zero, and memory_cell[b] = cell[b]. The window is
 *    rule 5 (inflation) and rule 6 (base) there over that bitmap. A robot without a cell casts nothing, but its memory still
 *    rolls and its window is still written.
 * 7. Independence: rule 7 there. memory and memory_cell are read and written in place: a robot's state is read only by the
 *    workgroup that writes it.
 *
 * Two consequences: with memory all zero on entry, mark_d2 >= 2 * 127 * 127 and footprint_d2 == -1 all three outputs equal
 * smpc_sensed_costmap_batch's on in->scan; and an all-zero memory needs no valid memory_cell (any shift of nothing is
 * nothing), so an episode starts from zeroed buffers and there is no reset flag.
 *
 * SMPC_ERR_INVALID_ARG / SMPC_ERR_UNSUPPORTED (nothing launched, nothing written): all those of smpc_sensed_costmap_batch
 * on `scan`; SMPC_ERR_INVALID_ARG for a NULL memory or memory_cell, mark_d2 < 0 or footprint_d2 < -1. B == 0 succeeds and
 * launches nothing. For device pointers one kernel on the handle's stream, no allocation and no host synchronisation
 * (capturable in a HIP graph); host pointers are staged like everywhere, memory and memory_cell both ways. */
int smpc_obstacle_memory_batch(smpc_handle* h, const smpc_obstacle_memory_in* in,
                               uint32_t* memory      /* [B][size_y][(size_x + 31) / 32], in and out */,
                               int32_t* memory_cell  /* [B][2], in and out */,
                               uint8_t* costmap      /* [B][size_y][size_x] */,
                               uint8_t* beam_kind    /* [B][n_beams] enum smpc_beam_kind, or NULL */,
                               int32_t* beam_cell    /* [B][n_beams][2], or NULL */);

#ifdef __cplusplus
}
#endif

#endif
