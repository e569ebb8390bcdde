/* smpc_plant.h — the robot plant: a per-robot model between the selected command and the pose, beside include/smpc.h (whose
 * list of structs and functions is unchanged, as is SMPC_ABI_VERSION). Same library, same handle, same error codes, same
 * staging of host-pointer calls, smpc_last_kernel_ms() covers the call's kernel.
 * This is the library's own rule: the reference controller has no counterpart (it hands its command to the deployment's
 * base controller). A closed-loop simulation that places the robot on the pose it planned has an actuator that follows any
 * command at once and a body that passes through what it hits. This call executes a command instead: delayed by a whole
 * number of periods, clamped to the velocity bounds, limited in how fast it may change, and integrated over the period in
 * substeps that stop where the disc of the robot would come closer to a wall cell or to an agent it already touches.
 * The state belongs to the caller, as the tracker's does: all zero is a valid start (a robot at rest at the origin with an
 * empty command queue), so there is no reset flag. */
#ifndef SMPC_PLANT_H
#define SMPC_PLANT_H

#include "smpc.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SMPC_PLANT_MAX_SUBSTEPS 16
#define SMPC_PLANT_MAX_LATENCY 8        /* also the row stride of cmd_queue, whatever L */
#define SMPC_PLANT_MAX_FOOTPRINT_D2 225 /* 15 cells: at most 31 x 31 = 961 offsets */

/* contact[b][0] */
enum smpc_plant_flag {
  SMPC_PLANT_BLOCKED_BY_WALL = 1,   /* substep K + 1 was blocked by a wall */
  SMPC_PLANT_BLOCKED_BY_AGENT = 2,  /* substep K + 1 was blocked by an agent (both may be set) */
  SMPC_PLANT_WALL_CONTACT = 4,      /* a wall cell within the footprint where the period started */
  SMPC_PLANT_AGENT_CONTACT = 8,     /* an agent within contact_dist where the period started */
  SMPC_PLANT_BAD_COMMAND = 16,      /* the target command was not finite and was executed as (0, 0) */
  SMPC_PLANT_BAD_STATE = 32         /* pose or twist not finite: nothing moved */
};

typedef struct smpc_plant_in {
  int32_t B;
  int32_t Np;               /* row stride of agents, 1..SMPC_MAX_AGENTS */
  int32_t S;                /* substeps of the period, 1..SMPC_PLANT_MAX_SUBSTEPS */
  int32_t L;                /* latency in periods, 0..SMPC_PLANT_MAX_LATENCY */
  int32_t on_device;
  int32_t Hx, Hy;           /* the world's cells; >= 1 when world is given */
  int32_t footprint_d2;     /* squared footprint radius in cells, -1..SMPC_PLANT_MAX_FOOTPRINT_D2; -1: no walls */
  int32_t wall_min_cost;    /* a cost >= this is a wall ... */
  int32_t unknown_is_wall;  /* ... 255 only when this is set */
  int32_t outside_is_wall;  /* cells beyond the world are walls */
  int32_t reserved;
  double dt;                /* finite, >= 0 */
  double v_min, v_max;      /* finite, v_min <= v_max */
  double w_max;             /* finite, >= 0 */
  double dv_up, dv_down, dw;  /* largest change per period of v away from zero, of v towards zero, of w (acceleration * dt,
                                 formed by the caller); >= 0, +inf allowed */
  double contact_dist;      /* finite, >= 0: centre distance below which an agent is in contact */
  double resolution;        /* finite, > 0 */
  double world_origin[2];
  const uint8_t* world;     /* [Hy][Hx], one map for all robots; NULL: no walls */
  const double*  cmd;       /* [B][2] v, w: the tick's command */
  const double*  agents;    /* [B][Np][5] smpc_people_batch.people rows; ONLY x and y are read */
  const int32_t* count;     /* [B], clamped to 0..Np */
} smpc_plant_in;

/* ---- The rule (csrc/smpc_plant_rule.hpp; the kernel: csrc/smpc_plant.hpp) --------------------------------------------------
 * Per robot b, in this order; every floating-point operation is rounded on its own (no fused multiply-add) except inside the
 * heading's sine and cosine. clamp(a, lo, hi) is lo when a < lo, else hi when a > hi, else a.
 * 1. Latency. With L > 0 let i = plant_tick[b] mod L (unsigned): the target command is cmd_queue[b][i] and that slot then
 *    takes cmd[b]. With L == 0 the target is cmd[b] and the queue is neither read nor written. plant_tick[b] becomes its
 *    value plus 1 in unsigned 32-bit arithmetic, whatever else happens. A zeroed queue executes (0, 0) for the first L ticks.
 * 2. Finite. If x, y, theta, v or w of the state is not finite: pose is left bit for bit, twist = (+0.0, +0.0),
 *    contact[b] = (32, 0), heading_cs[b] is not written, and the call is over for this robot (step 1 has happened). A target
 *    command with a non-finite component is replaced by (0, 0) and sets flag 16.
 * 3. Limits. vt = clamp(target v, v_min, v_max), wt = clamp(target w, -w_max, w_max); delta = vt - v; the linear limit lim is
 *    dv_up when (v >= 0 and delta >= 0) or (v <= 0 and delta <= 0), else dv_down; v1 = v + clamp(delta, -lim, lim).
 *    w1 = w + clamp(wt - w, -dw, dw).
 * 4. Heading. (c, s) = cosine and sine of theta as the rest of the tick chain obtains them (sincos_tab of csrc/smpc_math.hpp
 *    for |theta| <= 1e5, the library's sincos beyond); written to heading_cs[b] = (c, s) when it is given. Everything below
 *    is a pure function of c and s.
 * 5. Segment. Lx = (v1 * c) * dt, Ly = (v1 * s) * dt; q_0 = (x, y) and q_k = (x + Lx * (k / S), y + Ly * (k / S)) for
 *    k = 1..S, k / S being the quotient of the two as doubles. The heading is held over the period.
 * 6. Clearances at a position q.
 *    wall2(q): the cell of q is (floor((qx - ox) / res), floor((qy - oy) / res)). wall2(q) is the least jx^2 + jy^2 over the
 *    integer offsets (jx, jy) with jx^2 + jy^2 <= footprint_d2 whose cell (cell x + jx, cell y + jy) is a wall: inside the
 *    world a cost >= wall_min_cost that is not 255, or 255 with unknown_is_wall; outside it exactly when outside_is_wall is
 *    set. It is NONE (above every other value) when there is no such cell, when walls are off (world NULL or
 *    footprint_d2 < 0), or when a cell coordinate of q is not finite or beyond 2^30 in magnitude.
 *    agent2(q): the least d2 = ax * ax + ay * ay, ax = px - qx, ay = py - qy, over the rows j < clamp(count[b], 0, Np) with
 *    finite px, py and d2 < contact_dist * contact_dist, ordered by the bits of d2 (a double >= +0 orders as its integer);
 *    NONE when there is no such row. The agents stand where the period started.
 * 7. Advance. Substep k is blocked when wall2(q_k) < wall2(q_(k-1)) or agent2(q_k) < agent2(q_(k-1)): a contact stops the
 *    motion that approaches it, and only that; a robot may slide along a wall at constant clearance and may leave a contact
 *    it starts in. K is the largest k in 0..S with no blocked substep in 1..k. The new pose is (q_K, theta + w1 * dt), the
 *    new twist (v1 if K == S else +0.0, w1): the disc may always turn.
 * 8. Flags. 1: substep K + 1 was blocked by a wall; 2: ... by an agent (both may be set); 4: wall2(q_0) != NONE;
 *    8: agent2(q_0) != NONE; 16 and 32 as in step 2. contact[b] = (flags, K).
 * 9. Independence. A robot's state and outputs depend on that robot's inputs and state alone: not on B, its place in the
 *    batch, the stream or timing. A robot's state is read only by the wavefront that writes it.
 *
 * SMPC_ERR_INVALID_ARG (nothing launched, every buffer left alone, the state included): a NULL handle, input, pose, twist,
 * plant_tick, contact, cmd, agents or count; a NULL cmd_queue with L > 0; B < 0, Np < 1, S < 1, L < 0, footprint_d2 < -1;
 * a dt, v_min, v_max, w_max, contact_dist or resolution that is not finite; dt < 0, w_max < 0, contact_dist < 0,
 * resolution <= 0; v_min > v_max; a negative or NaN dv_up, dv_down or dw; Hx or Hy < 1 with world given
 * (a world_origin that is not finite gives cells that are not finite: no walls). SMPC_ERR_UNSUPPORTED: Np above SMPC_MAX_AGENTS, S,
 * L or footprint_d2 above the maxima above. B == 0 succeeds and writes nothing. For device pointers one kernel on the
 * handle's stream, no allocation and no host synchronisation (capturable in a HIP graph); host pointers are staged like
 * everywhere, the state both ways. */
int smpc_robot_plant_batch(smpc_handle* h, const smpc_plant_in* in,
                           double*   pose        /* [B][3] x, y, theta — state, read and written in place */,
                           double*   twist       /* [B][2] v, w — state, in place */,
                           double*   cmd_queue   /* [B][8][2] — state, in place; may be NULL when L == 0 */,
                           uint32_t* plant_tick  /* [B] — state, in place */,
                           int32_t*  contact     /* [B][2] flags, K — out */,
                           double*   heading_cs  /* [B][2] c, s — out; or NULL */);

#ifdef __cplusplus
}
#endif

#endif
