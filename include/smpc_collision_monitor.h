/* smpc_collision_monitor.h — the collision monitor: a per-robot safety layer between the selected command and the base,
 * beside include/smpc.h (whose list of structs and functions is unchanged, as is SMPC_ABI_VERSION). Same library, same handle,
 * same error codes, same staging of host-pointer calls, smpc_last_kernel_ms() covers the call's kernel.
 * This is the library's own rule for what Nav2's collision_monitor does in the chain controller -> velocity_smoother ->
 * collision_monitor -> base: the reference controller has no counterpart (it hands its command on). The monitor looks at the
 * raw scan, not at the costmap or the tracks: the points are the cells the tick's beams stopped at (beam_kind / beam_cell as
 * smpc_sensed_costmap_batch and smpc_obstacle_memory_batch write them), seen from the robot. Zones around the robot, shared by
 * all robots and given in the robot's frame with x forward, stop the command, scale it, limit it, or scale it by the time a
 * simulation of the command takes to bring the zone onto enough points. The call has no state. */
#ifndef SMPC_COLLISION_MONITOR_H
#define SMPC_COLLISION_MONITOR_H

#include "smpc.h"
#include "smpc_sensed_costmap.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SMPC_MONITOR_MAX_ZONES 8
#define SMPC_MONITOR_MAX_VERTICES 16
#define SMPC_MONITOR_MAX_STEPS 32

enum smpc_monitor_shape { SMPC_MONITOR_CIRCLE = 0, SMPC_MONITOR_POLYGON = 1 };

enum smpc_monitor_action { SMPC_MONITOR_STOP = 0, SMPC_MONITOR_SLOWDOWN = 1, SMPC_MONITOR_LIMIT = 2, SMPC_MONITOR_APPROACH = 3 };

/* action[b][0] */
enum smpc_monitor_flag {
  SMPC_MONITOR_BY_STOP = 1,       /* the deciding zone is a STOP zone: 1 << its action, as the next three */
  SMPC_MONITOR_BY_SLOWDOWN = 2,
  SMPC_MONITOR_BY_LIMIT = 4,
  SMPC_MONITOR_BY_APPROACH = 8,
  SMPC_MONITOR_BAD_INPUT = 16,    /* pose or command not finite: the command out is (0, 0) */
  SMPC_MONITOR_NO_CELL = 32       /* the robot has no cell: it has no points, no zone triggers */
};

typedef struct smpc_monitor_zone {
  int32_t shape;            /* enum smpc_monitor_shape */
  int32_t action;           /* enum smpc_monitor_action */
  int32_t n_vertices;       /* polygon: 3..SMPC_MONITOR_MAX_VERTICES; circle: not read */
  int32_t min_points;       /* >= 1: the zone triggers with at least this many points inside */
  double radius;            /* circle: finite, >= 0; polygon: not read beyond that check */
  double slowdown_ratio;    /* in [0, 1]; read by SLOWDOWN */
  double linear_limit;      /* >= 0, +inf allowed; read by LIMIT */
  double angular_limit;     /* >= 0, +inf allowed; read by LIMIT */
  double vertices[SMPC_MONITOR_MAX_VERTICES][2];  /* polygon: the first n_vertices rows (x, y), finite, either orientation */
} smpc_monitor_zone;

typedef struct smpc_collision_monitor_in {
  int32_t B;
  int32_t n_beams;          /* 1..SMPC_SENSED_MAX_BEAMS */
  int32_t Z;                /* zones, 1..SMPC_MONITOR_MAX_ZONES */
  int32_t M;                /* simulation steps of the APPROACH zones, 0..SMPC_MONITOR_MAX_STEPS; >= 1 with an APPROACH zone */
  int32_t on_device;
  int32_t reserved;
  double sim_dt;            /* finite, > 0 when M > 0; not read when M == 0 */
  double resolution;        /* finite, > 0 */
  double world_origin[2];
  const smpc_monitor_zone* zones; /* [Z] ALWAYS host memory, whatever on_device: read during the call, like this struct */
  const double*  robot_pose;      /* [B][3] x, y, theta */
  const double*  cmd;             /* [B][2] v, w: the command to judge */
  const uint8_t* beam_kind;       /* [B][n_beams] enum smpc_beam_kind */
  const int32_t* beam_cell;       /* [B][n_beams][2] offsets from the robot's cell */
} smpc_collision_monitor_in;

/* ---- The rule (csrc/smpc_collision_monitor_rule.hpp; the kernel: csrc/smpc_collision_monitor.hpp) ---------------------------
 * Per robot b, with (x, y, theta) = robot_pose[b] and (v, w) = cmd[b]; every floating-point operation is rounded on its own
 * (no fused multiply-add) except inside sine and cosine.
 * 1. Finite. If x, y, theta, v or w is not finite: cmd_out[b] = (+0.0, +0.0), action[b] = (BAD_INPUT, -1, -1, 0),
 *    zone_points[b][.] = 0, ratio[b] = +0.0, heading_cs[b] and step_cs[b] are not written, and the call is over for this robot.
 * 2. Heading. (c, s) = cosine and sine of theta exactly as smpc_plant.h rule 4 obtains them (sincos_tab of csrc/smpc_math.hpp
 *    for |theta| <= 1e5, the library's sincos beyond), written to heading_cs[b]. With M > 0, (c1, s1) = cosine and sine of the
 *    product w * sim_dt, obtained the same way and written to step_cs[b]; with M == 0 step_cs is not written. Everything
 *    below is a pure function of these four numbers.
 * 3. Points. The robot's cell a is that of smpc_sensed_costmap.h rule 1 (per axis floor((p - origin) / resolution), finite x
 *    and y, |q| <= 2^30); a robot without a cell has no points and flag NO_CELL. Beam k gives one point when beam_kind[b][k] is
 *    WORLD, AGENT or CORNER_PAIR (a pair counts once, as its recorded cell), every other value gives none. The point is the
 *    centre of cell a + beam_cell[b][k] (the sum as exact integers), per axis origin + (i + 0.5) * resolution as in
 *    smpc_global_plan.h (the sum i + 0.5, the product, the sum). In the robot's frame: r = centre - (x, y),
 *    p = (c * rx + s * ry, c * ry - s * rx). Duplicated cells are duplicated points.
 * 4. Inside, for a point q. Circle: qx * qx + qy * qy < radius * radius. Polygon: the parity of the edges i = 0..n-1, with
 *    j = (i + n - 1) mod n, for which (Vi.y > q.y) != (Vj.y > q.y) and, with dy = Vj.y - Vi.y and
 *    t = (Vj.x - Vi.x) * (q.y - Vi.y) - (q.x - Vi.x) * dy: t > 0 when dy > 0, t < 0 when dy < 0. No division.
 *    A zone triggers at a step when at least min_points of the step's points are inside.
 * 5. Approach. (X, Y) = (+0, +0), (C, S) = (1, 0). For m = 1..M: X += (v * C) * sim_dt, Y += (v * S) * sim_dt, then
 *    (C, S) <- (C * c1 - S * s1, S * c1 + C * s1); the points of step m are d = p - (X, Y), q = (C * dx + S * dy,
 *    C * dy - S * dx). Step 0 uses the points p themselves. The collision step of a zone is the first m in 0..M at which it
 *    triggers, or -1. An APPROACH zone with a collision step m yields the ratio m / M (the quotient of the two as doubles).
 * 6. Ratios. STOP: 0 when triggered at step 0. SLOWDOWN: slowdown_ratio when triggered at step 0. LIMIT, when triggered at
 *    step 0: the least of 1, linear_limit / |v| (only when |v| > linear_limit) and angular_limit / |w| (only when
 *    |w| > angular_limit). A zone that is not triggered yields 1. ratio[b] is the least over the zones; the deciding zone is
 *    the lowest index that attains it when it is < 1, else -1. cmd_out[b] is cmd[b] bit for bit (a -0.0 included) when the
 *    ratio is 1, (+0.0, +0.0) when it is 0, else (v * ratio, w * ratio). All zones judge the incoming command.
 *    action[b] = (flags, deciding zone or -1, collision step of the deciding zone or -1, number of points): the flags are
 *    1 << action of the deciding zone, and NO_CELL. zone_points[b][z] is the number of points inside zone z at step 0,
 *    the full count, whatever min_points.
 * 7. Independence. A robot's outputs depend on that robot's inputs alone: not on B, its place in the batch, the memory space,
 *    the stream or timing.
 *
 * SMPC_ERR_INVALID_ARG (nothing launched, every buffer left alone): a NULL handle, input, cmd_out, action, zones, robot_pose,
 * cmd, beam_kind or beam_cell; cmd_out == cmd; B < 0, Z < 1, n_beams < 1, M < 0; M == 0 with an APPROACH zone; a resolution
 * that is not finite or not > 0, with M > 0 a sim_dt likewise; a zone with an unknown shape or action, a polygon's n_vertices
 * outside 3..16, min_points < 1, a radius, linear_limit or angular_limit that is negative or NaN, a slowdown_ratio outside
 * [0, 1], a radius or one of a polygon's n_vertices vertices that is not finite. SMPC_ERR_UNSUPPORTED: Z, M or n_beams above
 * the maxima. B == 0 succeeds and writes nothing. For device pointers one kernel on the handle's stream, no allocation and no
 * host synchronisation (capturable in a HIP graph: the zones travel with the launch); host pointers are staged like everywhere. */
int smpc_collision_monitor_batch(smpc_handle* h, const smpc_collision_monitor_in* in,
                                 double*  cmd_out      /* [B][2] v, w — out; not the buffer of in->cmd */,
                                 int32_t* action       /* [B][4] flags, deciding zone, its collision step, points — out */,
                                 int32_t* zone_points  /* [B][Z] — out; or NULL */,
                                 double*  ratio        /* [B] — out; or NULL */,
                                 double*  heading_cs   /* [B][2] c, s — out; or NULL */,
                                 double*  step_cs      /* [B][2] c1, s1 — out with M > 0; or NULL */);

#ifdef __cplusplus
}
#endif

#endif
