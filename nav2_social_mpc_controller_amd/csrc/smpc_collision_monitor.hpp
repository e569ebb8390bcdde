// smpc_collision_monitor.hpp — the collision monitor (include/smpc_collision_monitor.h; the rule:
// smpc_collision_monitor_rule.hpp): per robot, the cells its beams stopped at become points in its frame, every zone counts the
// points inside it, an APPROACH zone again at every step of a simulation of the command, and the least ratio scales the command.
//   One wavefront per robot, four robots per workgroup, no LDS, no s_barrier. The robot's own scalars (pose, command) are loaded
//   by every lane and taken from lane 0, so they are wave-uniform by construction; the zones and the math table are read from
//   the kernel arguments by scalar loads where they are needed; what only meets the points in vector arithmetic is moved to
//   vector registers (cm_vector), which keeps the kernel clear of scalar spills; lane 0 alone stores the robot's rows.
//   * Points: lane j takes beams j, j + 64, ..: a chunk is eight of them per lane, in registers. With n_beams <= 512 there is
//     one chunk, built once (kResident); beyond that the chunks are rebuilt from beam_kind / beam_cell at every pass.
//   * A count is the sum over the chunk's slots of popcount(ballot(inside)): every lane holds it. The polygon walks its edges
//     outside and the chunk's slots inside, so a vertex is read once per pass; the parities are bits of one register.
//   * Reach: a point beyond cm_reach2 of a zone is outside it at every step, so a zone with fewer than min_points points
//     within reach is not simulated. At every step a polygon walks its edges only for the slots (a lane's k-th points) that
//     hold a point within the disc around the zone. The approach loop ends at the first triggering step, and before a step
//     whose ratio m / M would not undercut the least ratio so far. None of this shows in the result: a point that is
//     dropped is outside, a ratio that does not undercut does not decide.
//   Bounds: the entry point admits 1 <= Z <= 8, n <= 16 vertices, 0 <= M <= 32, 1 <= n_beams <= 4096 only. Global rows are
//   beam k < n_beams of robot b < B, zone_points column z < Z.
// Plain vector loads and stores, no atomics.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "smpc_collision_monitor_rule.hpp"
#include "smpc_math.hpp"

namespace smpc {

constexpr int kCmThreads = 256;  // four wavefronts = four robots
constexpr int kCmSlots = 8;      // points per lane and chunk

struct MonitorParams {
  int B, n_beams, Z, M;
  double sim_dt, res, ox, oy;
  const double* pose;        // [B][3]
  const double* cmd;         // [B][2]
  const uint8_t* kind;       // [B][n_beams]
  const int32_t* cell;       // [B][n_beams][2]
  double* cmd_out;           // [B][2]
  int32_t* action;           // [B][4]
  int32_t* zone_points;      // [B][Z] or null
  double* ratio;             // [B] or null
  double* heading;           // [B][2] or null
  double* step;              // [B][2] or null
  MonitorZone zones[kMonitorMaxZones];
  MathTab mt;
};

// lane 0's value in every lane (v_readfirstlane_b32 twice): the robot's own scalars
__device__ inline double cm_uniform(double v) {
  uint64_t u;
  __builtin_memcpy(&u, &v, sizeof(double));
  const uint64_t r = (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)u) |
                     (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(u >> 32)) << 32;
  double d;
  __builtin_memcpy(&d, &r, sizeof(double));
  return d;
}

// lane l's value in every lane (v_readlane_b32 twice)
__device__ inline double cm_lane(double v, int l) {
  uint64_t u;
  __builtin_memcpy(&u, &v, sizeof(double));
  const uint64_t r = (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)u, l) |
                     (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(u >> 32), l) << 32;
  double d;
  __builtin_memcpy(&d, &r, sizeof(double));
  return d;
}

// The same value in a vector register: what only meets the points in vector arithmetic (the heading, the simulated pose)
// need not occupy scalar registers, which the zones, the ballots and the loop state fill.
__device__ inline double cm_vector(double v) {
  asm("" : "+v"(v));
  return v;
}

__device__ inline unsigned long long cm_vector(unsigned long long v) {
  asm("" : "+v"(v));
  return v;
}

__device__ inline int cm_vector(int v) {
  asm("" : "+v"(v));
  return v;
}

// One chunk of a robot's points: slot j of this lane is beam first + 64 j + lane. A slot whose beam gives no point holds a NaN,
// which no test of the rule finds inside a zone or within reach, at any step: the counts need no mask.
struct MonitorChunk {
  double px[kCmSlots], py[kCmSlots];
  int slots;  // wave-uniform: slots of this chunk that lie below n_beams in some lane
};

// returns the chunk's number of points (wave-wide, in every lane)
__device__ inline int cm_load_chunk(MonitorChunk& ch, const uint8_t* kind, const int32_t* cell, int n_beams, int first, int lane,
                                     int has_cell, int32_t ax, int32_t ay, double ox, double oy, double res, double x, double y, double c,
                                     double s) {
  const int left = n_beams - first;
  ch.slots = left >= 64 * kCmSlots ? kCmSlots : (left + 63) / 64;
  int points = 0;
#pragma unroll
  for (int j = 0; j < kCmSlots; ++j) {
    ch.px[j] = __builtin_nan(""); ch.py[j] = __builtin_nan("");
    if (j < ch.slots) {  // wave-uniform
      const int k = first + 64 * j + lane;
      const bool hit = has_cell != 0 && k < n_beams && cm_is_hit((uint32_t)kind[k]);
      if (hit) {
        const double rx = cm_rel(ox, ax, cell[2 * k], res, x), ry = cm_rel(oy, ay, cell[2 * k + 1], res, y);
        cm_to_frame(c, s, rx, ry, &ch.px[j], &ch.py[j]);
      }
      points += __popcll(__ballot(hit));
    }
  }
  return points;
}

// The points of a chunk inside a zone at one step: the wave-wide count, in every lane. moved: the step's pose (X, Y, C, S)
// applies; else the points themselves. A polygon first asks which slots hold a point within its own disc (near2) at this step
// and walks its edges for those alone. In the `first` pass (step 0) the points within the zone's reach are counted too.
template <class ZoneP>
__device__ inline int cm_count_chunk(const MonitorChunk& ch, ZoneP z, bool moved, double X, double Y, double C, double S, double near2,
                                     double reach2, bool first, int* reach) {
  double qx[kCmSlots], qy[kCmSlots];
#pragma unroll
  for (int j = 0; j < kCmSlots; ++j) {
    qx[j] = ch.px[j]; qy[j] = ch.py[j];
    if (moved && j < ch.slots) cm_step_point(ch.px[j], ch.py[j], X, Y, C, S, &qx[j], &qy[j]);
  }
  int cnt = 0;
  if (z->shape == kMonitorCircle) {
    const double r2 = z->radius2;
#pragma unroll
    for (int j = 0; j < kCmSlots; ++j)
      if (j < ch.slots) cnt += __popcll(__ballot(cm_in_circle(qx[j], qy[j], r2)));
  } else {
    uint32_t act = 0u;  // wave-uniform bits
#pragma unroll
    for (int j = 0; j < kCmSlots; ++j)
      if (j < ch.slots && __ballot(cm_within_reach(qx[j], qy[j], near2)) != 0ull) act |= 1u << j;
    if (act != 0u) {
      uint32_t in = 0u;
      const int n = z->n;
      double vjx = z->vx[n - 1], vjy = z->vy[n - 1];
      for (int i = 0; i < n; ++i) {
        const double vix = z->vx[i], viy = z->vy[i];
#pragma unroll
        for (int j = 0; j < kCmSlots; ++j)
          if ((act >> j) & 1u) in ^= (uint32_t)cm_edge_counts(vix, viy, vjx, vjy, qx[j], qy[j]) << j;
        vjx = vix; vjy = viy;
      }
#pragma unroll
      for (int j = 0; j < kCmSlots; ++j)
        if ((act >> j) & 1u) cnt += __popcll(__ballot((in >> j) & 1u));
    }
  }
  if (first) {
    int r = 0;
#pragma unroll
    for (int j = 0; j < kCmSlots; ++j)
      if (j < ch.slots) r += __popcll(__ballot(cm_within_reach(ch.px[j], ch.py[j], reach2)));
    *reach += r;
  }
  return cnt;
}

template <bool kResident>
__global__ __launch_bounds__(kCmThreads) void smpc_collision_monitor_kernel(const MonitorParams) {
  SMPC_CHAIN_PRIORITY();
  const MonitorParams SMPC_TAB_AS* ka = (const MonitorParams SMPC_TAB_AS*)__builtin_amdgcn_kernarg_segment_ptr();
  const MathTabP mt = &ka->mt;  // everything is read from the kernel arguments where it is needed, not held from the start
  const int lane = (int)(threadIdx.x & 63u);
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const long long b = (long long)blockIdx.x * (kCmThreads / 64) + wave;
  if (b >= ka->B) return;  // wave-uniform
  size_t r = (size_t)b;
  const int Z = ka->Z, M = ka->M, n_beams = ka->n_beams;

  // step 1
  const double x = cm_uniform(ka->pose[3 * r]), y = cm_uniform(ka->pose[3 * r + 1]), th = cm_uniform(ka->pose[3 * r + 2]);
  const double v = cm_uniform(ka->cmd[2 * r]), w = cm_uniform(ka->cmd[2 * r + 1]);
  if (!(cm_finite(x) && cm_finite(y) && cm_finite(th) && cm_finite(v) && cm_finite(w))) {  // wave-uniform
    if (lane == 0) {
      ka->cmd_out[2 * r] = 0.0; ka->cmd_out[2 * r + 1] = 0.0;
      ka->action[4 * r] = kMonitorBadInput; ka->action[4 * r + 1] = -1; ka->action[4 * r + 2] = -1; ka->action[4 * r + 3] = 0;
      if (ka->ratio) ka->ratio[r] = 0.0;
    }
    if (ka->zone_points && lane < Z) ka->zone_points[r * (size_t)Z + (size_t)lane] = 0;
    return;
  }

  // From here on the row index is a value the compiler knows nothing about: it then keeps the index alone over the zone loop,
  // not the byte offsets of every output row it can derive from it.
  {
    unsigned long long opaque = (unsigned long long)r;
    asm volatile("" : "+s"(opaque));
    r = (size_t)opaque;
  }

  // step 2: lane 1 takes the step's angle, every other lane the heading: one sine and cosine for both
  const double angle = (lane == 1 && M > 0) ? cm_step_angle(w, ka->sim_dt) : th;
  double ca, sa;
  cm_heading(mt, angle, &ca, &sa);
  const double c = cm_uniform(ca), s = cm_uniform(sa);
  const double c1 = M > 0 ? cm_lane(ca, 1) : 1.0, s1 = M > 0 ? cm_lane(sa, 1) : 0.0;
  if (lane == 0) {
    if (ka->heading) { ka->heading[2 * r] = c; ka->heading[2 * r + 1] = s; }
    if (ka->step && M > 0) { ka->step[2 * r] = c1; ka->step[2 * r + 1] = s1; }
  }

  // step 3
  const double xv = cm_vector(x), yv = cm_vector(y), cv = cm_vector(c), sv = cm_vector(s), vv = cm_vector(v), wv = cm_vector(w);
  const double c1v = cm_vector(c1), s1v = cm_vector(s1), dtv = cm_vector(ka->sim_dt);
  const double oxv = cm_vector(ka->ox), oyv = cm_vector(ka->oy), resv = cm_vector(ka->res);
  int32_t ax = 0, ay = 0;
  const int has_cell = __builtin_amdgcn_readfirstlane((int)cm_robot_cell(x, y, ka->ox, ka->oy, ka->res, &ax, &ay));  // 0 or 1
  ax = cm_vector(__builtin_amdgcn_readfirstlane(ax)); ay = cm_vector(__builtin_amdgcn_readfirstlane(ay));
  // the robot's rows as per-lane addresses: the streaming kernel holds them over the zone loop, and not in scalar registers
  const uint8_t* kind = (const uint8_t*)cm_vector((unsigned long long)(ka->kind + r * (size_t)n_beams));
  const int32_t* cell = (const int32_t*)cm_vector((unsigned long long)(ka->cell + r * (size_t)n_beams * 2));
  const int per_chunk = 64 * kCmSlots;
  const int chunks = kResident ? 1 : (n_beams + per_chunk - 1) / per_chunk;
  MonitorChunk ch;
  int points = 0;
  if (kResident) points = cm_vector(cm_load_chunk(ch, kind, cell, n_beams, 0, lane, has_cell, ax, ay, oxv, oyv, resv, xv, yv, cv, sv));

  // steps 4 to 6: zone after zone, and for each the passes m = 0 (the points themselves; every zone) and m = 1..M (an
  // APPROACH zone that has not triggered, while a trigger could still decide). Every branch is wave-uniform.
  double best = 1.0;
  int decide = cm_vector(-1), dstep = cm_vector(-1), by = cm_vector(0);  // written under wave-uniform branches, read by lane 0's stores
  for (int zi = 0; zi < Z; ++zi) {
    const MonitorZone SMPC_TAB_AS* z = &ka->zones[zi];
    const int action = z->action, min_points = z->min_points;
    const double reach2 = cm_reach2(z->bound, vv, action == kMonitorApproach ? M : 0, dtv);
    const double near2 = cm_reach2(z->bound, vv, 0, dtv);
    double X = cm_vector(0.0), Y = cm_vector(0.0), C = cm_vector(1.0), S = cm_vector(0.0);
    double ratio = 1.0, f = 0.0;
    int step = -1, reach = 0;
    for (int m = 0;;) {
      int cnt = 0, loaded = 0;
      for (int k = 0; k < chunks; ++k) {
        if (!kResident) loaded += cm_load_chunk(ch, kind, cell, n_beams, k * per_chunk, lane, has_cell, ax, ay, oxv, oyv, resv, xv, yv, cv, sv);
        cnt += cm_count_chunk(ch, z, m > 0, X, Y, C, S, near2, reach2, m == 0, &reach);
      }
      if (m == 0) {
        if (!kResident && zi == 0) points = cm_vector(loaded);
        if (ka->zone_points && lane == 0) ka->zone_points[r * (size_t)Z + (size_t)zi] = cnt;
      }
      if (cnt >= min_points) {
        step = m;
        ratio = action == kMonitorStop ? 0.0
              : action == kMonitorSlowdown ? z->slowdown_ratio
              : action == kMonitorLimit ? cm_uniform(cm_limit_ratio(vv, wv, z->linear_limit, z->angular_limit))
              : f;
        break;
      }
      if (action != kMonitorApproach || reach < min_points || m == M) break;  // no later step can trigger
      ++m;
      f = cm_step_ratio(m, M);
      if (!(f < best)) break;  // this step and the later ones cannot decide
      cm_advance(vv, dtv, c1v, s1v, &X, &Y, &C, &S);
    }
    if (ratio < best) { best = ratio; decide = cm_vector(zi); dstep = cm_vector(step); by = cm_vector(1 << action); }
  }
  const int flags = by | ((has_cell ^ 1) * kMonitorNoCell);

  if (lane == 0) {
    ka->cmd_out[2 * r] = cm_scale(vv, best); ka->cmd_out[2 * r + 1] = cm_scale(wv, best);
    ka->action[4 * r] = flags; ka->action[4 * r + 1] = decide; ka->action[4 * r + 2] = dstep; ka->action[4 * r + 3] = points;
    if (ka->ratio) ka->ratio[r] = best;
  }
}

}  // namespace smpc
