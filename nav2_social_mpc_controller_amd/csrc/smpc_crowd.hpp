// smpc_crowd.hpp — one control period of the closed loop's crowd (smpc_crowd_step_batch): every robot's persons move under
// the Social Force Model of include/nav2_social_mpc_controller/sfm.hpp (computeForces :462-485 = desired + obstacle +
// social force, updatePosition :525-572 with its goal queue as a cursor into a waypoint list). Persons go across lanes as
// in smpc_metrics.hpp: a robot owns G = next power of two >= Np lanes, 64 / G robots share a wavefront. The robot is a
// partner of every person (loaded by every lane of the group), not a lane, so Np = 64 fits one wave.
// Person-to-person terms: the force on i from j is the exact negative of the force on j from i (see smpc_project.hpp), so
// every unordered pair is evaluated once with proj_pair_* (smpc_sfm.hpp) and the negated term is handed over by shuffle:
// half the instructions of the ordered double loop. In round k lane i takes partner (i + k) mod n; two rounds per trip keep
// two independent chains in flight (the kernel does one step per launch and is bound by the latency of that chain). The
// one exception to the antisymmetry is a pair closer than 1e-6 m, where BOTH persons take diff = (1e-6, 0): the reverse
// term of such a pair is evaluated on its own in a branch the wave takes once per trip, like the two-arctangent form of
// theta next to 0 and pi. The order of a person's sum is: robot, then per round its own term and the received one, a
// function of count[b] and robot_visible alone. No LDS, no atomics, no private segment; the grid entry of a person's cell
// is requested before the pair loop and consumed after it.
// Groups (smpc_crowd_step_groups_batch, computeGroupForce :325-393): the same body with kGroups = true adds one pass over
// the robot's grouped lanes after the pair rounds, in ascending lane order: three shuffles per grouped person (px, py, id)
// give every member the position sum, the size and the repulsion sum of its group; no transcendental in the pass, one
// exponential per member afterwards. A robot without a grouped person makes no trip. The plain kernel is the
// instantiation with kGroups = false and compiles to the code it had before the template existed.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/smpc.h"
#include "smpc_math.hpp"
#include "smpc_sfm.hpp"

namespace smpc {

constexpr int kCrowdThreads = 256;

struct CrowdParams {
  int B, Np, K, lgG;  // G = 1 << lgG lanes of one robot (power of two, Np <= G <= 64)
  int cyclic, robot_visible;
  int od_shared, od_width, od_height;
  float od_resolution;
  double dt, goal_radius, person_radius, desired_speed;
  const double* pose;            // [B][3]
  const double* twist;           // [B][2]
  const int32_t* count;          // [B]
  const double* waypoints;       // [B][Np][K][2]
  const int32_t* n_waypoints;    // [B][Np]
  const double* desired_speeds;  // [B][Np] or null
  const uint32_t* od_indexes;    // [B or 1][od_height][od_width] or null
  const double* od_origin;       // [B or 1][2]
  double* people;                // [B][Np][5]
  int32_t* cursor;               // [B][Np]
  MathTab mt;
};

// one partner's term with the coincident-pair convention: a pair closer than 1e-6 m takes diff = (1e-6, 0)
__device__ inline bool crowd_pair_begin(MathTabP mt, double dfx, double dfy, double dvx, double dvy, ProjPair& q) {
  const bool close = dfx * dfx + dfy * dfy < 1e-12;
  proj_pair_begin(mt, close ? 1e-6 : dfx, close ? 0.0 : dfy, dvx, dvy, q);
  return close;
}

// wrap(atan2(y, x)) with atan2(0, 0) = 0 (a standing person has heading 0)
__device__ inline double crowd_heading(MathTabP mt, double x, double y) {
  const double m = fmax(fabs(x), fabs(y));
  if (m == 0.0) return 0.0;
  return proj_wrap((m > 1e-100 && m < 1e100) ? atan2_dir(mt, y, x) : atan2(y, x));
}

// the kernel arguments of the groups kernel: the plain step's, then what smpc_crowd_groups adds
struct CrowdGroupsParams {
  CrowdParams c;
  const int32_t* group_id;  // [B][Np]
  double factor_gaze, factor_coherence, factor_repulsion;
};

// kGroups: the kernel arguments P are CrowdGroupsParams (whose head is the plain step's), otherwise CrowdParams
template <bool kGroups, class P>
__global__ __launch_bounds__(kCrowdThreads) void smpc_crowd_step_kernel(const P) {
  SMPC_CHAIN_PRIORITY();
  const auto& p = *(const CrowdParams __attribute__((address_space(4)))*)__builtin_amdgcn_kernarg_segment_ptr();
  const auto* gp = (const CrowdGroupsParams __attribute__((address_space(4)))*)__builtin_amdgcn_kernarg_segment_ptr();
  const MathTabP mt = &p.mt;
  const int G = 1 << p.lgG;
  const int tid = blockIdx.x * kCrowdThreads + threadIdx.x;
  const int robot = tid >> p.lgG, g = tid & (G - 1);
  const int base = (threadIdx.x & 63) - g;  // first lane of the robot's group in the wavefront
  const bool live = robot < p.B;            // the lanes behind the last robot stay for the shuffles and write nothing
  const size_t b = live ? robot : p.B - 1;
  const int n = min(max(p.count[b], 0), p.Np);
  const bool act = g < n;  // this lane carries a person (of robot B - 1 once more behind the last robot)
  const bool has = live && act;
  const size_t slot = b * (size_t)p.Np + (size_t)g;
  const double dt = p.dt;
  const double kFd = 2.0, kFo = 20.0, kSig = 0.2, kRelax = 0.5;

  // ---- loads: the robot (every lane of the group), this lane's person, its goal and the grid entry of its cell
  const double rx = p.pose[3 * b], ry = p.pose[3 * b + 1], ryaw = p.pose[3 * b + 2], rv = p.twist[2 * b];
  double px = 0, py = 0, vx = 0, vy = 0, des = p.desired_speed, gx = 0, gy = 0, ox = 0, oy = 0;
  int cur = 0, nwp = 0;
  bool has_goal = false, on_grid = false;
  unsigned int ob = 0;
  int gid = -1;
  if (act) {
    if constexpr (kGroups) gid = gp->group_id[slot];
    const double* row = p.people + slot * 5;
    px = row[0]; py = row[1]; vx = row[2]; vy = row[3];
    cur = p.cursor[slot];
    nwp = min(max(p.n_waypoints[slot], 0), p.K);
    if (p.desired_speeds) des = p.desired_speeds[slot];
    if (p.od_indexes) {
      const size_t grid = p.od_shared ? 0 : b;
      ox = p.od_origin[2 * grid]; oy = p.od_origin[2 * grid + 1];
      on_grid = proj_obstacle_issue(p, p.od_indexes + grid * (size_t)p.od_width * (size_t)p.od_height, ox, oy, px, py, ob) == SMPC_PROJ_OK;
    }
    has_goal = cur >= 0 && cur < nwp;
    if (has_goal) {
      const double* w = p.waypoints + (slot * (size_t)p.K + (size_t)cur) * 2;
      gx = w[0]; gy = w[1];
    }
  }

  // ---- computeSocialForce (sfm.hpp:237-281): the robot first, then the other persons round by round
  double ax = 0.0, ay = 0.0;
  if (p.robot_visible) {
    double sn, cs;
    if (__builtin_expect(!(fabs(ryaw) <= 1e5), 0)) sincos(ryaw, &sn, &cs);
    else sincos_tab(mt, ryaw, &sn, &cs);
    ProjPair q;
    crowd_pair_begin(mt, rx - px, ry - py, vx - rv * cs, vy - rv * sn, q);
    q.near_axis = q.near_axis && act;
    if (__builtin_expect(q.near_axis, 0)) proj_pair_exact_theta(q);
    proj_pair_end(mt, q, ax, ay);
  }
  const int gg = act ? g : 0;  // idle lanes of the group shadow person 0 (their results are dropped)
  for (int kk = 1; 2 * kk <= n; kk += 2) {
    const bool two = 2 * (kk + 1) <= n;
    ProjPair q[2];
    bool close[2];
    double dvx[2], dvy[2], sfx[2], sfy[2], hx[2], hy[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int k = two ? kk + h : kk;
      int j = gg + k;
      j = j >= n ? j - n : j;
      const double qx = __shfl(px, base + j, 64), qy = __shfl(py, base + j, 64);
      const double wx = __shfl(vx, base + j, 64), wy = __shfl(vy, base + j, 64);
      dvx[h] = vx - wx; dvy[h] = vy - wy;
      close[h] = crowd_pair_begin(mt, qx - px, qy - py, dvx[h], dvy[h], q[h]) && act;
      q[h].near_axis = q[h].near_axis && act;
    }
    if (__builtin_expect(q[0].near_axis || q[1].near_axis, 0)) { proj_pair_exact_theta(q[0]); proj_pair_exact_theta(q[1]); }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      proj_pair_end(mt, q[h], sfx[h], sfy[h]);
      hx[h] = sfx[h]; hy[h] = sfy[h];  // what the partner subtracts: this lane's term, whose negative is the partner's own
    }
    if (__builtin_expect(close[0] || close[1], 0)) {  // a coincident pair: the partner's own term has diff = (1e-6, 0) too
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        ProjPair r;
        double tx, ty;
        proj_pair_begin(mt, 1e-6, 0.0, -dvx[h], -dvy[h], r);
        proj_pair_exact_theta(r);
        proj_pair_end(mt, r, tx, ty);
        if (close[h]) { hx[h] = -tx; hy[h] = -ty; }
      }
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      if (h == 1 && !two) break;
      const int k = kk + h;
      ax += sfx[h]; ay += sfy[h];
      if (2 * k != n) {  // (for even n the last round pairs the lanes mutually: nothing to hand over)
        int src = gg - k;
        src = src < 0 ? src + n : src;
        ax -= __shfl(hx[h], base + src, 64); ay -= __shfl(hy[h], base + src, 64);
      }
    }
  }
  // ---- the members of this person's group: position sum, size and repulsion sum (sfm.hpp:378-388), over the robot's
  // grouped lanes in ascending order; every lane of the robot makes the same trips (the shuffles need their sources awake)
  double gsx = 0.0, gsy = 0.0, grx = 0.0, gry = 0.0;
  int gsize = 0;
  if constexpr (kGroups) {
    unsigned long long m = (__ballot(act && gid >= 0) >> base) & (G == 64 ? ~0ull : (1ull << G) - 1ull);
    const double reach = 4.0 * p.person_radius * p.person_radius;
    while (m) {
      const int j = __builtin_ctzll(m);  // < n: only lanes with a person are in the mask
      m &= m - 1ull;
      const double qx = __shfl(px, base + j, 64), qy = __shfl(py, base + j, 64);
      const int qid = __shfl(gid, base + j, 64);
      if (qid == gid) {
        gsx += qx; gsy += qy; ++gsize;
        const double ux = px - qx, uy = py - qy;
        if (j != g && ux * ux + uy * uy < reach) { grx += ux; gry += uy; }
      }
    }
  }
  if (!has) return;

  // ---- computeDesiredForce (sfm.hpp:188-203)
  double fx, fy;
  double dux = 0.0, duy = 0.0;  // the desired direction: the unit vector to the goal, or (0, 0)
  {
    const double ddx = gx - px, ddy = gy - py;
    const double z = ddx * ddx + ddy * ddy;
    const double inv = rsqrt_pos(fmax(z, 1e-300));
    if (has_goal && z * inv > p.goal_radius) {
      fx = kFd * ((z > 0 ? ddx * inv : ddx) * des - vx) / kRelax;
      fy = kFd * ((z > 0 ? ddy * inv : ddy) * des - vy) / kRelax;
      if constexpr (kGroups) { dux = z > 0 ? ddx * inv : ddx; duy = z > 0 ? ddy * inv : ddy; }
    } else {
      fx = -vx / kRelax;
      fy = -vy / kRelax;
    }
  }
  fx += ax; fy += ay;
  // ---- computeObstacleForce (sfm.hpp:205-222) from the nearest obstacle of the person's cell, as a POSITION
  double mx, my;
  if (on_grid && proj_obstacle_finish(p, ob, ox, oy, px, py, mx, my) == SMPC_PROJ_OK) {
    const double z = mx * mx + my * my;
    const double inv = rsqrt_pos(fmax(z, 1e-300));
    const double e = kFo * exp_tab(mt, -(z * inv - p.person_radius) * (1.0 / kSig));
    fx += e * (z > 0 ? mx * inv : mx);
    fy += e * (z > 0 ? my * inv : my);
  }
  // ---- computeGroupForce (sfm.hpp:325-393) of a group of two or more: gaze + coherence + repulsion. A person without a
  // group force skips the addition (adding +0.0 would turn a -0.0 component into +0.0).
  if constexpr (kGroups) {
    if (gsize >= 2) {
      const double size = (double)gsize;
      // gaze: the others' centre of mass lies behind the desired direction (angle > pi/2: e < 0 for a unit direction)
      const double im = div_fast(1.0, size - 1.0);
      const double e = dux * ((gsx - px) * im - px) + duy * ((gsy - py) * im - py);
      double hx = 0.0, hy = 0.0;
      if (e < 0.0) { hx = gp->factor_gaze * e * dux; hy = gp->factor_gaze * e * duy; }
      // coherence: rel (tanh(|rel| - maxDistance) + 1) / 2 = rel / (1 + exp(-2 z)), the exponent kept non-positive
      const double cx = div_fast(gsx, size) - px, cy = div_fast(gsy, size) - py;
      const double z = proj_sqrt(cx * cx + cy * cy) - 0.5 * (size - 1.0);
      const double t = exp_tab(mt, -2.0 * fabs(z));
      const double s = gp->factor_coherence * div_fast(z >= 0.0 ? 1.0 : t, 1.0 + t);
      hx += cx * s; hy += cy * s;
      hx += gp->factor_repulsion * grx; hy += gp->factor_repulsion * gry;
      fx += hx; fy += hy;
    }
  }
  // ---- updatePosition (sfm.hpp:525-572)
  const double yaw_old = crowd_heading(mt, vx, vy);
  vx += fx * dt; vy += fy * dt;
  {
    const double z = vx * vx + vy * vy;
    const double inv = rsqrt_pos(fmax(z, 1e-300));
    if (z * inv > des) { vx = (z > 0 ? vx * inv : vx) * des; vy = (z > 0 ? vy * inv : vy) * des; }
  }
  const double vz = proj_wrap(crowd_heading(mt, vx, vy) - yaw_old) / dt;
  px += vx * dt; py += vy * dt;
  if (has_goal) {
    const double ddx = gx - px, ddy = gy - py;
    if (proj_sqrt(ddx * ddx + ddy * ddy) <= p.goal_radius) ++cur;
  }
  if (p.cyclic && cur >= nwp) cur = 0;
  double* row = p.people + slot * 5;
  row[0] = px; row[1] = py; row[2] = vx; row[3] = vy; row[4] = vz;
  p.cursor[slot] = cur;
}

}  // namespace smpc
