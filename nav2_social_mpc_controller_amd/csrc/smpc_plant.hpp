// smpc_plant.hpp — the robot plant (include/smpc_plant.h; the rule: smpc_plant_rule.hpp): per robot, the command that is due
// after the latency is clamped and rate-limited, the period's straight segment is walked in S substeps, and the walk ends in
// front of the first substep that brings the disc closer to a wall cell within its footprint or to an agent in contact.
//   One wavefront per robot, four robots per workgroup, no LDS, no s_barrier. The robot's own state (pose, twist, the due
//   command) is loaded by every lane and taken from lane 0, so it is wave-uniform by construction; lane 0 alone stores.
//   * The agent scan: lane j loads x and y of agent j once and keeps them in registers over all substeps; at every point its
//     key is the bits of its squared distance when in contact, and a butterfly minimum of the 64-bit keys leaves the least
//     in every lane.
//   * The wall scan: the lanes take the offsets of the footprint's bounding square, row by row, in passes of 64 (at most 16
//     passes for the largest footprint: 31 x 31 = 961 offsets); each reads its world cell directly (the map is shared by all
//     robots and small beside the L2) and keeps the least squared offset that is a wall, then a butterfly minimum. The scan
//     runs at q_0 and then only when a substep's cell differs from the previous one: a substep is a fraction of a cell.
//   * The walk ends at the first blocked substep (a wave-uniform branch on values every lane holds).
//   Bounds: the entry point admits 1 <= Np <= 64, 1 <= S <= 16, 0 <= L <= 8, footprint_d2 <= 225 only. Global rows are
//   lane < clamp(count, 0, Np) of robot b < B, queue slot tick mod L < 8, and world cell (x, y) only after
//   0 <= x < Hx and 0 <= y < Hy (pl_is_wall).
// Plain vector loads and stores, no atomics.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "smpc_math.hpp"
#include "smpc_plant_rule.hpp"

namespace smpc {

constexpr int kPlThreads = 256;  // four wavefronts = four robots

struct PlantParams {
  int B, Np, S, L;
  PlantWalls walls;
  double dt, v_min, v_max, w_max, dv_up, dv_down, dw, contact2, res, ox, oy;
  const double* cmd;       // [B][2]
  const double* agents;    // [B][Np][5]
  const int32_t* count;    // [B]
  double* pose;            // [B][3]
  double* twist;           // [B][2]
  double* queue;           // [B][8][2] or null (L == 0)
  uint32_t* tick;          // [B]
  int32_t* contact;        // [B][2]
  double* heading;         // [B][2] or null
  MathTab mt;
};

// lane 0's value in every lane (v_readfirstlane_b32 twice): the robot's own scalars
__device__ inline double pl_uniform(double v) {
  const uint64_t u = pl_bits(v);
  const uint64_t r = (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)u) |
                     (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(u >> 32)) << 32;
  double d;
  __builtin_memcpy(&d, &r, sizeof(double));
  return d;
}

__global__ __launch_bounds__(kPlThreads) void smpc_robot_plant_kernel(const PlantParams p) {
  SMPC_CHAIN_PRIORITY();
  const MathTabP mt = &((const PlantParams SMPC_TAB_AS*)__builtin_amdgcn_kernarg_segment_ptr())->mt;
  const int lane = (int)(threadIdx.x & 63u);
  const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const long long b = (long long)blockIdx.x * (kPlThreads / 64) + w;
  if (b >= p.B) return;  // wave-uniform
  const size_t s = (size_t)b;
  const int S = p.S;

  // step 1: the command that is due, and the tick's command into its slot
  const uint32_t tick = (uint32_t)__builtin_amdgcn_readfirstlane((int)p.tick[s]);
  double tv, tw;
  if (p.L > 0) {
    double* slot = p.queue + (s * (size_t)kPlantMaxLatency + (size_t)(tick % (uint32_t)p.L)) * 2;
    tv = pl_uniform(slot[0]); tw = pl_uniform(slot[1]);
    const double cv = p.cmd[2 * s], cw = p.cmd[2 * s + 1];
    if (lane == 0) { slot[0] = cv; slot[1] = cw; }
  } else {
    tv = pl_uniform(p.cmd[2 * s]); tw = pl_uniform(p.cmd[2 * s + 1]);
  }
  if (lane == 0) p.tick[s] = tick + 1u;

  // step 2: the state
  const double x = pl_uniform(p.pose[3 * s]), y = pl_uniform(p.pose[3 * s + 1]), th = pl_uniform(p.pose[3 * s + 2]);
  const double v = pl_uniform(p.twist[2 * s]), wz = pl_uniform(p.twist[2 * s + 1]);
  if (!(pl_finite(x) && pl_finite(y) && pl_finite(th) && pl_finite(v) && pl_finite(wz))) {  // wave-uniform
    if (lane == 0) {
      p.twist[2 * s] = 0.0; p.twist[2 * s + 1] = 0.0;
      p.contact[2 * s] = kPlantBadState; p.contact[2 * s + 1] = 0;
    }
    return;
  }
  int flags = 0;
  if (!(pl_finite(tv) && pl_finite(tw))) { tv = 0.0; tw = 0.0; flags |= kPlantBadCommand; }

  // steps 3 to 5: the executed twist, the heading, the period's segment
  const double v1 = pl_limit_v(v, tv, p.v_min, p.v_max, p.dv_up, p.dv_down);
  const double w1 = pl_limit_w(wz, tw, p.w_max, p.dw);
  double c, sn;
  pl_heading(mt, th, &c, &sn);
  if (p.heading && lane == 0) { p.heading[2 * s] = c; p.heading[2 * s + 1] = sn; }
  const double Lx = pl_length(v1, c, p.dt), Ly = pl_length(v1, sn, p.dt);

  // step 6: lane j keeps agent j
  const int n = min(max(p.count[s], 0), p.Np);
  double px = 0.0, py = 0.0;
  bool has = false;
  if (lane < n) {
    const double* row = p.agents + (s * (size_t)p.Np + (size_t)lane) * 5;
    px = row[0]; py = row[1];
    has = pl_finite(px) && pl_finite(py);
  }
  const double contact2 = p.contact2;
  auto agent2 = [&](double qx, double qy) {
    uint64_t k = has ? pl_agent_key(px, py, qx, qy, contact2) : kPlantNoAgent;
    for (int o = 32; o > 0; o >>= 1) {
      const uint64_t other = __shfl_xor(k, o);
      k = other < k ? other : k;
    }
    return k;
  };
  const PlantWalls walls = p.walls;
  const int n_off = (2 * walls.r + 1) * (2 * walls.r + 1);
  auto wall2 = [&](int32_t cx, int32_t cy) {
    uint32_t k = kPlantNoWall;
    for (int t = lane; t < n_off; t += 64) {
      const uint32_t kt = pl_offset_key(walls, cx, cy, t);
      k = kt < k ? kt : k;
    }
    for (int o = 32; o > 0; o >>= 1) {
      const uint32_t other = (uint32_t)__shfl_xor((int)k, o);
      k = other < k ? other : k;
    }
    return k;
  };
  const bool walls_on = pl_walls_on(walls);

  // q_0
  int32_t cx = 0, cy = 0;
  bool cell_ok = __builtin_amdgcn_readfirstlane((int)(walls_on && pl_cell(x, y, p.ox, p.oy, p.res, &cx, &cy))) != 0;
  cx = __builtin_amdgcn_readfirstlane(cx); cy = __builtin_amdgcn_readfirstlane(cy);
  uint32_t wk = cell_ok ? wall2(cx, cy) : kPlantNoWall;
  uint64_t ak = agent2(x, y);
  if (wk != kPlantNoWall) flags |= kPlantWallContact;
  if (ak != kPlantNoAgent) flags |= kPlantAgentContact;

  // step 7: the walk
  int K = 0;
  double qx = x, qy = y;
  for (int k = 1; k <= S; ++k) {
    const double nx = pl_point(x, Lx, k, S), ny = pl_point(y, Ly, k, S);
    int32_t ncx = 0, ncy = 0;
    const bool nok = __builtin_amdgcn_readfirstlane((int)(walls_on && pl_cell(nx, ny, p.ox, p.oy, p.res, &ncx, &ncy))) != 0;
    ncx = __builtin_amdgcn_readfirstlane(ncx); ncy = __builtin_amdgcn_readfirstlane(ncy);
    uint32_t nwk = kPlantNoWall;
    if (nok) nwk = (cell_ok && ncx == cx && ncy == cy) ? wk : wall2(ncx, ncy);
    const uint64_t nak = agent2(nx, ny);
    const int blocked = __builtin_amdgcn_readfirstlane((nwk < wk ? kPlantBlockedByWall : 0) | (nak < ak ? kPlantBlockedByAgent : 0));
    if (blocked != 0) { flags |= blocked; break; }
    K = k; qx = nx; qy = ny; cx = ncx; cy = ncy; cell_ok = nok; wk = nwk; ak = nak;
  }

  // steps 7 and 8: the new state
  if (lane == 0) {
    p.pose[3 * s] = qx; p.pose[3 * s + 1] = qy; p.pose[3 * s + 2] = pl_turn(th, w1, p.dt);
    p.twist[2 * s] = K == S ? v1 : 0.0; p.twist[2 * s + 1] = w1;
    p.contact[2 * s] = flags; p.contact[2 * s + 1] = K;
  }
}

}  // namespace smpc
