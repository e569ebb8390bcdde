// smpc_crowd_pool.hpp — one control period of a shared world's pedestrians (smpc_crowd_pool_step_batch,
// include/smpc_crowd_pool.h; the host-compilable part of the rule: smpc_crowd_pool_rule.hpp): rows 0 .. M-1 of ONE table
// move under the Social Force Model, every row within interaction_range is a partner. The bins are the gather's
// (smpc_nearest.hpp: offsets [G + 1] and rows [A] of its workspace, built by its own count / scan / scatter kernels).
//   Work: blockIdx.x is a bin, blockIdx.y one of kCpSplit strides over the bin's rows in tiles of kCpTile = 64; the movers
//   of a tile share the 3 x 3 block of bins around them. Blocks behind the last bin copy the movers that are in no bin (no
//   finite position: inert by rule 1); a block without a tile returns at once.
//   * Tile: 64 rows of the bin into LDS (x, y, vx, vy and the row, -1 for a row that is no mover or is inert; an inert
//     mover is copied here), their two int64 accumulators zeroed.
//   * Candidates: the block's three ranges of `rows` laid end to end (smpc_nearest.hpp), staged through LDS 256 at a time
//     (any population works: the whole table in one bin is 1 + A / 256 chunks), a row that is not live marked -1.
//   * Gate: wave w owns movers w, w + 4, ... of the tile. Per mover (wave-uniform) one candidate per lane: rule 2, ballot,
//     and the survivors are compacted (popcount of the lower lanes) into the WAVE's own queue in LDS as finished pair
//     inputs (diff, dv, mover slot). A queue entry does not point back into the chunk, so the queue runs on across
//     chunks and movers and a full wave of 64 pairs is evaluated whenever it holds 64: about one candidate in three
//     passes the gate, and the expensive part still runs on full waves. What is left at the end of the tile (< 64) is
//     evaluated once, partly filled.
//   * Pair term (rule 3) with proj_pair_* of smpc_sfm.hpp, each ordered pair on its own; the two components are
//     quantized (rule 4) and added to the mover's accumulators with 64-bit integer LDS atomics: the sum is the same in
//     any order. Accumulators and queue are touched by the owning wave alone: wave-level fences, no s_barrier in the gate
//     loop beyond the two per chunk that guard the staging.
//   * Tail: lane t < 64 of wave 0 finishes mover t: desired + social + obstacle force and updatePosition, restated from
//     smpc_crowd.hpp:198-223 and :244-261 (not factored out of that kernel: its ISA stays as it is, untouched).
// Integer atomics only, plain vector stores. `agents` is never written (rule 6).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/smpc.h"
#include "smpc_crowd.hpp"
#include "smpc_crowd_pool_rule.hpp"
#include "smpc_math.hpp"
#include "smpc_nearest.hpp"
#include "smpc_sfm.hpp"

namespace smpc {

constexpr int kCpThreads = 256, kCpWaves = kCpThreads / 64;
constexpr int kCpTile = 64;     // rows of a bin per tile: one tail lane each
constexpr int kCpChunk = 256;   // candidates staged at a time: one per thread
constexpr int kCpQueue = 128;   // pairs a wave's queue holds: < 64 left over + 64 new
constexpr int kCpSplit = 4;     // blocks that stride over one bin's tiles

struct CrowdPoolParams {
  int M, A, K, cyclic, grid_x, grid_y;
  int od_width, od_height;
  float od_resolution;
  double range, dt, goal_radius, person_radius, desired_speed;
  const double* agents;           // [A][5]
  const double* waypoints;        // [M][K][2]
  const int32_t* n_waypoints;     // [M]
  const double* desired_speeds;   // [M] or null
  const uint32_t* od_indexes;     // [od_height][od_width] or null
  const double* od_origin;        // [2]
  const int32_t* offsets;         // [G + 1]
  const int32_t* rows;            // [A]
  double* next;                   // [M][5]
  int32_t* cursor;                // [M]
  MathTab mt;
};

// all five doubles of row i of the table into next[i], bit for bit (an inert mover)
__device__ inline void cp_copy_row(const double* agents, double* next, size_t i) {
  const uint64_t* from = reinterpret_cast<const uint64_t*>(agents) + i * 5;
  uint64_t* to = reinterpret_cast<uint64_t*>(next) + i * 5;
  uint64_t row[5];
  for (int k = 0; k < 5; ++k) row[k] = from[k];
  for (int k = 0; k < 5; ++k) to[k] = row[k];
}

// one wave of queued pairs: rule 3, rule 4 and the accumulators of the pairs' movers; `on`: this lane carries a pair
__device__ inline void cp_eval_pairs(MathTabP mt, bool on, double dfx, double dfy, double dvx, double dvy, int m,
                                     unsigned long long* accx, unsigned long long* accy) {
  if (!on) { dfx = 1.0; dfy = 0.0; dvx = 0.0; dvy = 0.0; m = 0; }  // idle lanes evaluate a harmless pair and drop it
  ProjPair q;
  crowd_pair_begin(mt, dfx, dfy, dvx, dvy, q);
  q.near_axis = q.near_axis && on;
  if (__builtin_expect(q.near_axis, 0)) proj_pair_exact_theta(q);
  double sx, sy;
  proj_pair_end(mt, q, sx, sy);
  if (on) {
    atomicAdd(&accx[m], (unsigned long long)cp_quantize(sx));
    atomicAdd(&accy[m], (unsigned long long)cp_quantize(sy));
  }
}

__global__ __launch_bounds__(kCpThreads) void smpc_crowd_pool_step_kernel(const CrowdPoolParams) {
  SMPC_CHAIN_PRIORITY();
  const auto& p = *(const CrowdPoolParams __attribute__((address_space(4)))*)__builtin_amdgcn_kernarg_segment_ptr();
  const MathTabP mt = &p.mt;
  __shared__ double cx[kCpChunk], cy[kCpChunk], cvx[kCpChunk], cvy[kCpChunk];  // the staged candidates
  __shared__ int32_t crow[kCpChunk];                                            // their rows, -1: no partner of anybody
  __shared__ double tx[kCpTile], ty[kCpTile], tvx[kCpTile], tvy[kCpTile];       // the tile's rows
  __shared__ int32_t trow[kCpTile];                                             // their rows, -1: nothing to move
  __shared__ unsigned long long accx[kCpTile], accy[kCpTile];                   // rule 4's sums
  __shared__ double qfx[kCpWaves][kCpQueue], qfy[kCpWaves][kCpQueue], qvx[kCpWaves][kCpQueue], qvy[kCpWaves][kCpQueue];
  __shared__ int32_t qm[kCpWaves][kCpQueue];
  const int tid = (int)threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int G = p.grid_x * p.grid_y, A = p.A, M = p.M;
  const int bin = (int)blockIdx.x;
  if (bin >= G) {  // the movers that are in no bin: no finite position, inert
    const long long i = (long long)(bin - G) * kCpThreads + tid;
    if (blockIdx.y == 0 && i < M) {
      const double x = p.agents[(size_t)i * 5], y = p.agents[(size_t)i * 5 + 1];
      if (!(nn_finite(x) && nn_finite(y))) cp_copy_row(p.agents, p.next, (size_t)i);
    }
    return;
  }
  const int b0 = min(max(p.offsets[bin], 0), A), nb = min(max(p.offsets[bin + 1] - b0, 0), A - b0);
  if ((int)blockIdx.y * kCpTile >= nb) return;  // block-uniform: no tile for this block
  const int bx = bin % p.grid_x, by = bin / p.grid_x;
  const int x0 = max(bx - 1, 0), x1 = min(bx + 1, p.grid_x - 1);
  int start[3], len[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const int y = by - 1 + r;
    start[r] = len[r] = 0;
    if (y >= 0 && y < p.grid_y) {
      start[r] = min(max(p.offsets[y * p.grid_x + x0], 0), A);
      len[r] = min(max(p.offsets[y * p.grid_x + x1 + 1] - start[r], 0), A - start[r]);
    }
  }
  const int n01 = len[0] + len[1], total = n01 + len[2];
  const double range = p.range;

  for (int t0 = (int)blockIdx.y * kCpTile; t0 < nb; t0 += kCpSplit * kCpTile) {
    // ---- the tile: 64 rows of this bin
    if (tid < kCpTile) {
      int32_t row = -1;
      double x = 0.0, y = 0.0, vx = 0.0, vy = 0.0;
      if (t0 + tid < nb) {
        const int32_t c = p.rows[b0 + t0 + tid];
        if ((uint32_t)c < (uint32_t)M) {
          const double* a = p.agents + (size_t)c * 5;
          x = a[0]; y = a[1]; vx = a[2]; vy = a[3];
          if (cp_live(x, y, vx, vy)) row = c;
          else cp_copy_row(p.agents, p.next, (size_t)c);  // inert with a finite position
        }
      }
      tx[tid] = x; ty[tid] = y; tvx[tid] = vx; tvy[tid] = vy;
      trow[tid] = row;
      accx[tid] = 0ull; accy[tid] = 0ull;
    }
    __syncthreads();
    int nq = 0;  // wave-uniform: pairs in this wave's queue
    for (int c0 = 0; c0 < total; c0 += kCpChunk) {
      // ---- the next 256 candidates of the 3 x 3 block
      {
        const int t = c0 + tid;
        int32_t row = -1;
        double x = 0.0, y = 0.0, vx = 0.0, vy = 0.0;
        if (t < total) {
          const int at = t < len[0] ? start[0] + t : t < n01 ? start[1] + (t - len[0]) : start[2] + (t - n01);
          const int32_t c = (uint32_t)at < (uint32_t)A ? p.rows[at] : -1;
          if ((uint32_t)c < (uint32_t)A) {
            const double* a = p.agents + (size_t)c * 5;
            x = a[0]; y = a[1]; vx = a[2]; vy = a[3];
            if (cp_live(x, y, vx, vy)) row = c;
          }
        }
        cx[tid] = x; cy[tid] = y; cvx[tid] = vx; cvy[tid] = vy;
        crow[tid] = row;
      }
      __syncthreads();
      const int nc = min(kCpChunk, total - c0);
      // ---- gate and compaction: this wave's movers against the chunk
      for (int m = w; m < kCpTile; m += kCpWaves) {
        const int32_t mrow = __builtin_amdgcn_readfirstlane(trow[m]);
        if (mrow < 0) continue;  // wave-uniform
        const double rx = tx[m], ry = ty[m], rvx = tvx[m], rvy = tvy[m];
        for (int k0 = 0; k0 < nc; k0 += 64) {
          const int k = k0 + lane;
          bool hit = false;
          double ax = 0.0, ay = 0.0;
          if (k < nc) {
            const int32_t c = crow[k];
            ax = cx[k]; ay = cy[k];
            hit = c >= 0 && c != mrow && cp_interacts(rx, ry, ax, ay, range);
          }
          const uint64_t mask = __ballot(hit);
          if (mask == 0ull) continue;  // wave-uniform
          if (hit) {
            const int at = nq + (int)__builtin_popcountll(mask & ((1ull << lane) - 1ull));  // < 63 + 64
            qfx[w][at] = ax - rx; qfy[w][at] = ay - ry;      // diff = partner - mover
            qvx[w][at] = rvx - cvx[k]; qvy[w][at] = rvy - cvy[k];  // dv = the mover's velocity - the partner's
            qm[w][at] = m;
          }
          nq += (int)__builtin_popcountll(mask);
          if (nq >= 64) {  // wave-uniform: a full wave of pairs, off the top of the queue
            nn_wave_sync();
            nq -= 64;
            const int e = nq + lane;
            cp_eval_pairs(mt, true, qfx[w][e], qfy[w][e], qvx[w][e], qvy[w][e], qm[w][e], accx, accy);
            nn_wave_sync();
          }
        }
      }
      __syncthreads();  // the chunk is read out: the next one may overwrite it
    }
    if (nq > 0) {  // wave-uniform: what is left of the tile's pairs, one partly filled wave
      nn_wave_sync();
      const bool on = lane < nq;
      const int e = on ? lane : 0;
      cp_eval_pairs(mt, on, qfx[w][e], qfy[w][e], qvx[w][e], qvy[w][e], qm[w][e], accx, accy);
      nn_wave_sync();
    }
    __syncthreads();  // every wave's sums are in
    // ---- the tail: one lane per mover
    if (tid < kCpTile && trow[tid] >= 0) {
      const size_t i = (size_t)trow[tid];
      const double kFd = 2.0, kFo = 20.0, kSig = 0.2, kRelax = 0.5;
      const double dt = p.dt;
      double px = tx[tid], py = ty[tid], vx = tvx[tid], vy = tvy[tid];
      const double ax = cp_force((int64_t)accx[tid]), ay = cp_force((int64_t)accy[tid]);
      int cur = p.cursor[i];
      const int nwp = min(max(p.n_waypoints[i], 0), p.K);
      const double des = p.desired_speeds ? p.desired_speeds[i] : p.desired_speed;
      double gx = 0.0, gy = 0.0, ox = 0.0, oy = 0.0;
      bool on_grid = false;
      unsigned int ob = 0;
      if (p.od_indexes) {
        ox = p.od_origin[0]; oy = p.od_origin[1];
        on_grid = proj_obstacle_issue(p, p.od_indexes, ox, oy, px, py, ob) == SMPC_PROJ_OK;
      }
      const bool has_goal = cur >= 0 && cur < nwp;
      if (has_goal) {
        const double* wpt = p.waypoints + (i * (size_t)p.K + (size_t)cur) * 2;
        gx = wpt[0]; gy = wpt[1];
      }
      // computeDesiredForce (sfm.hpp:188-203)
      double fx, fy;
      {
        const double ddx = gx - px, ddy = gy - py;
        const double z = ddx * ddx + ddy * ddy;
        const double inv = rsqrt_pos(fmax(z, 1e-300));
        if (has_goal && z * inv > p.goal_radius) {
          fx = kFd * ((z > 0 ? ddx * inv : ddx) * des - vx) / kRelax;
          fy = kFd * ((z > 0 ? ddy * inv : ddy) * des - vy) / kRelax;
        } else {
          fx = -vx / kRelax;
          fy = -vy / kRelax;
        }
      }
      fx += ax; fy += ay;
      // computeObstacleForce (sfm.hpp:205-222) from the nearest obstacle of the mover's cell, as a POSITION
      double mx, my;
      if (on_grid && proj_obstacle_finish(p, ob, ox, oy, px, py, mx, my) == SMPC_PROJ_OK) {
        const double z = mx * mx + my * my;
        const double inv = rsqrt_pos(fmax(z, 1e-300));
        const double e = kFo * exp_tab(mt, -(z * inv - p.person_radius) * (1.0 / kSig));
        fx += e * (z > 0 ? mx * inv : mx);
        fy += e * (z > 0 ? my * inv : my);
      }
      // updatePosition (sfm.hpp:525-572)
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
      double* row = p.next + i * 5;
      row[0] = px; row[1] = py; row[2] = vx; row[3] = vy; row[4] = vz;
      p.cursor[i] = cur;
    }
    __syncthreads();  // the tile is finished: the next one may overwrite it
  }
}

}  // namespace smpc
