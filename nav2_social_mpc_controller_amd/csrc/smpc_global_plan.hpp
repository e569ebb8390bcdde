// smpc_global_plan.hpp — global plans on a world map (include/smpc_global_plan.h; the rule: smpc_global_plan_rule.hpp):
//   smpc_goal_field_kernel    the exact integer cost-to-go of every world cell to one goal;
//   smpc_extract_plan_kernel  the walk down a field from each robot's pose, written as a plan [L][2].
//
// Goal field. One workgroup of 1024 lanes owns one goal's field, so workgroup barriers are the only synchronisation: no
// atomics, no write races, every cell of the field is written by the one lane that owns it in the tile being relaxed.
//   * The world is cut into tiles of 32 x 32 cells, one cell per lane. A tile visit loads the tile with its one-cell halo
//     into LDS (u32 potentials twice over, u16 weights; a weight of 0 marks an impassable cell or one outside the world),
//     each lane keeps the costs of its eight steps in registers, and the tile is relaxed to LOCAL convergence: a lane
//     pulls min(f[n] + k * w(n)) from one copy of the potentials and writes the other, one barrier per iteration; whether
//     any lane changed travels through a word per iteration parity. At most 1024 iterations (the cells of a tile); a tile
//     that has not settled by then is simply marked dirty again.
//   * Lanes whose cell changed write it back; those on the tile's rim mark the neighbouring tiles dirty. Dirty flags are
//     bytes in LDS, one per tile (per group of consecutive tiles once a world has more than 16384 tiles).
//   * A sweep runs over the flags in ascending order, 64 at a time by a ballot that every wave takes of the same bytes, and
//     looks at a chunk again after each visit, so what a visit marks further on is still visited in the same sweep. The
//     sweeps end when one finds no flag; more than world_x * world_y of them is a bug and sets *fail (SMPC_ERR_DEVICE).
//   Potentials only fall, towards the unique fixed point, so the order of the visits changes the time, not the result.
//
// Extraction. A sequential walk per robot, bound by latency: eight lanes per robot, one per neighbour, each with its loads
// of one step in flight together; the winner is the lowest passing lane of the robot's byte of the wave's ballot. The walk
// is made twice: the first pass judges it (steps, INCONSISTENT_FIELD) and writes nothing, the second writes the poses —
// a robot with an error keeps every byte of its rows. Runs beside the solves of an episode: SMPC_CHAIN_PRIORITY.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/smpc_global_plan.h"
#include "smpc_global_plan_rule.hpp"
#include "smpc_math.hpp"

namespace smpc {

constexpr int kGfTile = 32;                                // cells per tile side
constexpr int kGfThreads = kGfTile * kGfTile;              // one lane per tile cell
constexpr int kGfHalo = kGfTile + 2;                       // tile row with its halo
constexpr int kGfHaloCells = kGfHalo * kGfHalo;
constexpr int kGfFlagCap = 16384;                          // dirty flags (bytes of LDS)

struct GoalFieldParams {
  int G, world_x, world_y, world_shared;
  int tiles_x, n_tiles, tiles_per_flag, n_flags;           // n_flags <= kGfFlagCap
  GpCost cost;
  double resolution;
  const uint8_t* world;         // [G or 1][world_y][world_x]
  const double* world_origin;   // [G or 1][2]
  const double* goal;           // [G][2]
  uint32_t* field;              // [G][world_y][world_x]
  int32_t* status;              // [G] or null
  uint32_t* fail;               // one word, set when a field has not settled within its bound
};

__global__ __launch_bounds__(kGfThreads) void smpc_goal_field_kernel(const GoalFieldParams p) {
  __shared__ uint32_t s_f[2][kGfHaloCells];
  __shared__ uint16_t s_w[kGfHaloCells];
  __shared__ uint8_t s_flag[kGfFlagCap];
  __shared__ uint32_t s_stamp[2];
  const int g = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  const size_t wsel = p.world_shared ? 0 : (size_t)g;
  const uint32_t cells = (uint32_t)p.world_x * (uint32_t)p.world_y;  // < 2^31 (checked by the host)
  const uint8_t* world = p.world + wsel * (size_t)cells;
  uint32_t* field = p.field + (size_t)g * (size_t)cells;

  int32_t gx = 0, gy = 0;
  int status = 0;
  {
    const bool hx = gp_cell_axis(p.goal[2 * (size_t)g], p.world_origin[2 * wsel], p.resolution, p.world_x, &gx);
    const bool hy = gp_cell_axis(p.goal[2 * (size_t)g + 1], p.world_origin[2 * wsel + 1], p.resolution, p.world_y, &gy);
    if (!(hx && hy)) status = 1;
    else if (!gp_passable(p.cost, world[(size_t)gy * p.world_x + gx])) status = 2;
  }
  if (tid == 0 && p.status) p.status[g] = status;
  for (uint32_t i = tid; i < cells; i += kGfThreads) field[i] = kFieldUnreachable;
  for (int i = tid; i < p.n_flags; i += kGfThreads) s_flag[i] = 0;
  __syncthreads();
  if (status != 0) return;  // workgroup-uniform
  if (tid == 0) {
    field[(size_t)gy * p.world_x + gx] = 0u;
    s_flag[((gy / kGfTile) * p.tiles_x + gx / kGfTile) / p.tiles_per_flag] = 1;
  }

  const int lx = tid & (kGfTile - 1), ly = tid / kGfTile;
  const int li = (ly + 1) * kGfHalo + lx + 1;
  const int n_chunks = (p.n_flags + 63) / 64;
  for (uint32_t sweep = 0;; ++sweep) {
    bool dirty = false, failed = false;
    for (int c = 0; c < n_chunks && !failed; ++c) {
      for (int lo = 0; lo < 64;) {
        __syncthreads();  // the flags (and the field) as the last visit left them
        const int fi = c * 64 + lane;
        const unsigned long long m = __ballot(fi < p.n_flags && s_flag[fi] != 0) & (~0ull << lo);
        if (m == 0ull) break;  // every wave read the same bytes: workgroup-uniform
        if (sweep >= cells) { failed = true; break; }
        const int bit = __builtin_ctzll(m), grp = c * 64 + bit;
        dirty = true;
        lo = bit + 1;
        __syncthreads();  // every wave has read the chunk
        if (tid == 0) s_flag[grp] = 0;
        const int t_end = (grp + 1) * p.tiles_per_flag < p.n_tiles ? (grp + 1) * p.tiles_per_flag : p.n_tiles;
        for (int t = grp * p.tiles_per_flag; t < t_end; ++t) {
          // ---- one tile visit --------------------------------------------------------------------------------------
          const int ty = t / p.tiles_x, tx = t - ty * p.tiles_x;
          const int x0 = tx * kGfTile - 1, y0 = ty * kGfTile - 1;
          for (int i = tid; i < kGfHaloCells; i += kGfThreads) {
            const int hy = i / kGfHalo, hx = i - hy * kGfHalo;
            const int x = x0 + hx, y = y0 + hy;
            uint32_t f = kFieldUnreachable, w = 0u;
            if ((unsigned)x < (unsigned)p.world_x && (unsigned)y < (unsigned)p.world_y) {
              const size_t idx = (size_t)y * p.world_x + x;
              w = gp_weight(p.cost, world[idx]);
              f = field[idx];
            }
            s_f[0][i] = f; s_f[1][i] = f; s_w[i] = (uint16_t)w;
          }
          if (tid < 2) s_stamp[tid] = 0u;
          __syncthreads();
          uint32_t sc[8];  // cost of the step into neighbour k, 0: not allowed
          const uint32_t wc = s_w[li];
#pragma unroll
          for (int k = 0; k < 8; ++k) {
            const int dx = gp_dx(k), dy = gp_dy(k);
            sc[k] = wc ? gp_step_cost(k, s_w[li + dy * kGfHalo + dx], s_w[li + dx], s_w[li + dy * kGfHalo]) : 0u;
          }
          const uint32_t orig = s_f[0][li];
          uint32_t cur = orig;
          int buf = 0;
          bool more = true;
          for (uint32_t it = 1; it <= (uint32_t)kGfThreads && more; ++it) {
            uint32_t best = cur;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
              const uint32_t fn = s_f[buf][li + gp_dy(k) * kGfHalo + gp_dx(k)];
              const uint32_t cand = fn + sc[k];  // below the marker whenever it counts (the host's bound)
              best = (sc[k] != 0u && fn != kFieldUnreachable && cand < best) ? cand : best;
            }
            const bool changed = best < cur;
            cur = best;
            s_f[buf ^ 1][li] = cur;
            if (__ballot(changed) != 0ull && lane == 0) s_stamp[it & 1u] = it;
            __syncthreads();
            more = s_stamp[it & 1u] == it;  // the other word is the one iteration it + 1 writes
            buf ^= 1;
          }
          if (cur != orig) {
            field[(size_t)(y0 + 1 + ly) * p.world_x + (x0 + 1 + lx)] = cur;  // a cell of the world: it had a weight
            const int ax = lx == 0 ? -1 : (lx == kGfTile - 1 ? 1 : 0), ay = ly == 0 ? -1 : (ly == kGfTile - 1 ? 1 : 0);
            const int tiles_y = p.n_tiles / p.tiles_x;
            const bool inx = ax != 0 && (unsigned)(tx + ax) < (unsigned)p.tiles_x, iny = ay != 0 && (unsigned)(ty + ay) < (unsigned)tiles_y;
            if (inx) s_flag[(ty * p.tiles_x + tx + ax) / p.tiles_per_flag] = 1;
            if (iny) s_flag[((ty + ay) * p.tiles_x + tx) / p.tiles_per_flag] = 1;
            if (inx && iny) s_flag[((ty + ay) * p.tiles_x + tx + ax) / p.tiles_per_flag] = 1;
          }
          if (more && tid == 0) s_flag[grp] = 1;  // not settled within the bound: once more
          __syncthreads();  // the write-back is done before the next visit loads
        }
      }
    }
    if (failed) {
      if (tid == 0) *p.fail = 1u;
      break;
    }
    if (!dirty) break;
  }
}

constexpr int kEpThreads = 256;  // 32 robots of eight lanes

struct ExtractPlanParams {
  int B, G, L, stride, world_x, world_y, world_shared;
  GpCost cost;
  double resolution;
  const uint8_t* world;         // [G or 1][world_y][world_x]
  const double* world_origin;   // [G or 1][2]
  const uint32_t* field;        // [G][world_y][world_x]
  const double* goal;           // [G][2]
  const int32_t* robot_goal;    // [B]
  const double* pose;           // [B][3]
  double* plan;                 // [B][L][2]
  int32_t* plan_len;            // [B]
  int32_t* error;               // [B] or null
};

// Lane k of a robot at cell (x, y) with potential f: is neighbour k the next cell of the walk? *fn: its potential.
__device__ inline bool ep_probe(const ExtractPlanParams& p, const uint8_t* world, const uint32_t* field, int x, int y, uint32_t f,
                                int k, uint32_t* fn) {
  const int nx = x + gp_dx(k), ny = y + gp_dy(k);
  if (!((unsigned)nx < (unsigned)p.world_x && (unsigned)ny < (unsigned)p.world_y)) return false;
  // the loads of one step are independent of each other: one round trip per step
  const size_t idx = (size_t)ny * p.world_x + nx;
  const uint32_t vn = world[idx], pot = field[idx];
  uint32_t va = 0u, vb = 0u;
  if (k >= 4) { va = world[(size_t)y * p.world_x + nx]; vb = world[(size_t)ny * p.world_x + x]; }
  *fn = pot;
  const uint32_t sc = gp_step_cost(k, gp_weight(p.cost, vn), k >= 4 ? gp_weight(p.cost, va) : 1u, k >= 4 ? gp_weight(p.cost, vb) : 1u);
  return sc != 0u && pot != kFieldUnreachable && pot + sc == f;
}

__global__ __launch_bounds__(kEpThreads) void smpc_extract_plan_kernel(const ExtractPlanParams p) {
  SMPC_CHAIN_PRIORITY();
  const int lane = threadIdx.x & 63, k = lane & 7, first = lane & ~7;
  const long long b = ((long long)blockIdx.x * kEpThreads + threadIdx.x) >> 3;
  const uint32_t cells = (uint32_t)p.world_x * (uint32_t)p.world_y;
  const uint8_t* world = nullptr;
  const uint32_t* field = nullptr;
  int err = SMPC_PLAN_OK, cx = 0, cy = 0, rg = 0;
  uint32_t fc = 0u;
  double ox = 0.0, oy = 0.0, px = 0.0, py = 0.0;
  bool walk = false;
  if (b < p.B) {  // the eight lanes of a robot decide alike
    rg = p.robot_goal[b];
    if (rg < 0 || rg >= p.G) err = SMPC_PLAN_BAD_GOAL_INDEX;
    else {
      const size_t wsel = p.world_shared ? 0 : (size_t)rg;
      world = p.world + wsel * (size_t)cells;
      field = p.field + (size_t)rg * (size_t)cells;
      ox = p.world_origin[2 * wsel]; oy = p.world_origin[2 * wsel + 1];
      px = p.pose[3 * b]; py = p.pose[3 * b + 1];
      const bool hx = gp_cell_axis(px, ox, p.resolution, p.world_x, &cx), hy = gp_cell_axis(py, oy, p.resolution, p.world_y, &cy);
      if (!(hx && hy)) err = SMPC_PLAN_START_OUTSIDE;
      else if (!gp_passable(p.cost, world[(size_t)cy * p.world_x + cx])) err = SMPC_PLAN_START_BLOCKED;
      else {
        fc = field[(size_t)cy * p.world_x + cx];
        if (fc == kFieldUnreachable) err = SMPC_PLAN_UNREACHABLE;
        else walk = true;
      }
    }
  }
  // ---- first pass: the number of steps n, or INCONSISTENT_FIELD ------------------------------------------------------------
  uint32_t n = 0u;
  {
    int x = cx, y = cy;
    uint32_t f = fc;
    bool act = walk && f != 0u;
    while (__ballot(act) != 0ull) {
      uint32_t fn = 0u;
      const bool pass = act && ep_probe(p, world, field, x, y, f, k, &fn);
      const uint32_t mine = (uint32_t)(__ballot(pass) >> first) & 0xFFu;
      const int win = mine ? __builtin_ctz(mine) : 0;
      const uint32_t fw = __shfl(fn, first + win);
      if (act) {
        if (mine == 0u || n >= cells) { err = SMPC_PLAN_INCONSISTENT_FIELD; act = false; }
        else { x += gp_dx(win); y += gp_dy(win); f = fw; ++n; act = f != 0u; }
      }
    }
  }
  // ---- the plan's size -----------------------------------------------------------------------------------------------------
  int len = 0;
  uint32_t centres = 0u;
  bool goal_row = false;
  if (walk && err == SMPC_PLAN_OK) {
    const uint32_t total = 2u + (n ? (n - 1u) / (uint32_t)p.stride : 0u);   // pose, centres, goal point
    if (total > (uint32_t)p.L) { err = SMPC_PLAN_TRUNCATED; len = p.L; centres = (uint32_t)p.L - 1u; }
    else { len = (int)total; centres = total - 2u; goal_row = true; }
  } else {
    walk = false;
  }
  double* rows = p.plan + (size_t)(b < p.B ? b : 0) * (size_t)p.L * 2;
  if (b < p.B && k == 0) {
    p.plan_len[b] = len;
    if (p.error) p.error[b] = err;
    if (walk) {
      rows[0] = px; rows[1] = py;
      if (goal_row) { rows[2 * (size_t)(len - 1)] = p.goal[2 * (size_t)rg]; rows[2 * (size_t)(len - 1) + 1] = p.goal[2 * (size_t)rg + 1]; }
    }
  }
  // ---- second pass: the centres of c[j * stride], j = 1 .. centres -----------------------------------------------------------
  {
    int x = cx, y = cy;
    uint32_t f = fc, j = 1u, until = (uint32_t)p.stride;
    bool act = walk && centres != 0u;
    while (__ballot(act) != 0ull) {
      uint32_t fn = 0u;
      const bool pass = act && ep_probe(p, world, field, x, y, f, k, &fn);
      const uint32_t mine = (uint32_t)(__ballot(pass) >> first) & 0xFFu;
      const int win = mine ? __builtin_ctz(mine) : 0;
      const uint32_t fw = __shfl(fn, first + win);
      if (act) {
        if (mine == 0u) act = false;  // (the first pass walked the same cells: does not happen)
        else {
          x += gp_dx(win); y += gp_dy(win); f = fw;
          if (--until == 0u) {
            if (k < 2) rows[2 * (size_t)j + k] = k == 0 ? gp_centre(ox, x, p.resolution) : gp_centre(oy, y, p.resolution);
            until = (uint32_t)p.stride;
            act = ++j <= centres;
          }
        }
      }
    }
  }
}

}  // namespace smpc
