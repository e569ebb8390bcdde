// smpc_nearest.hpp — the nearest-agent gather of a shared world (include/smpc_nearest.h; the rule: smpc_nearest_rule.hpp):
// per robot, the at most Np nearest agents within range out of one table, nearest first, as the rows
// smpc_people_to_status_batch reads.
//   Binning: a counting sort of the agents' rows by bin into the workspace (offsets [G + 1], cursor [G], rows [A]).
//   * smpc_nearest_count_kernel: one lane per agent, one integer atomicAdd into cursor[bin] (zeroed by a memset before).
//     Agents without a finite x and y never qualify and are left out of the bins.
//   * smpc_nearest_scan_kernel: ONE workgroup of 1024 lanes turns the at most 65536 counts into exclusive prefix sums: each
//     lane sums a contiguous run of bins, the 1024 sums are scanned in LDS, each lane writes its run to offsets and cursor.
//   * smpc_nearest_scatter_kernel: one lane per agent, row -> rows[atomicAdd(cursor[bin], 1)]. The order inside a bin is the
//     atomics' arrival order; the result does not depend on it, because the selection key (d2, c) is a total order.
//   Bins are row-major in x: the three bins of one row of the 3 x 3 block around a robot are one contiguous range of rows.
//   Query (smpc_nearest_query_kernel): one wavefront per robot, four robots per workgroup, no barrier.
//   * The three ranges are laid end to end and taken 64 candidates at a time: a lane loads a row index, then that row's
//     x and y, computes d2 and applies the gate. Its key is (bits of d2, c).
//   * The wave keeps its best Np keys so far SORTED, lane k holding the k-th smallest. Once it holds Np, a candidate that
//     is not below the largest of them is dropped before any merge; a chunk that leaves no candidate costs no merge.
//   * Merge by rank counting with broadcast reads (v_readlane from a wave-uniform lane number): a kept key's new rank is its
//     lane plus the candidates below it, a candidate's rank is the kept keys plus the candidates below it. Only the lanes
//     that hold a key are broadcast (kept keys + surviving candidates, not 128). Keys of rank < Np go to slot[rank] of the
//     wave's own 64 slots of LDS and are read back by lane: a scatter needs no second pass that way. The slots are the
//     wave's alone, so a wave-level fence orders the stores and the loads; no s_barrier.
//   * Finally lane k < count copies the row of its key, all five words loaded before the first is stored.
// Integer atomics only, plain vector stores.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "smpc_math.hpp"
#include "smpc_nearest_rule.hpp"

namespace smpc {

constexpr int kNnThreads = 256;        // count / scatter: one lane per agent; query: four wavefronts = four robots
constexpr int kNnScanThreads = 1024;   // the scan's single workgroup

struct NearestParams {
  int B, Np, A, grid_x, grid_y;
  double ox, oy, bin_size, max_range;
  const double* agents;       // [A][5]
  const double* robot_pose;   // [B][3]
  const int32_t* self;        // [B] or null
  int32_t* offsets;           // [G + 1]
  int32_t* cursor;            // [G]
  int32_t* rows;              // [A]
  double* people;             // [B][Np][5]
  int32_t* count;             // [B]
  int32_t* source;            // [B][Np] or null
};

// the bin of agent c, or -1 when it has no finite position
__device__ inline int nn_agent_bin(const NearestParams& p, size_t c) {
  const double x = p.agents[c * 5], y = p.agents[c * 5 + 1];
  if (!(nn_finite(x) && nn_finite(y))) return -1;
  return nn_bin_axis(y, p.oy, p.bin_size, p.grid_y) * p.grid_x + nn_bin_axis(x, p.ox, p.bin_size, p.grid_x);
}

__global__ __launch_bounds__(kNnThreads) void smpc_nearest_count_kernel(const NearestParams p) {
  SMPC_CHAIN_PRIORITY();
  const long long c = (long long)blockIdx.x * kNnThreads + threadIdx.x;
  if (c >= p.A) return;
  const int bin = nn_agent_bin(p, (size_t)c);
  if (bin >= 0) atomicAdd(&p.cursor[bin], 1);
}

__global__ __launch_bounds__(kNnScanThreads) void smpc_nearest_scan_kernel(const NearestParams p) {
  SMPC_CHAIN_PRIORITY();
  __shared__ int32_t sums[kNnScanThreads];
  const int G = p.grid_x * p.grid_y, per = (G + kNnScanThreads - 1) / kNnScanThreads;
  const int t = (int)threadIdx.x, lo = min(t * per, G), hi = min(lo + per, G);
  int32_t mine = 0;
  for (int i = lo; i < hi; ++i) mine += p.cursor[i];
  sums[t] = mine;
  __syncthreads();
  for (int d = 1; d < kNnScanThreads; d <<= 1) {
    const int32_t below = t >= d ? sums[t - d] : 0;
    __syncthreads();
    sums[t] += below;
    __syncthreads();
  }
  int32_t run = sums[t] - mine;  // the agents in the bins before lo
  for (int i = lo; i < hi; ++i) {
    const int32_t n = p.cursor[i];
    p.offsets[i] = run;
    p.cursor[i] = run;
    run += n;
  }
  if (t == kNnScanThreads - 1) p.offsets[G] = sums[t];
}

__global__ __launch_bounds__(kNnThreads) void smpc_nearest_scatter_kernel(const NearestParams p) {
  SMPC_CHAIN_PRIORITY();
  const long long c = (long long)blockIdx.x * kNnThreads + threadIdx.x;
  if (c >= p.A) return;
  const int bin = nn_agent_bin(p, (size_t)c);
  if (bin < 0) return;
  const int32_t at = atomicAdd(&p.cursor[bin], 1);
  if ((uint32_t)at < (uint32_t)p.A) p.rows[at] = (int32_t)c;  // (always: count and scatter saw the same table)
}

// the value `v` of lane `from` (wave-uniform) in every lane: v_readlane_b32
__device__ inline uint32_t nn_lane32(uint32_t v, int from) { return (uint32_t)__builtin_amdgcn_readlane((int)v, from); }
__device__ inline uint64_t nn_lane64(uint64_t v, int from) {
  return (uint64_t)nn_lane32((uint32_t)v, from) | (uint64_t)nn_lane32((uint32_t)(v >> 32), from) << 32;
}

// orders this wave's LDS stores before its LDS loads (and the other way round): the slots are the wave's own
__device__ inline void nn_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__global__ __launch_bounds__(kNnThreads) void smpc_nearest_query_kernel(const NearestParams p) {
  SMPC_CHAIN_PRIORITY();
  __shared__ uint64_t slot_d[kNnThreads / 64][64];
  __shared__ uint32_t slot_c[kNnThreads / 64][64];
  const int lane = (int)(threadIdx.x & 63u);
  const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const long long b = (long long)blockIdx.x * (kNnThreads / 64) + w;
  if (b >= p.B) return;  // wave-uniform
  const size_t s = (size_t)b;
  const double rx = p.robot_pose[3 * s], ry = p.robot_pose[3 * s + 1];
  if (!(nn_finite(rx) && nn_finite(ry))) {  // wave-uniform
    if (lane == 0) p.count[s] = 0;
    return;
  }
  const int32_t self = p.self ? p.self[s] : -1;
  const int bx = nn_bin_axis(rx, p.ox, p.bin_size, p.grid_x), by = nn_bin_axis(ry, p.oy, p.bin_size, p.grid_y);
  const int x0 = max(bx - 1, 0), x1 = min(bx + 1, p.grid_x - 1);
  int start[3], len[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const int y = by - 1 + r;
    start[r] = len[r] = 0;
    if (y >= 0 && y < p.grid_y) {
      start[r] = p.offsets[y * p.grid_x + x0];
      len[r] = max(p.offsets[y * p.grid_x + x1 + 1] - start[r], 0);
    }
  }
  const int n01 = len[0] + len[1], total = n01 + len[2];
  const int Np = p.Np;
  uint64_t best_d = ~0ull;  // lane k < n_best: the k-th smallest key so far
  uint32_t best_c = ~0u;
  int n_best = 0;  // wave-uniform
  for (int t0 = 0; t0 < total; t0 += 64) {
    const int t = t0 + lane;
    bool cand = false;
    uint64_t cand_d = ~0ull;
    uint32_t cand_c = ~0u;
    if (t < total) {
      const int at = t < len[0] ? start[0] + t : t < n01 ? start[1] + (t - len[0]) : start[2] + (t - n01);
      const int32_t c = (uint32_t)at < (uint32_t)p.A ? p.rows[at] : -1;
      if ((uint32_t)c < (uint32_t)p.A && c != self) {
        const double ax = p.agents[(size_t)c * 5], ay = p.agents[(size_t)c * 5 + 1];
        const double d2 = nn_d2(rx, ry, ax, ay);
        if (nn_finite(ax) && nn_finite(ay) && nn_in_range(d2, p.max_range)) {
          const NnKey k = nn_key(d2, (uint32_t)c);
          cand = true; cand_d = k.d; cand_c = k.c;
        }
      }
    }
    if (n_best == Np)  // full: only a key below the largest kept one can enter
      cand = cand && nn_key_less(cand_d, cand_c, nn_lane64(best_d, Np - 1), nn_lane32(best_c, Np - 1));
    const uint64_t mask = __ballot(cand);
    if (mask == 0ull) continue;  // wave-uniform
    uint32_t rank_b = (uint32_t)lane, rank_c = 0u;
    for (uint64_t m = mask; m != 0ull; m &= m - 1ull) {
      const int i = __builtin_amdgcn_readfirstlane(__builtin_ctzll(m));
      const uint64_t kd = nn_lane64(cand_d, i);
      const uint32_t kc = nn_lane32(cand_c, i);
      rank_b += nn_key_less(kd, kc, best_d, best_c) ? 1u : 0u;
      rank_c += nn_key_less(kd, kc, cand_d, cand_c) ? 1u : 0u;
    }
    for (int i = 0; i < n_best; ++i)
      rank_c += nn_key_less(nn_lane64(best_d, i), nn_lane32(best_c, i), cand_d, cand_c) ? 1u : 0u;
    if (lane < n_best && rank_b < (uint32_t)Np) { slot_d[w][rank_b] = best_d; slot_c[w][rank_b] = best_c; }
    if (cand && rank_c < (uint32_t)Np) { slot_d[w][rank_c] = cand_d; slot_c[w][rank_c] = cand_c; }
    nn_wave_sync();
    n_best = min(Np, n_best + (int)__builtin_popcountll(mask));
    best_d = lane < n_best ? slot_d[w][lane] : ~0ull;
    best_c = lane < n_best ? slot_c[w][lane] : ~0u;
    nn_wave_sync();
  }
  if (lane < n_best) {
    const uint64_t* from = reinterpret_cast<const uint64_t*>(p.agents) + (size_t)best_c * 5;
    uint64_t* to = reinterpret_cast<uint64_t*>(p.people) + (s * (size_t)Np + (size_t)lane) * 5;
    uint64_t row[5];
    for (int k = 0; k < 5; ++k) row[k] = from[k];
    for (int k = 0; k < 5; ++k) to[k] = row[k];
    if (p.source) p.source[s * (size_t)Np + (size_t)lane] = (int32_t)best_c;
  }
  if (lane == 0) p.count[s] = n_best;
}

}  // namespace smpc
