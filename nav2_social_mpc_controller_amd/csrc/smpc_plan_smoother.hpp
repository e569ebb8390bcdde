// smpc_plan_smoother.hpp — plan smoothing (include/smpc_plan_smoother.h; the rule: smpc_plan_smoother_rule.hpp):
//   smpc_smooth_plan_kernel<S>   one wavefront per plan, four plans per workgroup, the iterate in registers, no LDS.
//
// Layout. Pose i lives in lane i mod 64, slot i div 64; a lane holds S slots (S = 7 for L <= 448, S = 16 for L <= 1024) of
// four doubles: the iterate y and the round's starting rows p, both axes, plus one word per slot for the row's last cell
// verdict. Loads and stores are coalesced (a slot is 64 consecutive rows), and a plan of n rows costs ceil(n / 64) slots: the
// slots behind it are skipped on a wave-uniform test. Rows i - 1 and i + 1 of the previous iterate are the slot rotated by one
// lane either way; lane 0 takes row i - 1 from the rotation of the slot below, lane 63 row i + 1 from that of the slot above.
// The sweep runs through the slots upwards and overwrites them in place: the rotation of a slot is taken before it is
// overwritten and handed on, so every candidate is formed from the previous iterate (Jacobi).
//
// The cell test. The two divisions of a candidate's cell are made every sweep (the rule's own function: no shortcut is taken
// that could name another cell for some double); the map is read only by the lanes whose candidate has left the cell of their
// last verdict, behind a wave-uniform test, which after the first sweeps is false nearly always.
//
// The round. "change <= tolerance" for the sweep's maximum is "no lane moved a row by more than tolerance": one ballot. The
// maximum itself is reduced once, after the last sweep. Rejections are counted from ballots into a scalar. The only open loop
// runs at most max_its * (refinement_num + 1) times.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/smpc_plan_smoother.h"
#include "smpc_math.hpp"
#include "smpc_plan_smoother_rule.hpp"

namespace smpc {

constexpr int kSmThreads = 256;          // four wavefronts = four plans
constexpr int kSmSlotsShort = 7;         // L <= 448
constexpr int kSmSlotsLong = 16;         // L <= 1024 = SMPC_SMOOTH_MAX_POSES
static_assert(64 * kSmSlotsLong == SMPC_SMOOTH_MAX_POSES, "the long kernel holds the longest plan");

struct PlanSmootherParams {
  int B, L, world_x, world_y, world_shared, max_its, refinement_num;
  uint32_t lethal_min, allow_unknown;
  double res, w_data, w_smooth, tolerance;
  const uint8_t* world;         // [B or 1][world_y][world_x]
  const double* origin;         // [B or 1][2]
  const int32_t* plan_len;      // [B]
  const int32_t* range;         // [B][2] or null
  double* plan;                 // [B][L][2]
  int32_t* status;              // [B]
  int32_t* info;                // [B][4] or null
  double* change;               // [B] or null
};

// the value of the lane below (lane 0: of lane 63) and of the lane above (lane 63: of lane 0)
__device__ inline double sm_from_below(double v, int lane) { return __shfl(v, (lane + 63) & 63); }
__device__ inline double sm_from_above(double v, int lane) { return __shfl(v, (lane + 1) & 63); }

// The same value, opaque to the compiler where it stands: the lane predicates derived from the movable mask are then computed
// slot by slot inside the sweep instead of being kept in a scalar register pair each from the top of the kernel.
__device__ inline uint32_t sm_fresh(uint32_t v) {
  asm volatile("" : "+v"(v));
  return v;
}

template <int S>
__global__ __launch_bounds__(kSmThreads) void smpc_smooth_plan_kernel(const PlanSmootherParams p) {
  const int lane = (int)(threadIdx.x & 63u);
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const long long bb = (long long)blockIdx.x * (kSmThreads / 64) + wv;
  if (bb >= p.B) return;  // wave-uniform
  const size_t b = (size_t)bb;
  const size_t wsel = p.world_shared ? 0 : b;
  const uint8_t* world = p.world + wsel * (size_t)p.world_x * (size_t)p.world_y;
  const SmMap map = {p.origin[2 * wsel], p.origin[2 * wsel + 1], p.res, p.world_x, p.world_y, p.lethal_min, p.allow_unknown};
  double* rows = p.plan + b * (size_t)p.L * 2;
  const int32_t n = sm_rows(p.plan_len[b], p.L);   // <= L <= 64 * S (the host picks S)

  double yx[S], yy[S], px[S], py[S];
  uint32_t verdict[S];
  bool finite = true;
#pragma unroll
  for (int k = 0; k < S; ++k) {
    const int i = 64 * k + lane;
    yx[k] = 0.0; yy[k] = 0.0;
    if (i < n) {
      yx[k] = rows[2 * (size_t)i]; yy[k] = rows[2 * (size_t)i + 1];
      finite = finite && sm_finite(yx[k]) && sm_finite(yy[k]);
    }
    px[k] = yx[k]; py[k] = yy[k];
    verdict[k] = kSmNoVerdict;
  }
  int32_t first = 0, last = 0;
  const bool has_range = p.range != nullptr;
  const bool any_movable = sm_movable(n, has_range, has_range ? p.range[2 * b] : 0, has_range ? p.range[2 * b + 1] : 0, &first, &last);
  uint32_t movable = 0u;   // bit k: this lane's row of slot k may move
#pragma unroll
  for (int k = 0; k < S; ++k) {
    const int i = 64 * k + lane;
    movable |= (i >= first && i <= last) ? (1u << k) : 0u;
  }

  SmProgress prog = sm_start();
  unsigned long long rejected = 0ull;
  double moved = 0.0;   // this lane's largest |h| of the last sweep
  // every branch below is on a value the 64 lanes share
  if (__ballot(!finite) != 0ull) {
    prog.status = kSmoothBadPlan;
  } else if (!any_movable) {
    prog.status = kSmoothTooShort;
  } else {
    const long long bound = sm_sweep_bound(p.max_its, p.refinement_num);
    for (long long t = 0; t < bound; ++t) {
      moved = 0.0;
      double below_x = 0.0, below_y = 0.0;   // the slot below, rotated upwards: its lane 63 in lane 0
      double above_x = sm_from_above(yx[0], lane), above_y = sm_from_above(yy[0], lane);   // this slot, rotated downwards
      const uint32_t may_move = sm_fresh(movable);
#pragma unroll
      for (int k = 0; k < S; ++k) {
        if (64 * k < n) {   // wave-uniform: the slots behind the plan hold no row
          const double ox = yx[k], oy = yy[k];
          const double up_x = sm_from_below(ox, lane), up_y = sm_from_below(oy, lane);
          double next_x = 0.0, next_y = 0.0;   // the slot above, rotated downwards: its lane 0 in lane 63
          if (k + 1 < S) {
            next_x = sm_from_above(yx[k + 1], lane);
            next_y = sm_from_above(yy[k + 1], lane);
          }
          const double mx = lane == 0 ? below_x : up_x, my = lane == 0 ? below_y : up_y;          // row i - 1
          const double qx = lane == 63 ? next_x : above_x, qy = lane == 63 ? next_y : above_y;    // row i + 1
          const bool mine = ((may_move >> k) & 1u) != 0u;
          const double cx = sm_candidate(px[k], ox, mx, qx, p.w_data, p.w_smooth);
          const double cy = sm_candidate(py[k], oy, my, qy, p.w_data, p.w_smooth);
          int32_t idx = 0;
          const bool in_map = mine && sm_cell(map, cx, cy, &idx);
          const bool stale = in_map && !sm_verdict_is_of(verdict[k], idx);
          if (__ballot(stale) != 0ull) {
            if (stale) verdict[k] = sm_verdict(idx, sm_passable(map, (uint32_t)world[(size_t)idx]));
          }
          const bool accepted = in_map && sm_verdict_passable(verdict[k]);
          rejected += (unsigned long long)__popcll(__ballot(mine && !accepted));
          if (accepted) {
            yx[k] = cx; yy[k] = cy;
            const double hx = sm_moved(cx, ox), hy = sm_moved(cy, oy);
            const double h = hx > hy ? hx : hy;
            moved = h > moved ? h : moved;
          }
          below_x = up_x; below_y = up_y;
          above_x = next_x; above_y = next_y;
        }
        __builtin_amdgcn_sched_barrier(0);   // slot by slot: interleaving the slots costs more registers than a lane has
      }
      const bool within = __ballot(!(moved <= p.tolerance)) == 0ull;
      const int then = sm_after_sweep(prog, within, p.max_its, p.refinement_num);
      if (then == kSmStop) break;
      if (then == kSmNextRound) {
#pragma unroll
        for (int k = 0; k < S; ++k) { px[k] = yx[k]; py[k] = yy[k]; }
      }
    }
#pragma unroll
    for (int k = 0; k < S; ++k) {
      const int i = 64 * k + lane;
      if ((movable >> k) & 1u) { rows[2 * (size_t)i] = yx[k]; rows[2 * (size_t)i + 1] = yy[k]; }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
      const double other = __shfl_xor(moved, m);
      moved = other > moved ? other : moved;
    }
  }
  if (lane == 0) {
    p.status[b] = prog.status;
    if (p.info) { int32_t* o = p.info + 4 * b; o[0] = prog.sweeps; o[1] = prog.rounds; o[2] = sm_saturate(rejected); o[3] = n; }
    if (p.change) p.change[b] = moved;
  }
}

}  // namespace smpc
