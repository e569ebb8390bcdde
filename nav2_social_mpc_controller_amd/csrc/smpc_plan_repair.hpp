// smpc_plan_repair.hpp — plan repair (include/smpc_plan_repair.h; the rule: smpc_plan_repair_rule.hpp):
//   smpc_repair_judge_kernel   rules 1 to 5: which robots have a blocked stretch in view, and where they rejoin their plan;
//   smpc_repair_field_kernel   rules 6 to 10 for those robots: the region's field, the walk, the splice.
//
// Judging. One wavefront per robot, four robots per workgroup, no LDS. The closest pose is an arg-min over passes of 64
// poses: every lane keeps the best key (d2, i) of its own poses, a butterfly over the key makes the wave agree. The stretch
// in view is walked in passes of 64 poses from i0: a ballot of the poses without a cell in the region ends it, a ballot of
// the blocked poses below that end gives the least and the greatest blocked index, carried from pass to pass; the rejoin is
// the first set bit of a third ballot over the poses behind i2. A robot with work left gets the transient status
// kRepairPending and leaves i0 and j in the first 8 bytes of its workspace rows (L >= 2: they hold 32).
//
// Field. A workgroup takes robots blockIdx.x, blockIdx.x + gridDim.x, .. and skips every one that is not pending: a clear
// robot costs one status word. The region's potentials (u32) and weights (u16) sit in LDS with a one-cell halo, (S + 2)^2 *
// 6 bytes (99,846 at R = 63); the robot's cell is the region's centre. The cells are relaxed in place in four colours,
// (x & 1, y & 1): two cells of one colour are never neighbours, so a phase reads only what the phases before wrote; one
// barrier per phase, no atomics, no write races. A sweep is four phases, the colour of the robot's cell last, so the cap
// F(a) a sweep reads at its start is not written before the sweep's last phase. A candidate above the cap is dropped (rule
// 10). Whether any lane changed a cell travels through a word per sweep parity. Potentials only fall, towards the unique
// fixed point; sweeps are bounded by S * S. Eight lanes of the first wavefront then walk down the field, one neighbour each,
// the winner the lowest set bit of a ballot, and write the detour's centres into the workspace; the workgroup appends the
// old rows from j on, and behind a barrier copies the workspace over the plan, so rows that move forwards and rows that
// move backwards are the same case.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/smpc_plan_repair.h"
#include "smpc_math.hpp"
#include "smpc_plan_repair_rule.hpp"

namespace smpc {

constexpr int kPrJudgeThreads = 256;    // four wavefronts = four robots
constexpr int kPrFieldMaxThreads = 1024;

struct PlanRepairParams {
  int B, L, size_x, size_y, costmap_shared, R, stride;
  GpCost cost;
  double res, clearance_d2;
  const uint8_t* costmap;       // [B or 1][size_y][size_x]
  const double* origin;         // [B or 1][2]
  const double* pose;           // [B][3]
  const int32_t* plan_start;    // [B] or null
  double* plan;                 // [B][L][2]
  int32_t* plan_len;            // [B]
  double* workspace;            // [B][L][2]
  int32_t* status;              // [B]
  int32_t* info;                // [B][4] or null
  uint32_t* field;              // [B][S][S] or null
};

// LDS of the field kernel for radius R: potentials, then weights, over the haloed region
inline size_t pr_field_lds_bytes(int R) {
  const size_t cells = (size_t)(2 * R + 3) * (size_t)(2 * R + 3);
  return (cells * 6 + 15) & ~(size_t)15;
}

// A workgroup-uniform value in a vector register: what a robot carries through the field kernel and only meets per-lane
// arithmetic or a store need not occupy scalar registers, which the kernel's arguments and the sweep's loop state fill.
template <typename T> __device__ inline T pr_vector(T v) {
  asm("" : "+v"(v));
  return v;
}

// The same value, computed afresh where it stands: a lane predicate derived from it is then not kept in a scalar register
// pair from the top of the kernel to its only use.
__device__ inline int pr_fresh(int v) {
  asm volatile("" : "+v"(v));
  return v;
}

// a pose of the stretch in view: kPoseOutOfView, or what its cell makes of it
__device__ inline int pr_classify(const PlanRepairParams& p, const PrWindow& win, const uint8_t* costmap, double px, double py, int32_t ax, int32_t ay) {
  int32_t cx = 0, cy = 0;
  if (!pr_region_cell(win, px, py, ax, ay, p.R, &cx, &cy)) return kPoseOutOfView;
  return pr_pose_class(p.cost, (uint32_t)costmap[(size_t)cy * (size_t)p.size_x + (size_t)cx], cx == ax && cy == ay);
}

__global__ __launch_bounds__(kPrJudgeThreads) void smpc_repair_judge_kernel(const PlanRepairParams p) {
  SMPC_CHAIN_PRIORITY();
  const int lane = (int)(threadIdx.x & 63u);
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const long long bb = (long long)blockIdx.x * (kPrJudgeThreads / 64) + wv;
  if (bb >= p.B) return;  // wave-uniform
  const size_t b = (size_t)bb;
  const size_t wsel = p.costmap_shared ? 0 : b;
  const uint8_t* costmap = p.costmap + wsel * (size_t)p.size_x * (size_t)p.size_y;
  const double* rows = p.plan + b * (size_t)p.L * 2;
  const PrWindow win = {p.origin[2 * wsel], p.origin[2 * wsel + 1], p.res, p.size_x, p.size_y};

  int32_t st = kRepairPending, i0 = -1, i1 = -1, j = -1;
  const int32_t n = p.plan_len[b], s = p.plan_start ? p.plan_start[b] : 0;
  const double x = p.pose[3 * b], y = p.pose[3 * b + 1];
  int32_t ax = 0, ay = 0;
  // every branch below is on a value the 64 lanes share
  if (n < 2 || n > p.L || s < 0 || s >= n) {
    st = kRepairNoPlan;
  } else if (!(gp_cell_axis(x, win.ox, win.res, win.sx, &ax) && gp_cell_axis(y, win.oy, win.res, win.sy, &ay))) {
    st = kRepairNoCell;
  } else {
    // ---- rule 3: the closest pose ----------------------------------------------------------------------------------------
    bool bv = false;
    double bd = 0.0;
    int32_t bi = 0;
    for (long long i = (long long)s + lane; i < n; i += 64) {
      const double d = pr_d2(rows[2 * (size_t)i], rows[2 * (size_t)i + 1], x, y);
      const bool v = pr_finite(d);
      if (pr_closer(v, d, (int32_t)i, bv, bd, bi)) { bv = true; bd = d; bi = (int32_t)i; }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
      const bool ov = __shfl_xor((int)bv, m) != 0;
      const double od = __shfl_xor(bd, m);
      const int32_t oi = __shfl_xor(bi, m);
      if (pr_closer(ov, od, oi, bv, bd, bi)) { bv = true; bd = od; bi = oi; }
    }
    if (!bv) {
      st = kRepairNoPlan;
    } else {
      i0 = bi;
      // ---- rule 4: the stretch in view, its least and greatest blocked pose ---------------------------------------------
      int32_t i2 = -1;
      long long e = n;
      for (long long base = i0; base < n; base += 64) {
        const long long i = base + lane;
        int cls = kPoseOutOfView;
        if (i < n) cls = pr_classify(p, win, costmap, rows[2 * (size_t)i], rows[2 * (size_t)i + 1], ax, ay);
        const unsigned long long out = __ballot(i < n && cls == kPoseOutOfView);
        const int lim = out ? __builtin_ctzll(out) : 64;
        const unsigned long long blocked = __ballot(cls == kPoseBlocked) & (lim < 64 ? (1ull << lim) - 1ull : ~0ull);
        if (blocked) {
          if (i1 < 0) i1 = (int32_t)(base + __builtin_ctzll(blocked));
          i2 = (int32_t)(base + 63 - __builtin_clzll(blocked));
        }
        if (out) { e = base + lim; break; }
      }
      if (i1 < 0) {
        st = kRepairClear;
      } else {
        // ---- rule 5: the rejoin --------------------------------------------------------------------------------------------
        const double qx = rows[2 * (size_t)i2], qy = rows[2 * (size_t)i2 + 1];
        for (long long base = (long long)i2 + 1; base < e; base += 64) {
          const long long i = base + lane;
          bool ok = false;
          if (i < e) {
            const double px = rows[2 * (size_t)i], py = rows[2 * (size_t)i + 1];
            ok = pr_classify(p, win, costmap, px, py, ax, ay) == kPosePassable && pr_d2(px, py, qx, qy) >= p.clearance_d2;
          }
          const unsigned long long hit = __ballot(ok);
          if (hit) { j = (int32_t)(base + __builtin_ctzll(hit)); break; }
        }
        if (j < 0) st = kRepairNoRejoin;
      }
    }
  }
  if (lane == 0) {
    p.status[b] = st;
    if (p.info) { int32_t* o = p.info + 4 * b; o[0] = i0; o[1] = i1; o[2] = j; o[3] = -1; }
    if (st == kRepairPending) {
      const int32_t keep[2] = {i0, j};
      __builtin_memcpy(p.workspace + b * (size_t)p.L * 2, keep, sizeof(keep));
    }
  }
}

__global__ __launch_bounds__(kPrFieldMaxThreads) void smpc_repair_field_kernel(const PlanRepairParams pk) {
  PlanRepairParams p = pk;  // addresses and what only the region's set-up and the splice read: vector registers
  p.costmap = pr_vector(pk.costmap); p.origin = pr_vector(pk.origin); p.pose = pr_vector(pk.pose); p.plan = pr_vector(pk.plan);
  p.plan_len = pr_vector(pk.plan_len); p.workspace = pr_vector(pk.workspace); p.status = pr_vector(pk.status); p.info = pr_vector(pk.info);
  p.field = pr_vector(pk.field); p.L = pr_vector(pk.L); p.stride = pr_vector(pk.stride); p.size_x = pr_vector(pk.size_x); p.size_y = pr_vector(pk.size_y);
  p.res = pr_vector(pk.res); p.cost.neutral = pr_vector(pk.cost.neutral); p.cost.weight = pr_vector(pk.cost.weight);
  p.cost.lethal_min = pr_vector(pk.cost.lethal_min); p.cost.allow_unknown = pr_vector(pk.cost.allow_unknown);
  extern __shared__ __attribute__((aligned(16))) uint32_t pr_lds[];
  __shared__ uint32_t s_stamp[2];
  __shared__ int32_t s_walk[3];  // failed, m, K
  const int tid = (int)threadIdx.x, lane = tid & 63, nthreads = (int)blockDim.x;
  const int wave = tid >> 6, nwaves = nthreads >> 6;
  const int R = p.R, S = 2 * R + 1, pitch = S + 2, cells = pitch * pitch;
  uint32_t* s_f = pr_lds;
  uint16_t* s_w = reinterpret_cast<uint16_t*>(pr_lds + cells);
  const int ia = (R + 1) * pitch + R + 1;  // the robot's cell: the region's centre
  const uint32_t sweep_max = (uint32_t)(S * S);
  const int vpitch = pr_vector(pitch);     // the eight neighbour offsets of a probe: per-lane arithmetic

  for (long long bb = blockIdx.x; bb < p.B; bb += gridDim.x) {
    const size_t b = (size_t)bb;
    if (p.status[b] != kRepairPending) continue;  // workgroup-uniform: nobody writes the word before the barriers below
    const size_t wsel = p.costmap_shared ? 0 : b;
    const uint8_t* costmap = p.costmap + wsel * (size_t)p.size_x * (size_t)p.size_y;
    double* rows = p.plan + b * (size_t)p.L * 2;
    double* ws = p.workspace + b * (size_t)p.L * 2;
    const PrWindow win = {pr_vector(p.origin[2 * wsel]), pr_vector(p.origin[2 * wsel + 1]), p.res, p.size_x, p.size_y};
    const int32_t n = pr_vector(p.plan_len[b]);
    int32_t keep[2];
    __builtin_memcpy(keep, ws, sizeof(keep));  // what the judging kernel left
    const int32_t i0 = pr_vector(keep[0]), j = pr_vector(keep[1]);
    const double x = pr_vector(p.pose[3 * b]), y = pr_vector(p.pose[3 * b + 1]);
    int32_t ax = 0, ay = 0, tx = 0, ty = 0;
    (void)gp_cell_axis(x, win.ox, win.res, win.sx, &ax);   // the judging kernel found these four
    (void)gp_cell_axis(y, win.oy, win.res, win.sy, &ay);
    (void)gp_cell_axis(rows[2 * (size_t)j], win.ox, win.res, win.sx, &tx);
    (void)gp_cell_axis(rows[2 * (size_t)j + 1], win.oy, win.res, win.sy, &ty);
    const int x0 = ax - R - 1, y0 = ay - R - 1;  // window cell of the halo's corner

    // ---- rule 6: the region, then its field ------------------------------------------------------------------------------
    for (int hy = wave; hy < pitch; hy += nwaves) {
      for (int hx = lane; hx < pitch; hx += 64) {
        const int wx = x0 + hx, wy = y0 + hy;
        uint32_t w = 0u;
        if (hx >= 1 && hx <= S && hy >= 1 && hy <= S && (unsigned)wx < (unsigned)p.size_x && (unsigned)wy < (unsigned)p.size_y)
          w = pr_weight(p.cost, (uint32_t)costmap[(size_t)wy * (size_t)p.size_x + (size_t)wx], wx == ax && wy == ay);
        s_w[hy * pitch + hx] = (uint16_t)w;
        s_f[hy * pitch + hx] = (wx == tx && wy == ty) ? 0u : kFieldUnreachable;
      }
    }
    if (tid < 2) s_stamp[tid] = 0u;
    __syncthreads();
    const int last_colour = (R & 1) * 3;  // the colour of the centre (R, R) in region coordinates: (R & 1, R & 1)
    bool failed = false;
    for (uint32_t sweep = 1;; ++sweep) {
      const uint32_t cap = s_f[ia];
      bool changed = false;
#pragma unroll 1
      for (int ph = 1; ph <= 4; ++ph) {
        const int colour = (last_colour + ph) & 3, cx = colour & 1, cy = colour >> 1;
        const int nx = (S + 1 - cx) >> 1, ny = (S + 1 - cy) >> 1;  // nx <= 64: one lane per cell of a colour's row
        for (int qy = wave; qy < ny; qy += nwaves) {
          if (lane < nx) {
            const int idx = (2 * qy + cy + 1) * pitch + 2 * lane + cx + 1;
            const uint32_t cur = s_f[idx], v = pr_relax(s_f, s_w, idx, vpitch, cap);
            if (v != cur) { s_f[idx] = v; changed = true; }
          }
        }
        if (ph == 4 && __ballot(changed) != 0ull && lane == 0) s_stamp[sweep & 1u] = sweep;
        __syncthreads();
      }
      if (s_stamp[sweep & 1u] != sweep) break;  // the other word is the one sweep + 1 writes
      if (sweep >= sweep_max) { failed = true; break; }
    }
    const uint32_t fa = s_f[ia];

    const int tl = pr_fresh(tid), ll = tl & 63;  // this lane, for the robot's tail
    // ---- rule 10 -----------------------------------------------------------------------------------------------------------
    if (p.field) {
      uint32_t* out = p.field + b * (size_t)S * (size_t)S;
      for (int ry = wave; ry < S; ry += nwaves)
        for (int rx = ll; rx < S; rx += 64) out[(size_t)ry * S + rx] = pr_field_out(s_f[(ry + 1) * pitch + rx + 1], fa);
    }

    // ---- rule 7: the walk, and the detour's centres into the workspace -----------------------------------------------------
    int32_t st = failed ? kRepairInconsistent : (fa == kFieldUnreachable ? kRepairUnreachable : kRepairPending);
    if (st == kRepairPending && wave == 0) {
      int idx = ia, rx = R, ry = R;
      int32_t m = 0, K = 0, until = p.stride;
      uint32_t fc = fa;
      bool bad = false;
      while (fc != 0u) {  // wave-uniform
        const unsigned long long pass = __ballot(ll < 8 && pr_walk_probe(s_f, s_w, idx, vpitch, ll & 7)) & 0xFFull;
        if (pass == 0ull || (uint32_t)m >= sweep_max) { bad = true; break; }
        const int k = __builtin_ctzll(pass);
        idx += pr_offset(k, pitch); rx += gp_dx(k); ry += gp_dy(k);
        fc = s_f[idx];
        ++m;
        if (--until == 0) {
          until = p.stride;
          if (fc != 0u) {  // c[m] is a pose only while m is not the walk's last cell
            if (K < p.L && ll < 2) ws[2 * (size_t)K + ll] = ll == 0 ? gp_centre(win.ox, ax - R + rx, win.res) : gp_centre(win.oy, ay - R + ry, win.res);
            ++K;
          }
        }
      }
      if (ll == 0) { s_walk[0] = bad ? 1 : 0; s_walk[1] = m; s_walk[2] = K; }
    }
    __syncthreads();

    // ---- rule 8: the splice ------------------------------------------------------------------------------------------------
    int32_t m = -1;
    if (st == kRepairPending) {  // workgroup-uniform
      const int32_t K = s_walk[2];
      if (s_walk[0]) {
        st = kRepairInconsistent;
      } else {
        m = s_walk[1];
        const int64_t len = pr_new_length(i0, K, n, j);
        if (len > (int64_t)p.L) {
          st = kRepairTooLong;
        } else {
          st = kRepairRepaired;
          const size_t tail = 2 * (size_t)(n - j), moved = 2 * (size_t)K + tail;
          for (size_t r = (size_t)tl; r < tail; r += (size_t)nthreads) ws[2 * (size_t)K + r] = rows[2 * (size_t)j + r];
          __syncthreads();  // every old row is read, the workspace complete
          for (size_t r = (size_t)tl; r < moved; r += (size_t)nthreads) rows[2 * ((size_t)i0 + 1) + r] = ws[r];
          if (tl < 2) rows[2 * (size_t)i0 + tl] = tl == 0 ? x : y;
          if (tl == 0) p.plan_len[b] = (int32_t)len;
        }
      }
    }
    if (tl == 0) {
      p.status[b] = st;
      if (p.info) p.info[4 * b + 3] = m;
    }
    __syncthreads();  // the region and the walk's words are free for the next robot
  }
}

}  // namespace smpc
