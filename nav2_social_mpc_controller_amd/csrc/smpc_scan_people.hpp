// smpc_scan_people.hpp — people detections from the scan (include/smpc_scan_people.h; the rule: smpc_scan_people_rule.hpp):
// per robot, neighbouring beams whose hits lie close together form segments, and a segment of a person's size is a detection.
//   One wavefront per robot, four robots per workgroup, no LDS, no s_barrier. Pass p takes beams 64 p .. 64 p + 63, lane j
//   beam 64 p + j, so a beam's predecessor sits in the lane below (one shuffle), for lane 0 in what the pass before carried
//   over; a lane's beam of the next pass is loaded before this pass's work; before the first pass beam n - 1 is read once more, by every lane from one address.
//   * A segment is judged where it closes: at beam k >= 1 whose predecessor is foreground and which is not linked to it, the
//     segment s .. k - 1 ends. s is the last start below k: the highest bit below the lane of the pass's ballot of starts,
//     or the start carried over. m = k - s.
//   * Sums: E_k = the sum of the foreground offsets of the beams below k, an exclusive wave scan plus the passes before
//     (|E| <= 4096 * 46340 fits 32 bits: a foreground offset lies within sqrt(range_d2) < 2^15.5). S = E_k - E_s, where the
//     closing lane takes E_s and o_s from the start's lane by a shuffle, or from the carry.
//   * Wrap: a segment that closes with no start below it anywhere is the head 0 .. k - 1 of the segment that wraps; it is
//     set aside (at most once). What is open at beam n - 1 is judged behind the loop, by every lane alike: the last start's
//     run to n - 1 plus the head, or with no start at all the whole circle (0, n). It has the largest s, so the rows come
//     out in ascending s as they are.
//   * Rows: the rank of an accepted segment is the running count plus the accepted lanes below it. Once Nd rows are out and
//     seg_stats is not asked for, no later pass can change anything: the loop ends.
//   Bounds: the entry point admits 1 <= n_beams <= 4096 and 1 <= Nd <= 64 only. Global reads are beam k < n_beams of robot
//   b < B, global writes rows rank < Nd of robot b < B, det_count[b] and seg_stats[b][0..3].
// Plain vector loads and stores, no atomics.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "smpc_math.hpp"
#include "smpc_scan_people_rule.hpp"

namespace smpc {

constexpr int kSpThreads = 256;  // four wavefronts = four robots

struct ScanPeopleParams {
  int B, n_beams, Nd, subtract_map, min_points, link_d2, width_d2_min, width_d2_max, range_d2;
  double res, ox, oy, body_offset;
  const double* pose;     // [B][3]
  const uint8_t* kind;    // [B][n_beams]
  const int32_t* cell;    // [B][n_beams][2]
  double* detections;     // [B][Nd][5]
  int32_t* det_count;     // [B]
  int32_t* det_segment;   // [B][Nd][4] or null
  int32_t* seg_stats;     // [B][4] or null
};

// A wave-uniform value in a vector register: what is carried from pass to pass and only meets per-lane arithmetic need not
// occupy scalar registers, which the kernel's arguments, the ballots and the loop state fill.
__device__ inline int sp_vector(int v) {
  asm("" : "+v"(v));
  return v;
}

// lane l's value, wave-uniform, in a vector register
__device__ inline int sp_lane(int v, int l) { return sp_vector(__builtin_amdgcn_readlane(v, l)); }

// beam k of a robot: its kind and its offset (one 8-byte load; the rows are 8-byte aligned wherever int32 pairs are)
__device__ inline void sp_load(const uint8_t* kind, const int32_t* cell, int k, uint32_t* kd, int* ox, int* oy) {
  int32_t o[2];
  __builtin_memcpy(o, cell + 2 * (size_t)k, sizeof(o));
  *kd = (uint32_t)kind[k]; *ox = o[0]; *oy = o[1];
}

// inclusive sum over the lanes 0 .. lane of the wavefront
__device__ inline int sp_wave_scan(int v, int lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int u = __shfl_up(v, d);
    if (lane >= d) v += u;
  }
  return v;
}

// one accepted segment's rows
__device__ inline void sp_write(const ScanPeopleParams& p, size_t row, int s, int m, int Sx, int Sy, int32_t ax, int32_t ay, double x, double y) {
  double px, py;
  sp_position(sp_centre(Sx, m, ax, p.ox, p.res), sp_centre(Sy, m, ay, p.oy, p.res), x, y, p.body_offset, &px, &py);
  double* dst = p.detections + row * 5;
  dst[0] = px; dst[1] = py; dst[2] = 0.0; dst[3] = 0.0; dst[4] = 0.0;
  if (p.det_segment) {
    int32_t* seg = p.det_segment + row * 4;
    seg[0] = s; seg[1] = m; seg[2] = Sx; seg[3] = Sy;
  }
}

__global__ __launch_bounds__(kSpThreads) void smpc_scan_people_kernel(const ScanPeopleParams p) {
  SMPC_CHAIN_PRIORITY();
  const int lane = (int)(threadIdx.x & 63u);
  const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const long long b = (long long)blockIdx.x * (kSpThreads / 64) + w;
  if (b >= p.B) return;  // wave-uniform
  const size_t r = (size_t)b;
  const int n = p.n_beams, Nd = p.Nd;
  const uint64_t below = (1ull << lane) - 1ull;  // the lanes before this one

  // step 1
  const double x = p.pose[3 * r], y = p.pose[3 * r + 1];
  int32_t ax = 0, ay = 0;
  if (!sp_robot_cell(x, y, p.ox, p.oy, p.res, &ax, &ay)) {  // wave-uniform: every lane read the same pose
    if (lane == 0) p.det_count[r] = 0;
    if (p.seg_stats && lane < 4) p.seg_stats[4 * r + (size_t)lane] = 0;
    return;
  }
  const uint8_t* kind = p.kind + r * (size_t)n;
  const int32_t* cell = p.cell + r * (size_t)n * 2;

  // beam n - 1: the predecessor of beam 0, and where the open segment ends
  const int last_x = sp_vector(cell[2 * (size_t)(n - 1)]), last_y = sp_vector(cell[2 * (size_t)(n - 1) + 1]);
  const bool last_fg = sp_foreground((uint32_t)kind[n - 1], p.subtract_map, last_x, last_y, p.range_d2);

  int pred_x = last_x, pred_y = last_y;  // carried over: the beam below lane 0
  bool pred_fg = last_fg;
  int base_x = 0, base_y = 0;            // the foreground offsets of the passes before, summed
  bool has_start = false;                // the last start so far: its beam, E there, its offset
  int cs = 0, cEx = 0, cEy = 0, cfx = 0, cfy = 0;
  bool has_head = false;                 // the head of the wrapping segment: beams 0 .. head_m - 1
  int head_m = 0, hSx = 0, hSy = 0, hlx = 0, hly = 0;
  int first_x = 0, first_y = 0;          // o_0
  int acc = 0, n_seg = 0, n_pts = 0, n_wid = 0;
  bool done = false;                     // Nd rows are out and nothing else is asked for
  uint32_t next_kd = 0u;                 // the next pass's beam of this lane, loaded one pass ahead
  int next_x = 0, next_y = 0;
  if (lane < n) sp_load(kind, cell, lane, &next_kd, &next_x, &next_y);

  for (int p0 = 0; p0 < n; p0 += 64) {   // every branch on a ballot or a carried value is wave-uniform
    const int k = p0 + lane;
    const bool valid = k < n;
    const uint32_t kd = next_kd;         // zeros where k >= n
    const int ox = next_x, oy = next_y;
    next_kd = 0u; next_x = 0; next_y = 0;
    if (k + 64 < n) sp_load(kind, cell, k + 64, &next_kd, &next_x, &next_y);
    // steps 2 and 3
    const bool fg = valid && sp_foreground(kd, p.subtract_map, ox, oy, p.range_d2);
    const uint64_t fgm = __ballot(fg);
    int qx = __shfl_up(ox, 1), qy = __shfl_up(oy, 1);
    bool qfg = ((fgm << 1) >> lane) & 1ull;
    if (lane == 0) { qx = pred_x; qy = pred_y; qfg = pred_fg; }
    const bool link = n >= 2 && fg && qfg && sp_linked(ox, oy, qx, qy, p.link_d2);
    // step 4
    const bool start = fg && !link;
    const bool closer = valid && k >= 1 && qfg && !link;  // the segment that ends at k - 1
    const uint64_t sm = __ballot(start), cm = __ballot(closer);
    // step 5
    const int ix = sp_wave_scan(fg ? ox : 0, lane), iy = sp_wave_scan(fg ? oy : 0, lane);
    const int Ex = base_x + ix - (fg ? ox : 0), Ey = base_y + iy - (fg ? oy : 0);

    if (cm != 0ull) {
      const uint64_t sb = sm & below;
      const bool local = sb != 0ull;
      const int src = local ? 63 - __builtin_clzll(sb) : 0;
      int sEx = __shfl(Ex, src), sEy = __shfl(Ey, src), fx = __shfl(ox, src), fy = __shfl(oy, src);
      int s = p0 + src;
      if (!local) { sEx = cEx; sEy = cEy; fx = cfx; fy = cfy; s = cs; }
      const bool head = closer && !local && !has_start;
      const bool seg = closer && !head;
      const int m = k - s, Sx = Ex - sEx, Sy = Ey - sEy;
      // step 6
      const int32_t gate = sp_gate(m, sp_dist2(fx, fy, qx, qy), p.min_points, p.width_d2_min, p.width_d2_max);
      const bool ok = seg && gate == kScanAccepted;
      const uint64_t okm = __ballot(ok);
      // steps 7 and 8
      const int rank = acc + (int)__builtin_popcountll(okm & below);
      if (ok && rank < Nd) sp_write(p, r * (size_t)Nd + (size_t)rank, s, m, Sx, Sy, ax, ay, x, y);
      acc += (int)__builtin_popcountll(okm);
      n_seg += (int)__builtin_popcountll(__ballot(seg));
      n_pts += (int)__builtin_popcountll(__ballot(seg && gate == kScanByPoints));
      n_wid += (int)__builtin_popcountll(__ballot(seg && gate == kScanByWidth));
      const uint64_t hm = __ballot(head);
      if (hm != 0ull) {  // at most once: the first closer of all
        const int hl = __builtin_ctzll(hm);
        has_head = true;
        head_m = sp_vector(p0 + hl);
        hSx = sp_lane(Ex, hl); hSy = sp_lane(Ey, hl);
        hlx = sp_lane(qx, hl); hly = sp_lane(qy, hl);
      }
    }

    // what the next pass needs
    if (sm != 0ull) {
      const int hs = 63 - __builtin_clzll(sm);
      has_start = true;
      cs = sp_vector(p0 + hs);
      cEx = sp_lane(Ex, hs); cEy = sp_lane(Ey, hs);
      cfx = sp_lane(ox, hs); cfy = sp_lane(oy, hs);
    }
    if (p0 == 0) { first_x = sp_lane(ox, 0); first_y = sp_lane(oy, 0); }
    base_x += sp_lane(ix, 63); base_y += sp_lane(iy, 63);
    pred_x = sp_lane(ox, 63); pred_y = sp_lane(oy, 63);
    pred_fg = (fgm >> 63) != 0ull;
    if (acc >= Nd && !p.seg_stats) { done = true; break; }
  }

  // what is open at beam n - 1: every lane holds the same numbers, lane 0 stores
  if (!done && last_fg) {
    int s = 0, m = n, Sx = base_x, Sy = base_y, fx = first_x, fy = first_y, lx = last_x, ly = last_y;
    if (has_start) {
      s = cs; m = n - cs + head_m; Sx = base_x - cEx + hSx; Sy = base_y - cEy + hSy; fx = cfx; fy = cfy;
      if (has_head) { lx = hlx; ly = hly; }
    }
    const int32_t gate = sp_gate(m, sp_dist2(fx, fy, lx, ly), p.min_points, p.width_d2_min, p.width_d2_max);
    if (gate == kScanAccepted) {
      if (acc < Nd && lane == 0) sp_write(p, r * (size_t)Nd + (size_t)acc, s, m, Sx, Sy, ax, ay, x, y);
      ++acc;
    }
    ++n_seg;
    n_pts += gate == kScanByPoints;
    n_wid += gate == kScanByWidth;
  }
  if (lane == 0) {
    p.det_count[r] = min(Nd, acc);
    if (p.seg_stats) { p.seg_stats[4 * r] = n_seg; p.seg_stats[4 * r + 1] = n_pts; p.seg_stats[4 * r + 2] = n_wid; p.seg_stats[4 * r + 3] = acc; }
  }
}

}  // namespace smpc
