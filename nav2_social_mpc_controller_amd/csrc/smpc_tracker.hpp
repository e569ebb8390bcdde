// smpc_tracker.hpp — people tracks (include/smpc_tracker.h; the rule: smpc_tracker_rule.hpp): per robot, the tick's
// detections are associated with the robot's track slots, matched slots take an alpha-beta update, unmatched ones coast or
// are freed, unmatched detections are born into free slots, and the confirmed slots leave nearest first as the rows
// smpc_people_to_status_batch reads.
//   One wavefront per robot, four robots per workgroup, no s_barrier. Lane i owns slot i: its four doubles and four ints are
//   loaded once and stored once, and live in registers in between.
//   * Detections: lane j loads x and y of detection j into the wave's own 64 + 64 doubles of LDS (zeros where there is no
//     used detection, so no word of it is read unwritten); a ballot of the used ones is the wave-uniform mask `avail`.
//   * Association in rounds. A lane whose best pair is stale scans the detections of `avail` (broadcast LDS reads, ascending
//     j, strict less: the lowest j of equal d2 stays) for its smallest key. A butterfly minimum of the 64-bit keys (a double
//     >= +0 orders as its bits) finds the round's least d2; the lowest lane that holds it is the winner (d2, then slot, then
//     detection: the order of the rule). Its detection leaves `avail`; only the lanes whose best pair was that detection
//     scan again. At most min(Nt, Nd) rounds; a round without a qualifying pair ends the loop.
//   * Births by ranks: detection lane j of `avail` writes j to born[rank of j in avail]; free lane i with rank f among the
//     free lanes takes born[f] when f < min(free, unmatched). Ascending j meets ascending slot, and id = next_id + f.
//   * Output: the rank of a confirmed lane is the number of confirmed lanes whose (key, slot) is less, counted over
//     broadcast reads (v_readlane from a wave-uniform lane number) of the confirmed lanes only.
//   Bounds: the entry point admits 1 <= Nd, Nt, Np <= 64 only. Every LDS index is a lane number or a bit number of a 64-bit
//   mask (masked with 63 where it comes from a register); global rows are lane < Nt, lane < clamp(det_count, 0, Nd) and
//   rank < Np of robot b < B.
// Plain vector loads and stores, no atomics.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "smpc_math.hpp"
#include "smpc_tracker_rule.hpp"

namespace smpc {

constexpr int kTkThreads = 256;  // four wavefronts = four robots

struct TrackerParams {
  int B, Nd, Nt, Np, confirm_hits, max_missed;
  double dt, alpha, gain, gate;
  const double* detections;   // [B][Nd][5]
  const int32_t* det_count;   // [B]
  const double* robot_pose;   // [B][3]
  double* tracks;             // [B][Nt][4]
  int32_t* meta;              // [B][Nt][4]
  int32_t* next_id;           // [B]
  double* people;             // [B][Np][5]
  int32_t* count;             // [B]
  int32_t* out_track;         // [B][Np][2] or null
};

// the value `v` of lane `from` (wave-uniform) in every lane: v_readlane_b32
__device__ inline uint64_t tk_lane64(uint64_t v, int from) {
  return (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, from) |
         (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), from) << 32;
}

// orders this wave's LDS stores before its LDS loads: the slots are the wave's own
__device__ inline void tk_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__global__ __launch_bounds__(kTkThreads) void smpc_track_people_kernel(const TrackerParams p) {
  SMPC_CHAIN_PRIORITY();
  __shared__ double det_x[kTkThreads / 64][64];
  __shared__ double det_y[kTkThreads / 64][64];
  __shared__ int32_t born[kTkThreads / 64][64];
  const int lane = (int)(threadIdx.x & 63u);
  const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const long long b = (long long)blockIdx.x * (kTkThreads / 64) + w;
  if (b >= p.B) return;  // wave-uniform
  const size_t s = (size_t)b;
  const int Nt = p.Nt, Nd = p.Nd, Np = p.Np;
  const uint64_t below = (1ull << lane) - 1ull;  // the lanes before this one

  // steps 0 and 1: the slot, sanitised and predicted
  const bool slot = lane < Nt;
  double* const track = p.tracks + (s * (size_t)Nt + (size_t)(slot ? lane : 0)) * 4;
  int32_t* const meta = p.meta + (s * (size_t)Nt + (size_t)(slot ? lane : 0)) * 4;
  double x = 0.0, y = 0.0, vx = 0.0, vy = 0.0;
  int32_t state = kTrackFree, hits = 0, missed = 0, id = 0;
  if (slot) {
    x = track[0]; y = track[1]; vx = track[2]; vy = track[3];
    state = meta[0]; hits = meta[1]; missed = meta[2]; id = meta[3];
  }
  bool live = slot && tk_live(state, x, y, vx, vy);
  if (!live) { x = y = vx = vy = 0.0; state = kTrackFree; hits = missed = id = 0; }
  const double xp = tk_predict(x, vx, p.dt), yp = tk_predict(y, vy, p.dt);

  // step 2: the detections, into the wave's LDS
  const int n_det = min(max(p.det_count[s], 0), Nd);
  double zx = 0.0, zy = 0.0;
  bool used = false;
  if (lane < n_det) {
    const double* d = p.detections + (s * (size_t)Nd + (size_t)lane) * 5;
    zx = d[0]; zy = d[1];
    used = tk_finite(zx) && tk_finite(zy);
  }
  det_x[w][lane] = used ? zx : 0.0;
  det_y[w][lane] = used ? zy : 0.0;
  tk_wave_sync();
  uint64_t avail = __ballot(used);  // used detections not accepted yet; wave-uniform

  // step 3: greedy association in the order (d2, slot, detection)
  const double gate2 = tk_gate2(p.gate);
  bool matched = false, stale = live;
  int match_j = 0, best_j = 0;
  uint64_t best = kTrackNoKey;
  const int rounds = min(Nt, Nd);
  for (int r = 0; r < rounds && avail != 0ull; ++r) {
    if (__ballot(stale) != 0ull) {  // wave-uniform
      uint64_t nb = kTrackNoKey;
      int nj = 0;
      for (uint64_t m = avail; m != 0ull; m &= m - 1ull) {
        const int j = __builtin_amdgcn_readfirstlane(__builtin_ctzll(m)) & 63;
        const uint64_t k = tk_pair_key(det_x[w][j], det_y[w][j], xp, yp, gate2);
        if (k < nb) { nb = k; nj = j; }
      }
      if (stale) { best = nb; best_j = nj; }
      stale = false;
    }
    const uint64_t mine = live && !matched ? best : kTrackNoKey;
    uint64_t least = mine;
    for (int o = 32; o > 0; o >>= 1) {
      const uint64_t other = __shfl_xor(least, o);
      least = other < least ? other : least;
    }
    if (least == kTrackNoKey) break;  // wave-uniform: no qualifying pair is left
    const int wi = __builtin_amdgcn_readfirstlane(__builtin_ctzll(__ballot(mine == least))) & 63;
    const int wj = __builtin_amdgcn_readlane(best_j, wi) & 63;
    if (lane == wi) { matched = true; match_j = wj; }
    avail &= ~(1ull << wj);
    stale = live && !matched && best_j == wj;
  }

  // steps 4 and 5: update or coast
  if (live) {
    if (matched) {
      const double rx = det_x[w][match_j & 63] - xp, ry = det_y[w][match_j & 63] - yp;
      x = tk_update(xp, p.alpha, rx); y = tk_update(yp, p.alpha, ry);
      vx = tk_update(vx, p.gain, rx); vy = tk_update(vy, p.gain, ry);
      hits = tk_hit(hits); missed = 0;
      if (state == kTrackTentative && hits >= p.confirm_hits) state = kTrackConfirmed;
    } else {
      x = xp; y = yp;
      missed = tk_miss(missed);
      if (!tk_survives_miss(state, missed, p.max_missed)) {
        x = y = vx = vy = 0.0; state = kTrackFree; hits = missed = id = 0;
        live = false;
      }
    }
  }

  // step 6: births by ranks
  const bool is_free = slot && state == kTrackFree;
  const uint64_t free_mask = __ballot(is_free);
  const int n_born = min((int)__builtin_popcountll(free_mask), (int)__builtin_popcountll(avail));
  if ((avail >> lane) & 1ull) born[w][__builtin_popcountll(avail & below) & 63] = lane;
  tk_wave_sync();
  const uint32_t first_id = (uint32_t)p.next_id[s];
  if (is_free) {
    const int f = (int)__builtin_popcountll(free_mask & below);
    if (f < n_born) {
      const int j = born[w][f & 63] & 63;
      x = det_x[w][j]; y = det_y[w][j]; vx = vy = 0.0;
      state = tk_birth_state(p.confirm_hits); hits = 1; missed = 0; id = (int32_t)(first_id + (uint32_t)f);
    }
  }
  if (slot) {
    track[0] = x; track[1] = y; track[2] = vx; track[3] = vy;
    meta[0] = state; meta[1] = hits; meta[2] = missed; meta[3] = id;
  }
  if (lane == 0) p.next_id[s] = (int32_t)(first_id + (uint32_t)n_born);

  // step 7: the confirmed slots, nearest first
  const double rx = p.robot_pose[3 * s], ry = p.robot_pose[3 * s + 1];
  if (!(tk_finite(rx) && tk_finite(ry))) {  // wave-uniform
    if (lane == 0) p.count[s] = 0;
    return;
  }
  const bool conf = slot && state == kTrackConfirmed;
  const uint64_t key = conf ? tk_out_key(x, y, rx, ry) : kTrackNoKey;
  const uint64_t conf_mask = __ballot(conf);
  uint32_t rank = 0u;
  for (uint64_t m = conf_mask; m != 0ull; m &= m - 1ull) {
    const int i = __builtin_amdgcn_readfirstlane(__builtin_ctzll(m)) & 63;
    rank += tk_key_less(tk_lane64(key, i), (uint32_t)i, key, (uint32_t)lane) ? 1u : 0u;
  }
  if (conf && rank < (uint32_t)Np) {
    double* row = p.people + (s * (size_t)Np + (size_t)rank) * 5;
    row[0] = x; row[1] = y; row[2] = vx; row[3] = vy; row[4] = 0.0;
    if (p.out_track) {
      int32_t* t = p.out_track + (s * (size_t)Np + (size_t)rank) * 2;
      t[0] = lane; t[1] = id;
    }
  }
  if (lane == 0) p.count[s] = min(Np, (int)__builtin_popcountll(conf_mask));
}

}  // namespace smpc
