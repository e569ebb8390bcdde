// smpc_visibility.hpp — the line-of-sight filter of the people a robot perceives (include/smpc_visibility.h; the rule:
// smpc_visibility_rule.hpp): per robot, the persons within range whose sight line over the world map no cell occludes are
// compacted, in order, into the rows smpc_people_to_status_batch reads next.
//   * One wavefront per robot (four robots per workgroup, no barrier). Its persons are taken 64 at a time, one per lane:
//     the lane loads its person, finds the cells, applies the range gate and sets up its ray (vis_ray), all in one pass.
//   * The cells of a ray are known before anything is loaded, and every column of every ray is independent (vis_column).
//     So the columns of the chunk's rays are laid end to end (a prefix sum of the rays' lengths over the lanes) and the lanes
//     share out that one list, 64 columns per round: a lane finds the ray of its column by a binary search of the prefix
//     sums (six cross-lane reads), fetches the ray (three more) and tests the column's two to four cells. A round is one
//     memory round trip whatever the rays' lengths, where a ray at a time costs one per ray: 8 rays of 38 columns are 5
//     rounds, not 8, and the persons' rows come in one trip instead of one each. A hit sets the ray's bit in the lane's mask;
//     the masks are OR-ed across the wave once, after the last round. (A ray that is hit is still walked to its end.)
//   * Compaction: a ballot of the seen lanes; a seen lane's row goes to the slot given by the seen lanes before it, copied as
//     five 8-byte words, bit for bit. No LDS allocation, no atomics, plain vector stores.
// The world map is small and read-only: its bytes come from L2.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "smpc_math.hpp"
#include "smpc_visibility_rule.hpp"

namespace smpc {

constexpr int kVisThreads = 256;  // four wavefronts = four robots

struct VisibilityParams {
  int B, Np, world_x, world_y, world_shared;
  VisOcc occ;
  double resolution, max_range;
  const uint8_t* world;          // [B or 1][world_y][world_x]
  const double* world_origin;    // [B or 1][2]
  const double* robot_pose;      // [B][3]
  const double* people;          // [B][Np][5]
  const int32_t* count;          // [B]
  double* visible;               // [B][Np][5]
  int32_t* visible_count;        // [B]
  uint8_t* seen;                 // [B][Np] or null
};

// The value `v` of lane `from` (0 .. 63) of the wavefront: ds_bpermute_b32, no LDS is allocated. Not __shfl(): with this
// kernel's call sites beside its own, the compiler emitted other index arithmetic inside smpc_extract_plan_kernel
// (tools/isa_identity.py), and no existing kernel may change.
__device__ inline uint32_t vis_lane_read(uint32_t v, uint32_t from) {
  return (uint32_t)__builtin_amdgcn_ds_bpermute((int)(from << 2), (int)v);
}

__global__ __launch_bounds__(kVisThreads) void smpc_visible_people_kernel(const VisibilityParams p) {
  SMPC_CHAIN_PRIORITY();
  const uint32_t lane = threadIdx.x & 63u;
  const long long b = (long long)blockIdx.x * (kVisThreads / 64) + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (b >= p.B) return;  // wave-uniform
  const size_t s = (size_t)b, g = p.world_shared ? 0 : s;
  const uint8_t* world = p.world + g * (size_t)p.world_x * (size_t)p.world_y;
  const double ox = p.world_origin[2 * g], oy = p.world_origin[2 * g + 1];
  const double rx = p.robot_pose[3 * s], ry = p.robot_pose[3 * s + 1];
  const int cnt = min(max(p.count[s], 0), p.Np);
  const uint64_t* rows = reinterpret_cast<const uint64_t*>(p.people) + s * (size_t)p.Np * 5;
  uint64_t* out = reinterpret_cast<uint64_t*>(p.visible) + s * (size_t)p.Np * 5;
  int32_t ax = 0, ay = 0;
  const bool robot_ok = vis_robot_cell(rx, ry, ox, oy, p.resolution, &ax, &ay);
  const auto occ = [&](int32_t x, int32_t y) {
    // transparent outside the world; there the load goes to cell (0, 0), which always exists, so that it needs no branch
    const bool inside = (uint32_t)x < (uint32_t)p.world_x && (uint32_t)y < (uint32_t)p.world_y;
    const size_t at = inside ? (size_t)y * (size_t)p.world_x + (size_t)x : 0;
    return inside & vis_occludes(p.occ, (uint32_t)world[at]);
  };
  int n_seen = 0;  // wave-uniform
  for (int base = 0; base < cnt; base += 64) {  // a chunk of up to 64 persons, one per lane
    const int j = base + (int)lane;
    const bool mine = j < cnt;
    uint32_t code = kSeenNotFinite, len = 0u, dims = 0u, dir = 0u;
    if (mine) {
      const double px = p.people[(s * (size_t)p.Np + (size_t)j) * 5], py = p.people[(s * (size_t)p.Np + (size_t)j) * 5 + 1];
      if (!robot_ok || !(vis_finite(px) && vis_finite(py))) code = kSeenNotFinite;
      else if (!vis_in_range(rx, ry, px, py, p.max_range)) code = kSeenOutOfRange;
      else {
        // in range of a robot with a cell: the person's cell is within 32769 cells of it (the host bounds max_range / resolution)
        const VisRay ray = vis_ray(ax, ay, (int32_t)vis_cell_axis(px, ox, p.resolution), (int32_t)vis_cell_axis(py, oy, p.resolution));
        code = kSeenSeen;
        len = ray.M;
        dims = ray.M | (ray.m << 16);  // both <= 32769 < 2^16
        dir = (uint32_t)(ray.ux + 1) | (uint32_t)(ray.uy + 1) << 2 | (uint32_t)(ray.vx + 1) << 4 | (uint32_t)(ray.vy + 1) << 6;
      }
    }
    // the rays' columns end to end: ray `lane` owns the columns start .. start + len - 1 of the list (<= 64 * 32769 entries)
    uint32_t incl = len;
    for (uint32_t d = 1u; d < 64u; d <<= 1) {
      const uint32_t below = vis_lane_read(incl, (lane - d) & 63u);
      if (lane >= d) incl += below;
    }
    const uint32_t start = incl - len, total = vis_lane_read(incl, 63u);
    uint64_t hits = 0ull;  // bit r: a column of ray r that this lane tested hides its person
    for (uint32_t t0 = 0u; t0 < total; t0 += 64u) {  // wave-uniform
      const uint32_t t = t0 + lane;
      uint32_t r = 0u;  // the last lane whose start is <= t: the ray that owns column t (rays without columns share a start with the next)
      for (uint32_t step = 32u; step != 0u; step >>= 1) {
        const uint32_t at = vis_lane_read(start, r + step);
        if (at <= t) r += step;
      }
      const uint32_t rstart = vis_lane_read(start, r), rdims = vis_lane_read(dims, r), rdir = vis_lane_read(dir, r);
      if (t < total) {
        VisRay ray;
        ray.ax = ax; ray.ay = ay;
        ray.ux = (int32_t)(rdir & 3u) - 1; ray.uy = (int32_t)((rdir >> 2) & 3u) - 1;
        ray.vx = (int32_t)((rdir >> 4) & 3u) - 1; ray.vy = (int32_t)((rdir >> 6) & 3u) - 1;
        ray.M = rdims & 0xFFFFu; ray.m = rdims >> 16;
        if (vis_column(ray, t - rstart, occ)) hits |= 1ull << r;
      }
    }
    for (uint32_t d = 1u; d < 64u; d <<= 1)
      hits |= (uint64_t)vis_lane_read((uint32_t)hits, lane ^ d) | (uint64_t)vis_lane_read((uint32_t)(hits >> 32), lane ^ d) << 32;
    if (code == kSeenSeen && ((hits >> lane) & 1ull) != 0ull) code = kSeenHidden;
    const bool is_seen = mine && code == kSeenSeen;
    const uint64_t seen_mask = __ballot(is_seen);
    if (is_seen) {
      const size_t slot = (size_t)n_seen + (size_t)__builtin_popcountll(seen_mask & ((1ull << lane) - 1ull));  // slot <= j: in the robot's rows
      uint64_t row[5];  // all five loads before the first store: `visible` is not known to be apart from `people`
      for (int c = 0; c < 5; ++c) row[c] = rows[(size_t)j * 5 + c];
      for (int c = 0; c < 5; ++c) out[slot * 5 + c] = row[c];
    }
    if (mine && p.seen) p.seen[s * (size_t)p.Np + (size_t)j] = (uint8_t)code;
    n_seen += __builtin_popcountll(seen_mask);
  }
  if (lane == 0u) p.visible_count[s] = n_seen;
}

}  // namespace smpc
