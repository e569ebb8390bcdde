// smpc_metrics.hpp — per-robot navigation metrics of a closed-loop episode (smpc_episode_metrics_batch): one launch
// folds one sample of the world state (robot pose and executed twist, people, clearance grid, the tick's solve status and
// command source) into a row of SMPC_METRIC_COLS doubles per robot. Persons go across lanes: a robot owns G = next power
// of two >= Np lanes, 64 / G robots share a wavefront. The minimum distance and the force sums over a robot's persons
// are xor-butterflies over its G lanes (lanes without a person contribute +inf / 0), so their order is a function of
// Np alone. Lane 0 of the group reads, updates and writes the row; a row frozen at its goal is not written at all.
// The social work is SocialWorkCost's wr + wp (critics/social_work_cost_function.hpp:125-143) from one evaluation per
// pair with social_force_general(): libm exp / atan2, no tables, no LDS.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/smpc.h"
#include "smpc_math.hpp"
#include "smpc_social_force.hpp"

namespace smpc {

constexpr int kMetricsThreads = 256;

struct MetricsParams {
  int B, Np, G;  // G = lanes of one robot (power of two, Np <= G <= 64)
  int od_shared, od_width, od_height;
  float od_resolution;
  double dt, goal_tolerance, robot_radius, person_radius, intimate_radius, personal_radius, social_radius;
  const double* pose;    // [B][3]
  const double* twist;   // [B][2]
  const double* people;  // [B][Np][5]
  const int32_t* count;  // [B]
  const double* goal;    // [B][2] or null
  const float* od_distances;  // [B or 1][od_height][od_width] or null
  const double* od_origin;    // [B or 1][2]
  const int32_t* status;      // [B] or null
  const int32_t* source;      // [B] or null
  double* acc;                // [B][SMPC_METRIC_COLS]
};

__global__ __launch_bounds__(kMetricsThreads) void smpc_episode_metrics_kernel(const MetricsParams p) {
  SMPC_CHAIN_PRIORITY();
  const int G = p.G;
  const int tid = blockIdx.x * kMetricsThreads + threadIdx.x;
  const int robot = tid / G, g = tid - robot * G;
  const bool live = robot < p.B;  // the lanes behind the last robot stay for the shuffles and write nothing
  const size_t b = live ? robot : p.B - 1;
  const bool owner = live && g == 0;

  // the row and the robot's scalar inputs are requested first: they arrive while the pair term is evaluated
  double row[SMPC_METRIC_COLS];
  if (owner) {
#pragma unroll
    for (int c = 0; c < SMPC_METRIC_COLS; ++c) row[c] = p.acc[b * SMPC_METRIC_COLS + c];
  }
  const double x = p.pose[3 * b], y = p.pose[3 * b + 1], yaw = p.pose[3 * b + 2];
  const double v = p.twist[2 * b];
  const int cnt = min(max(p.count[b], 0), p.Np);
  bool on_grid = false;
  double clearance = 0.0;
  if (owner && p.od_distances) {
    const size_t grid = p.od_shared ? 0 : b;
    const double res = (double)p.od_resolution;
    const double cx = floor((x - p.od_origin[2 * grid]) / res), cy = floor((y - p.od_origin[2 * grid + 1]) / res);
    on_grid = cx >= 0.0 && cx < (double)p.od_width && cy >= 0.0 && cy < (double)p.od_height;  // NaN: off the grid
    if (on_grid)
      clearance = (double)p.od_distances[(grid * (size_t)p.od_height + (size_t)cy) * (size_t)p.od_width + (size_t)cx];
  }

  // ---- this lane's person: distance and the robot's pair term F (the force on the person from the robot alone is -F)
  const bool has = g < cnt;
  double dist = INFINITY, fx = 0.0, fy = 0.0, f2 = 0.0;
  if (has) {
    const double* q = p.people + (b * (size_t)p.Np + (size_t)g) * 5;
    double sn, cs;
    sincos(yaw, &sn, &cs);
    const double dx = x - q[0], dy = y - q[1];
    dist = sqrt(dx * dx + dy * dy);
    const Force F = social_force_general(dx, dy, v * cs - q[2], v * sn - q[3]);
    fx = F.fx; fy = F.fy;
    f2 = fx * fx + fy * fy;
  }
  for (int off = 1; off < G; off <<= 1) {
    dist = fmin(dist, __shfl_xor(dist, off, 64));
    fx += __shfl_xor(fx, off, 64);
    fy += __shfl_xor(fy, off, 64);
    f2 += __shfl_xor(f2, off, 64);
  }
  if (!owner) return;

  // ---- the row's read-modify-write
  if (row[SMPC_M_SAMPLES] == 0.0) {  // no samples yet: a zero-filled row is a reset
#pragma unroll
    for (int c = 0; c < SMPC_METRIC_COLS; ++c) row[c] = 0.0;
    row[SMPC_M_MIN_PERSON_DIST] = INFINITY;
    row[SMPC_M_MIN_CLEARANCE] = INFINITY;
    row[SMPC_M_TIME_TO_GOAL] = -1.0;
  } else if (row[SMPC_M_TIME_TO_GOAL] >= 0.0) {
    return;  // the goal was reached in an earlier call: the row stays as it is, bit for bit
  }
  if (row[SMPC_M_SAMPLES] > 0.0) {
    const double mx = x - row[SMPC_M_LAST_X], my = y - row[SMPC_M_LAST_Y];
    row[SMPC_M_PATH_LENGTH] += sqrt(mx * mx + my * my);
    row[SMPC_M_HEADING_CHANGE] += fabs(wrap_to_pi(yaw - row[SMPC_M_LAST_YAW]));
  }
  row[SMPC_M_SUM_SPEED] += v;
  if (cnt > 0) {
    row[SMPC_M_PEOPLE_SAMPLES] += 1.0;
    row[SMPC_M_MIN_PERSON_DIST] = fmin(row[SMPC_M_MIN_PERSON_DIST], dist);
    row[SMPC_M_SUM_MIN_PERSON_DIST] += dist;
    row[SMPC_M_INTIMATE_SAMPLES] += dist < p.intimate_radius ? 1.0 : 0.0;
    row[SMPC_M_PERSONAL_SAMPLES] += dist < p.personal_radius ? 1.0 : 0.0;
    row[SMPC_M_SOCIAL_SAMPLES] += dist < p.social_radius ? 1.0 : 0.0;
    row[SMPC_M_PERSON_COLLISION_SAMPLES] += dist < p.robot_radius + p.person_radius ? 1.0 : 0.0;
  }
  row[SMPC_M_SOCIAL_WORK] += (fx * fx + fy * fy) + f2;  // wr + wp
  if (p.od_distances) {
    if (on_grid) {
      row[SMPC_M_MIN_CLEARANCE] = fmin(row[SMPC_M_MIN_CLEARANCE], clearance);
      row[SMPC_M_OBSTACLE_COLLISION_SAMPLES] += clearance < p.robot_radius ? 1.0 : 0.0;
    } else {
      row[SMPC_M_OFF_GRID_SAMPLES] += 1.0;
    }
  }
  if (p.source) row[SMPC_M_FALLBACK_SAMPLES] += p.source[b] != 0 ? 1.0 : 0.0;
  if (p.status) {
    const int st = p.status[b];
    row[SMPC_M_UNUSABLE_SOLVES] += (st != SMPC_CONVERGENCE && st != SMPC_NO_CONVERGENCE) ? 1.0 : 0.0;
  }
  row[SMPC_M_LAST_X] = x; row[SMPC_M_LAST_Y] = y; row[SMPC_M_LAST_YAW] = yaw;
  row[SMPC_M_SAMPLES] += 1.0;
  if (p.goal) {
    const double gx = x - p.goal[2 * b], gy = y - p.goal[2 * b + 1];
    const double gd = sqrt(gx * gx + gy * gy);
    row[SMPC_M_GOAL_DIST] = gd;
    if (gd <= p.goal_tolerance) row[SMPC_M_TIME_TO_GOAL] = row[SMPC_M_SAMPLES] * p.dt;
  }
#pragma unroll
  for (int c = 0; c < SMPC_METRIC_COLS; ++c) p.acc[b * SMPC_METRIC_COLS + c] = row[c];
}

}  // namespace smpc
