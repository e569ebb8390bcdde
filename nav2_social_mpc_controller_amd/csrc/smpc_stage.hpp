// smpc_stage.hpp — the staging pass: the people block of the reference layout turned into the records, valid masks and
// agent-angle tags the sweep reads (stage_people). Two callers, one text: the staging kernel (smpc_stage_kernel.hpp), once
// per people block ahead of a launch, and load_scene() of a solve kernel that stages at the scene fetch (smpc_sweep.hpp).
// Host and device: tests/native/stage_shim.hip runs it lane by lane on the host.
#pragma once

#include "smpc_launch.hpp"
#include "smpc_math.hpp"

namespace smpc {

// Gather the slot's people block, agent index fastest across lanes (coalesced runs of one people row, 16 loads in flight
// per lane), convert to one 32-byte record (px, py, vx, vy) per (agent, step) at record index a * T + t of `ag` (the
// staging kernel: LDS; at the scene fetch: the scene's records in global memory), and compute per step the bit mask of
// valid agents (vmask) and the agent-angle tag (aa). Executed by all W lanes of the slot.
// Shape: T and N as launch values or literals (smpc_launch.hpp). KP: the launch parameters where the caller has them.
template <int W, class Shape = RuntimeShape, class KP = KParamsK>
__host__ __device__ inline void stage_people(KP kp, int scene, int sl, double* ag, unsigned long long* vmask, double* aa) {
  const auto& k = *kp;
  const int T = Shape::T(k), N = Shape::N(k);
  const size_t s = scene;
  const double x0 = k.pose0[3 * s], y0 = k.pose0[3 * s + 1], yaw0 = k.pose0[3 * s + 2];
  const double* ppl = k.people + s * (size_t)(T + 1) * 6 * N;
  const int TN = T * N;
  // people_proj[t+1] field f agent a is at ((t+1)*6 + f)*N + a. Element (a, t) lands at a*T + t.
  for (int e0 = sl; e0 < TN; e0 += 4 * W) {
    double gx[4], gy[4], gyaw[4], glv[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int e = min(e0 + u * W, TN - 1);
      const int t = e / N, a = e - t * N;
      const double* f = ppl + (size_t)(t + 1) * 6 * N + a;
      gx[u] = f[0]; gy[u] = f[N]; gyaw[u] = f[2 * N]; glv[u] = f[4 * N];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int e = e0 + u * W;
      if (e < TN) {
        const int t = e / N, a = e - t * N;
        double sn, cs;
        if (__builtin_expect(!(fabs(gyaw[u]) <= 1e5), 0)) sincos(gyaw[u], &sn, &cs);
        else sincos_tab(&k.mt, gyaw[u], &sn, &cs);
        const int q = a * T + t;
        v4d rec = {gx[u], gy[u], glv[u] * cs, glv[u] * sn};  // aVel, social_work:187-188
        reinterpret_cast<v4d*>(ag)[q] = rec;
      }
    }
  }
  if (sl < T) {
    const double* f = ppl + (size_t)(sl + 1) * 6 * N;
    unsigned long long m = 0;
    double aa_target = kNoTarget;
    // a7 AgentAngle tag: depends on constants only (critics/agent_angle_cost_function.hpp:130-190)
    int closest = -1;
    double best = INFINITY;
    for (int a0 = 0; a0 < N; a0 += 4) {  // loads of four agents in flight at a time
      double ft[4], fx[4], fy[4], fl[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int a = min(a0 + u, N - 1);
        ft[u] = f[3 * N + a]; fx[u] = f[a]; fy[u] = f[N + a]; fl[u] = f[4 * N + a];
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int a = a0 + u;
        if (a < N) {
          if (ft[u] != -1.0) m |= (1ull << a);  // social_work:175
          const double ddx = fx[u] - x0, ddy = fy[u] - y0;
          const double d2 = ddx * ddx + ddy * ddy;
          if (d2 < best && fl[u] > 0.05) { best = d2; closest = a; }
        }
      }
    }
    if (closest >= 0 && !(best > 4.0)) {
      const double ax = f[closest], ay = f[N + closest], ayaw = f[2 * N + closest];
      const double agent_angle_initial = atan2(ay - y0, ax - x0);
      // atan2(sin u, cos u) of the reference (:148-152) restated as the range reduction wrap_angle(u)
      const double heading_diff = wrap_angle(ayaw - yaw0);
      const double rel = wrap_angle(agent_angle_initial - yaw0);
      const double kThr = M_PI / 6.0, kUp = 5 * M_PI / 6.0;
      if (heading_diff <= -kUp || heading_diff >= kThr) {
        if (!(rel < 0.0)) aa_target = yaw0 + (-(M_PI / 6.0));
      } else {
        if (!(rel > 0.0)) aa_target = yaw0 + (M_PI / 6.0);
      }
    }
    vmask[sl] = m;
    aa[sl] = aa_target;
  }
}

}  // namespace smpc
