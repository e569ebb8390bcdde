// smpc_stage.hpp — the staging pass: the people block of the reference layout turned into the records, valid masks and
// agent-angle tags the sweep reads (stage_people), and the kernel that runs it once per people block.
#pragma once

#include "smpc_sweep.hpp"

namespace smpc {

// Staging pass (its own kernel, once per people block): gather the slot's people block, agent index fastest across
// lanes (coalesced runs of one people row, 16 loads in flight per lane), convert to one 32-byte record (px, py, vx, vy)
// per (agent, step) at record index a * T + t in LDS (ag), and compute per step the bit mask of valid agents (vmask)
// and the agent-angle tag (aa). Executed by all W lanes of the slot.
template <int W>
__device__ inline void stage_people(KParamsK kp, int scene, int sl, double* ag, unsigned long long* vmask, double* aa) {
  const auto& k = *kp;
  const int T = k.T, N = k.N;
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

// Staging pass: people block of the reference layout ([T+1][6][N] per scene) -> the records the sweep reads
// ([N][T] x (px, py, vx, vy), written as whole 128-byte lines through LDS) + per-step valid mask and agent-angle tag.
// One slot per scene like the sweep kernels; once per people block (a solve re-reads the records ~50 times).
template <int W>
__global__ __launch_bounds__(64) void smpc_stage_kernel(const KParams) {
  SMPC_CHAIN_PRIORITY();
  const auto& k = *(KParamsK)__builtin_amdgcn_kernarg_segment_ptr();
  constexpr int S = kWave / W;
  extern __shared__ __attribute__((aligned(32))) double lds_all[];
  const int lane = threadIdx.x & 63;
  const int slot = lane / W, sl = lane - slot * W;
  const int T = k.T, N = k.N;
  const LdsLayout L = make_layout(T, N, 2, kLayoutStage, W);
  double* lds = lds_all + (size_t)slot * L.total;
  const int scene_raw = blockIdx.x * S + slot;
  const bool live = scene_raw < k.B;
  const int scene = live ? scene_raw : k.B - 1;
  const bool has_people = k.has_people ? k.has_people[scene] != 0 : true;
  double* ag = lds + L.ag;
  unsigned long long* vmask = reinterpret_cast<unsigned long long*>(lds + L.valid);
  double* aa = lds + L.lanec;
  if (has_people) stage_people<W>(&k, scene, sl, ag, vmask, aa);
  wave_lds_fence();
  if (live && has_people) {
    const size_t s = scene;
    const int nrec = N * T;
    v4d* dst = reinterpret_cast<v4d*>(k.stage_rec + s * (size_t)4 * nrec);
    const v4d* src = reinterpret_cast<const v4d*>(ag);
    for (int q = sl; q < nrec; q += W) dst[q] = src[q];  // consecutive lanes, consecutive 32-byte records
    if (sl < T) {
      double* aux = k.stage_aux + (s * T + sl) * 2;
      aux[0] = (lds + L.valid)[sl];
      aux[1] = aa[sl];
    }
  }
}

}  // namespace smpc
