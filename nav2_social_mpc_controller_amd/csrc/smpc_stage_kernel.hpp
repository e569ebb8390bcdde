// smpc_stage_kernel.hpp — the staging kernel: stage_people() (smpc_stage.hpp) once per people block, ahead of the launches
// that read the staged block (K1, every solve kernel that does not stage at the scene fetch, smpc_stage_people_batch).
#pragma once

#include "smpc_stage.hpp"
#include "smpc_sweep.hpp"

namespace smpc {

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
