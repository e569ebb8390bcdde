// smpc_probes.hpp — the two probe kernels behind smpc_math_probe and smpc_fp64_peak_probe.
#pragma once

#include "smpc_launch.hpp"
#include "smpc_lm.hpp"

namespace smpc {
struct ProbeParams { int fn, n; const double* a; const double* b; double* o0; double* o1; MathTab mt; AtanNodeTab an; };
__global__ void smpc_math_probe_kernel(const ProbeParams) {
  const auto& k = *(const ProbeParams __attribute__((address_space(4)))*)__builtin_amdgcn_kernarg_segment_ptr();
  __shared__ double atab[kAtanTabDoubles];  // the LDS copy of the nodes, as in the sweep kernels
  for (int j = threadIdx.x; j < kAtanTabDoubles; j += blockDim.x) atab[j] = k.an.v[j];
  __syncthreads();
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= k.n) return;
  const double a = (k.fn == 7) ? 0.0 : k.a[i], b = k.b ? k.b[i] : 0.0;
  double r0 = 0.0, r1 = 0.0;
  switch (k.fn) {
    case 0: r0 = exp_tab(&k.mt, a); break;
    case 1: r0 = atan2_dir(&k.mt, a, b); break;
    case 2: sincos_tab(&k.mt, a, &r0, &r1); break;
    case 3: r0 = rsqrt_pos(a); break;
    case 4: r0 = div_fast(a, b); break;
    case 5: r0 = rcp_estimate(a); break;
    case 8: r0 = atan2_unit(&k.mt, atab, a, b); break;
    case 7: {  // a = [c4 c3 c2 c1 c0 lo hi _] per problem: the line search's bracketed root finder, trips in out1
      const double q[5] = {k.a[8 * i], k.a[8 * i + 1], k.a[8 * i + 2], k.a[8 * i + 3], k.a[8 * i + 4]};
      int trips = 0;
      r0 = bracketed_root<4>(q, k.a[8 * i + 5], k.a[8 * i + 6], &trips);
      r1 = (double)trips;
      break;
    }
    default: r0 = rsq_estimate(a); break;
  }
  k.o0[i] = r0;
  if (k.o1) k.o1[i] = r1;
}
}  // namespace smpc

namespace smpc {
// FP64 vector peak probe (SURVEY §7 asks for the denominator of the FP64 roofline to be measured, not assumed):
// eight independent v_fma_f64 chains per lane, nothing else in the loop.
__global__ __launch_bounds__(256) void smpc_fp64_peak_kernel(double* out, int iters) {
  double a0 = 1.0 + threadIdx.x * 1e-9, a1 = a0 + 1e-9, a2 = a0 + 2e-9, a3 = a0 + 3e-9;
  double a4 = a0 + 4e-9, a5 = a0 + 5e-9, a6 = a0 + 6e-9, a7 = a0 + 7e-9;
  const double m = 0.999999999, c = 1e-9;
  for (int i = 0; i < iters; ++i) {
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      a0 = fma(a0, m, c); a1 = fma(a1, m, c); a2 = fma(a2, m, c); a3 = fma(a3, m, c);
      a4 = fma(a4, m, c); a5 = fma(a5, m, c); a6 = fma(a6, m, c); a7 = fma(a7, m, c);
    }
  }
  out[blockIdx.x * blockDim.x + threadIdx.x] = ((a0 + a1) + (a2 + a3)) + ((a4 + a5) + (a6 + a7));
}
}  // namespace smpc
