// smpc_eval_kernel.hpp — smpc_eval_kernel, the stand-alone K1 kernel around sweep().
#pragma once

#include "smpc_sweep.hpp"

namespace smpc {

// K1 stand-alone: one sweep per scene at given parameters, rows written to HBM (parity checks, roofline runs).
// Up to three parameter blocks the sweep fits the 168 registers that three waves per SIMD allow (the headline shapes;
// K1 is a latency-bound streaming kernel, the third wave is worth 20 % of its time); beyond that the row buffers grow
// with P and the allocator is left alone.
#ifndef SMPC_EVAL_MIN_WAVES
#define SMPC_EVAL_MIN_WAVES(NB) ((NB) <= 3 ? 3 : 1)
#endif
// smpc_eval_kernel<NB, W, kVT, kSP>: the variants are template parameters, as for the solve kernel (smpc_solve_kernel.hpp).
template <int NB, int W, bool kVT = false, bool kSP = false>
__global__ __launch_bounds__(64, SMPC_EVAL_MIN_WAVES(NB)) void smpc_eval_kernel(const KParams) {
  using Shape = RuntimeShape;
#include "smpc_eval_body.inc"
}

// K1 of one shape of SMPC_FIXED_SHAPES (smpc_launch.hpp): <Shape::kNB, Shape::kW, false, false> with T, N, CH, bl as
// literals, beside smpc_eval_kernel like smpc_solve_fixed_kernel beside smpc_solve_kernel.
template <class Shape>
__global__ __launch_bounds__(64, SMPC_EVAL_MIN_WAVES(Shape::kNB)) void smpc_eval_fixed_kernel(const KParams) {
  static_assert(Shape::kFixed, "smpc_eval_fixed_kernel<FixedShape<T, N, CH, bl>>");
  constexpr int NB = Shape::kNB, W = Shape::kW;
  constexpr bool kVT = false, kSP = false;
#include "smpc_eval_body.inc"
}

}  // namespace smpc
