// smpc_solve_kernel.hpp — the solve kernel: the per-slot Levenberg-Marquardt state machine (the ceres::Solve call of
// reference src/optimizer.cpp:381, options :117-131) and the post-solve unpack (src/optimizer.cpp:390-446).
//
// A wave is a persistent "sweep engine": every trip of the main loop runs ONE sweep() for all slots of the wave
// at each slot's current trial point, then each slot advances its own LM state (phases of smpc_lm.hpp) and produces its
// next trial point, or finishes its scene and pulls the next one from the global scene queue. Slots never wait for
// each other: iteration counts and line-search lengths differ per scene, the sweep is the only shared code.
// Every LM quantity is uniform across the W lanes of a slot (computed redundantly, LM vectors parked in LDS).
#pragma once

#include "smpc_lm.hpp"
#include "smpc_sweep.hpp"

namespace smpc {

// waves per SIMD the solve kernel's register allocation must allow: three for the two-scenes-per-wave kernels up to three
// parameter blocks (the headline shapes sit at 160-168 registers; stated so that an edit cannot silently cost the third
// wave, which is what overlapped launches of several streams live on), two otherwise — the one-scene-per-wave kernels
// serve small batches (the plugin's own B = 1 call) and long horizons, whose launches take at most eight waves per CU,
// and their helper-lane loop needs the registers (held to 168 it spilled 14)
#ifndef SMPC_SOLVE_MIN_WAVES
#define SMPC_SOLVE_MIN_WAVES(NB, W) (((NB) <= 3 && (W) == 32) ? 3 : 2)
#endif
// The LM vectors and matrices of a slot are spread over its lanes: lane q < P owns parameter q (its entry of x, of the
// trial point, of the step, row q of the scaled Gram and of its Cholesky factor). One instruction then updates all P
// entries; sums over the parameters go through a few LDS words in index order (the same order a serial loop would
// add them in). Nothing P x P lives in registers, so the P = 8..12 instantiations do not spill.
//
// One template, five parameters: smpc_solve_kernel<NB, W, kVT, kSP, kTrace>. NB parameter blocks, W lanes per scene slot.
// Without kSP the handle's weights and bounds are launch constants; with it every scene brings its own row of
// smpc_scene_params (kept in the slot's LDS, see load_scene() and SMPC_SCENE_PRM) and the horizon is always read per scene
// (kVT; T for every scene when the batch gives no T_scene). kTrace (smpc_solve_trace_batch; the most general variant only,
// kVT = kSP = true): the solve also leaves one row of kTraceCols doubles per LM iteration in k.o_trace, in the format and
// by the rules of the oracle's Minimizer::Run (TraceRow): row 0 behind the initial evaluation, row i where iteration i
// ends (accepted, rejected, invalid step, parameter / function tolerance), none where the solve ends before ++iteration
// or without a row in the oracle. The row index is the iteration number. Every value of a row is uniform over the slot:
// lane j < 9 of the slot stores column j. Without kTrace the `if constexpr (kTrace)` blocks leave nothing behind.
// Variants of this kernel are template parameters, never a device function the kernel calls: behind a function boundary,
// always_inline included, the compiler optimises the body once on its own before inlining it, which changes the register
// assignment and instruction order of the existing instantiations. tools/isa_identity.py compares the machine code of
// two trees function by function: run it on any edit that is meant to leave the generated code as it is.
template <int NB, int W, bool kVT = false, bool kSP = false, bool kTrace = false>
__global__ __launch_bounds__(64, SMPC_SOLVE_MIN_WAVES(NB, W)) void smpc_solve_kernel(const KParams) {
  using Shape = RuntimeShape;
#include "smpc_solve_body.inc"
}

// The solve kernel of one shape of SMPC_FIXED_SHAPES (smpc_launch.hpp): <Shape::kNB, Shape::kW, false, false, false> with
// T, N, CH, bl and everything derived from them as literals. A kernel template of its own beside smpc_solve_kernel, whose
// instantiations keep their names and their code; the body is the same text.
template <class Shape>
__global__ __launch_bounds__(64, SMPC_SOLVE_MIN_WAVES(Shape::kNB, Shape::kW)) void smpc_solve_fixed_kernel(const KParams) {
  static_assert(Shape::kFixed, "smpc_solve_fixed_kernel<FixedShape<T, N, CH, bl>>");
  constexpr int NB = Shape::kNB, W = Shape::kW;
  constexpr bool kVT = false, kSP = false, kTrace = false;
#include "smpc_solve_body.inc"
}

}  // namespace smpc
