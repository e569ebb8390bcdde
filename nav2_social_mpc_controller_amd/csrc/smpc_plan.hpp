// smpc_plan.hpp — what a launch of the sweep kernels (solve, K1) and of the staging pass will be, decided once per call
// by pure host functions: the slot width, the kernel variant, fixed shape or not, stage-at-fetch or not, the helper lanes
// and the LDS bytes. No kernel, no HIP runtime call: a host-only program can print plans (tests/test_sweep_plan.py). The
// host code that issues the launch (smpc_sweep_host.hpp) maps a plan to the kernel function and sizes the grid, which needs
// the device.
#pragma once

#include <cstddef>
#include <cstdlib>

#include "smpc_launch.hpp"

namespace smpc {

// The experiment / test knobs of the environment. Read at every ABI call that launches or answers a query (the tests
// change them between the calls of one process), once per call, and nowhere else.
struct Knobs {
  bool no_helpers = false;    // SMPC_NO_HELPERS: hp_A = N, and no fixed-shape kernel (a fixed shape folds hp_A in); the LDS
                              // layout keeps the helper regions
  int solve_width = 0;        // SMPC_SOLVE_WIDTH = 32 | 64: the slot width of a solve of a shape that fits two scenes per wave
  int lone_waves_per_cu = 8;  // SMPC_LONE_WAVES_PER_CU >= 1: waves per CU of a solve launch sized for having the GPU to itself
  int max_waves_per_cu = 0;   // SMPC_MAX_WAVES_PER_CU >= 1: limit on the resident waves per CU a solve launch counts on
  int prio_step = 0;          // SMPC_PRIO_STEP >= 1: KParams::prio_step
  bool full_gram = false;     // SMPC_FULL_GRAM: KParams::full_gram
  bool debug_grid = false;    // SMPC_DEBUG_GRID: a solve launch reports its LDS bytes and waves per CU on stderr and, once it has
                              // finished, its trips: all, those with one slot idle for good, those that took the helped loop
  bool no_lone_help = false;  // SMPC_NO_LONE_HELP: KParams::lone_trips without kLoneHelp, every trip of a solve is paired
};

inline Knobs read_knobs() {
  Knobs kn;
  const auto number = [](const char* name) { const char* v = std::getenv(name); return v ? std::atoi(v) : 0; };
  kn.no_helpers = std::getenv("SMPC_NO_HELPERS") != nullptr;
  if (const int c = number("SMPC_SOLVE_WIDTH"); c == 32 || c == 64) kn.solve_width = c;
  if (const int c = number("SMPC_LONE_WAVES_PER_CU"); c >= 1) kn.lone_waves_per_cu = c;
  if (const int c = number("SMPC_MAX_WAVES_PER_CU"); c >= 1) kn.max_waves_per_cu = c;
  if (const int c = number("SMPC_PRIO_STEP"); c >= 1) kn.prio_step = c;
  kn.full_gram = std::getenv("SMPC_FULL_GRAM") != nullptr;
  kn.debug_grid = std::getenv("SMPC_DEBUG_GRID") != nullptr;
  kn.no_lone_help = std::getenv("SMPC_NO_LONE_HELP") != nullptr;
  return kn;
}

// Eval: K1. Trace (smpc_solve_trace_batch): the solve that also leaves a row per LM iteration, compiled for the most
// general variant only, kVT = kSP = true. A batch without T_scene runs it as it is (the kernel takes T for every scene),
// one without scene_params with the handle's own weights and bounds as every scene's row (neutral_rows()): both give the
// plain kernels' results bit for bit.
enum class Sweep { Eval, Solve, Trace };

// The parameter-block counts the library has kernels for.
constexpr bool nb_has_kernels(int nb) {
#ifdef SMPC_ONLY_NB  // development builds: one instantiation only (seconds instead of a minute to compile)
  return nb == SMPC_ONLY_NB;
#else
  return nb >= 1 && nb <= SMPC_MAX_BLOCKS;
#endif
}

// What the plan is made from: the call's shape (CH, bl, nb as smpc_dims() reports them), what the batch brings, and the
// handle's part (CUs of its device, smpc_set_solve_share, smpc_set_fixed_shapes).
struct SweepShape {
  Sweep kind;
  int B, T, N, CH, bl, nb;
  bool has_T_scene, has_scene_params;  // smpc_scene_batch.T_scene / .scene_params
  int num_cu, share;
  bool fixed_shapes;
};

struct SweepPlan {
  Sweep kind;
  int nb;
  int W, S;             // slot width, and the 64 / W scenes of a wave
  // vt: the kernel reads T, CH, bl of each scene from LDS instead of taking them as launch constants (the batch carries a
  // horizon per scene). sp: kSP, weights and bounds per scene, which reads the horizon per scene as well (T_scene or T).
  bool vt, sp, trace;
  int fixed;            // index in SMPC_FIXED_SHAPES of the shape whose kernels the launch runs, or -1
  bool stages;          // the kernel stages each scene's people block itself at the scene fetch: no staging pass ahead of it
  int hp_A;             // KParams::hp_A
  LdsLayout L;          // of one slot
  size_t shmem;         // dynamic LDS bytes of a wave
};

// Slot width of a solve launch. A shape that fits two scenes per wave (W = 32) still runs ONE scene per wave while the
// batch is small: up to one scene per SIMD (4 x CUs), two scenes in the lockstep of one wave only make each other wait
// (their LM phases differ from trip to trip; measured 4-17 % slower than a wave each, with bit-identical results); and
// where the W = 64 kernel's helper lanes pay (helper_owner_agents(): the 64 - T lanes beyond the horizon take over half
// of every step's agent list), up to the number of waves a lone launch takes anyway (8 per CU): every sweep of every
// scene is shorter then — the plugin's own call (B = 1, 8 people) 1.24 -> 1.06 ms, 1024 scenes 1.60 -> 1.13 ms, equal at
// 2048 (tools/gpu_width.py). Decided by the shape of the batch alone (B, T, N, the handle's share): a scene's result
// never depends on timing. With helper lanes it differs from the W = 32 kernel's in the last bits (the order of the
// sums over the agents).
inline int solve_slot_width(const SweepShape& k, const Knobs& kn) {
  if (slot_width(k.T, k.N) == 64) return 64;
  if (kn.solve_width) return kn.solve_width;
  const int share = k.share > 1 ? k.share : 1;
  const bool helpers_pay = helper_owner_agents(k.T, k.N, 64) < k.N;
  const int per_cu = helpers_pay ? kn.lone_waves_per_cu : 4;
  return (k.B <= per_cu * k.num_cu / share) ? 64 : 32;
}

// Whether the solve kernel of shape `index` of SMPC_FIXED_SHAPES stages at the scene fetch (K1 never does).
constexpr bool fixed_shape_stages(int index) {
  int i = 0;
#define SMPC_X(t, n, ch, b) \
  if (index == i++) return FixedShape<t, n, ch, b>::kStageAtFetch;
  SMPC_FIXED_SHAPES(SMPC_X)
#undef SMPC_X
  return false;
}

inline SweepPlan plan_sweep(const SweepShape& k, const Knobs& kn) {
  const bool eval = k.kind == Sweep::Eval;
  SweepPlan p;
  p.kind = k.kind;
  p.nb = k.nb;
  p.W = eval ? slot_width(k.T, k.N) : solve_slot_width(k, kn);
  p.S = kWave / p.W;
  p.trace = k.kind == Sweep::Trace;
  p.sp = p.trace || k.has_scene_params;
  p.vt = p.trace || k.has_T_scene;
  // The kernels of a shape of SMPC_FIXED_SHAPES: T, N, CH, bl as literals instead of launch values, the same results bit
  // for bit. They stand in for the plain instantiation <NB, W, false, false> only: a launch with a horizon or parameters
  // per scene, a trace, or the other slot width (the one-scene-per-wave kernel of a small batch; a shape's kernels are
  // compiled for its FixedShape::kW = slot_width(T, N)) runs the run-time-shape kernel it always ran. And none at all
  // with smpc_set_fixed_shapes(0) or under SMPC_NO_HELPERS, which works through the launch value hp_A that a fixed shape
  // folds in.
  p.fixed = -1;
  if (k.fixed_shapes && !kn.no_helpers && !p.vt && !p.sp && p.W == slot_width(k.T, k.N) && nb_has_kernels(k.nb))
    p.fixed = smpc::fixed_shape_index(k.T, k.N, k.CH, k.bl);
  p.stages = k.kind == Sweep::Solve && fixed_shape_stages(p.fixed);
  p.hp_A = kn.no_helpers ? k.N : helper_owner_agents(k.T, k.N, p.W);
  const int P = 2 * k.nb;
  p.L = make_layout(k.T, k.N, P, eval ? kLayoutEval : kLayoutSolve, p.W, p.sp);
  // behind the slot blocks: the feasibility rows of every slot (solve) or the row staging blocks + parked sensitivities (K1)
  const size_t extra = eval ? (size_t)eval_extra_doubles(k.T, P, p.W) : (size_t)wave_extra_doubles(P, p.W);
  // ... and behind those the wave's copy of the arctangent's node table
  p.shmem = ((size_t)atan_tab_offset(p.S * p.L.total, (int)extra) + kAtanTabDoubles) * sizeof(double);
  return p;
}

// The staging pass (smpc_stage_kernel<W>): the people block of a scene in LDS on its way to the staged records.
struct StagePlan { int W, S; LdsLayout L; size_t shmem; };

inline StagePlan plan_stage(int T, int N) {
  StagePlan p;
  p.W = slot_width(T, N);
  p.S = kWave / p.W;
  p.L = make_layout(T, N, 2, kLayoutStage, p.W);
  p.shmem = (size_t)p.S * p.L.total * sizeof(double);
  return p;
}

}  // namespace smpc
