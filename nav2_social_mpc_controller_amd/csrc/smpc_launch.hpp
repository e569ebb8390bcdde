// smpc_launch.hpp — what a launch of the sweep kernels (solve, K1, staging) is made of, for the host code that sizes and
// issues it and for the kernels alike: the launch-parameter struct KParams, the lane mapping's constants, and the LDS
// carve-up of a slot with the sizing functions behind it. Host and device; no device builtins.
//
// Lane mapping: a 64-lane wavefront is split into S = 64/W "slots" of W lanes (W = 32 when T+1 <= 32, else 64);
// each slot works on its own scene, lane `sl` of a slot owns horizon step t = sl (pose after t+1 steps) for every
// critic, and walks the N agents of that step in a register-resident loop (no cross-lane traffic for the social
// terms). The horizon's cos/sin block and the staged people block live in LDS; per-step reductions over the slot
// use wavefront shuffles.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/smpc.h"
#include "smpc_math.hpp"

namespace smpc {

constexpr int kWave = 64;
constexpr double kNoTarget = 1e300;  // agent-angle tag: no steering target at this step
constexpr int kSoc = 15;  // sum F(2), sum dF/d{x,y,th,v}(8), sum |G|^2 (1), sum d|G|^2/d{x,y,th,v} (4)

typedef double v4d __attribute__((ext_vector_type(4)));  // one staged people record (px, py, vx, vy): 32 bytes, moved whole
typedef double v2d __attribute__((ext_vector_type(2)));

struct KParams {
  int B, T, N, CH, bl, nb, P, nbounded, nfeas;
  int size_x, size_y, costmap_shared;
  double dt, resolution;
  double inv_resolution;  // 1 / resolution, rounded once on the host
  smpc_params prm;
  const double* pose0;
  const double* init_params;
  const double* path_pts;
  const double* goal_yaw;
  const double* people;
  const uint8_t* has_people;
  const int32_t* T_scene;  // [B] rollout steps of each scene (<= T), or null: every scene has T (smpc_scene_batch.T_scene)
  const uint8_t* costmap;
  const double* costmap_origin;
  // solve outputs
  double* o_params;
  double* o_cmds;
  double* o_path;
  int32_t* o_status;
  int32_t* o_reason;
  int32_t* o_iterations;
  int32_t* o_evaluations;
  double* o_initial_cost;
  double* o_final_cost;
  int* queue;  // [kQueueWords]: [0] the scene work queue, zeroed before every solve launch; behind it what the kernels with
               // lone trips count (lone_trip_kernel()): [1] trips with exactly one slot idle for good, [2] all trips,
               // [3] the trips of [1] that took the helped agent loop — counted (kLoneCount) and zeroed only by a
               // launch under SMPC_DEBUG_GRID, which reports them
  // staged people block (smpc_stage_people_batch / the library's own staging pass): what the sweep reads
  const double* people_rec;  // [B][N][T][4]  px, py, vx, vy of people_proj[t + 1][a]
  const double* people_aux;  // [B][T][2]     bit mask of valid agents (u64 bits), agent-angle target (kNoTarget: none)
  const int32_t* order;      // [B] queue order of the solve kernel (null: index order)
  int hp_A;                  // helper lanes (W = 64 kernels, see sweep()): agents the owner lane of a step walks itself;
                             // == N: no helpers. Agents hp_A .. N-1 of every step are walked by the lanes beyond the horizon
  int full_gram;             // != 0: every sweep of a solve forms the whole Gram (SMPC_FULL_GRAM: the check that stopping at
                             // its last column changes nothing)
  int prio_step;             // > 0: a wave whose oldest scene has made n sweeps runs at wave priority min(n / prio_step, 3)
  int lone_trips;            // LoneTripBits. kLoneHelp: a trip with one slot idle for good is a lone trip, its idle half
                             // evaluates every other agent (sweep()); without it (SMPC_NO_LONE_HELP) every trip is paired.
                             // Results are the same bit for bit. kLoneCount (SMPC_DEBUG_GRID): the launch counts its trips
                             // into queue[1..3]; without it no trip pays for the counting and those words are left alone
  double* stage_rec;         // staging kernel outputs (same layouts)
  double* stage_aux;
  unsigned long long* stamps;  // diagnostic builds only (SMPC_STAMPS): per-wave cycle sums per phase, [grid][8]
  // eval (K1) inputs / outputs
  const double* e_x;
  double* e_residuals;
  double* e_jacobian;
  double* e_cost;
  double* e_gradient;
  int e_M;  // row stride of the eval outputs (M with people)
  int e_row_order;  // 0: reference (step-major) row order, 1: critic-major (smpc_eval_batch_out.row_order)
  MathTab mt;  // polynomial coefficients of smpc_math.hpp, read through scalar loads
  AtanNodeTab an;  // nodes of atan2_unit(), copied into LDS by every wave (load_atan_nodes)
  const smpc_scene_params* scene_params;  // [B] per-scene weights / bounds (smpc_scene_batch.scene_params): the sp kernels
  // trace kernels only (smpc_solve_trace_batch, kTrace)
  double* o_trace;      // [B][trace_rows][kTraceCols] one row per LM iteration; rows >= trace_rows are not stored
  int32_t* o_trace_n;   // [B] rows the solve produced (may exceed trace_rows), or null
  int trace_rows;
  // kernels that stage at the scene fetch only (Shape::kStageAtFetch; smpc_solve_fixed_kernel)
  int stage_at_fetch;   // != 0: people_rec / people_aux hold nothing yet. The slot that fetches a scene turns its people
                        // block (`people`) into records at stage_rec, masks and tags in its LDS (load_scene()); no
                        // staging kernel ran and stage_aux is not used. 0: people_rec / people_aux are read as staged
};
constexpr int kTraceCols = SMPC_TRACE_COLS;
constexpr int kQueueWords = 4;  // KParams::queue
enum LoneTripBits { kLoneHelp = 1, kLoneCount = 2 };  // KParams::lone_trips

// The solve kernels that know lone trips (sweep(), kLone): two scenes per wave, launch-constant horizon and weights, no
// trace. Every other kernel is compiled without a line of it.
__host__ __device__ constexpr bool lone_trip_kernel(int W, bool vt, bool sp, bool trace) { return W == 32 && !vt && !sp && !trace; }

// Kernel parameters are read through the kernel-argument segment (constant address space) instead of being held in
// SGPRs for the whole kernel: the ~90 scalars of KParams otherwise overflow the SGPR file and come back as
// v_readlane / v_writelane spill traffic on the VALU (1.4 k such instructions in the solve kernel before).
typedef const KParams __attribute__((address_space(4))) * KParamsK;

constexpr int kSensInRegsMaxBlocks = 6;  // K1 keeps a lane's sensitivities in registers up to this many parameter blocks
// doubles of wave-shared LDS of the K1 kernel: two row staging blocks per slot, and the parked sensitivities
__host__ __device__ constexpr int eval_extra_doubles(int T, int P, int W) {
  return (64 / W) * (2 * T * P) + (P / 2 > kSensInRegsMaxBlocks ? (64 / W) * (5 * (P / 2) * W) : 0);
}
// The node table of atan2_unit() sits behind everything else in a wave's LDS (solve and K1 kernels).
__host__ __device__ constexpr int atan_tab_offset(int slot_doubles, int extra_doubles) { return (slot_doubles + extra_doubles + 3) & ~3; }
constexpr int kAtanTabDoubles = kAtanNodes * kAtanNodeStride;
// Cross-lane sum of the per-lane Gram shares (solve kernel): values go through LDS in chunks of whole columns of the
// packed upper triangle, at most kGramChunk values at a time; lane (part, v) of a slot then adds up value v of the 16
// lanes of its part and the parts are combined by shuffles (W / 16 + 3 additions instead of 3 log2(W) shuffle
// instructions per value). The buffer (W rows of kGramChunk + 1 doubles) lies over the sweep's own temporaries — the
// cos / sin block and the scans are dead once the sensitivities are formed — plus a tail of its own; outside the
// sweep the same area holds the temporaries of the LM algebra.
constexpr int kGramChunk = 16;
__host__ __device__ constexpr int gram_red_doubles(int W) { return W * (kGramChunk + 1); }
// doubles of wave-shared LDS behind the per-slot blocks of the solve kernel: the feasibility rows of every slot
__host__ __device__ constexpr int wave_extra_doubles(int P, int W) {
  return (kWave / W) * ((P / 2 > 1 ? P / 2 - 1 : 1) * (P + 1));
}

// LDS carve-up (in doubles) of ONE slot.
struct LdsLayout {
  int ag;       // [N][T][4]  staged people block (px, py, vx, vy) — staging kernel only; the sweep reads the staged
                //            records from global memory (HBM once in K1, L2 on the later sweeps of a solve)
  int valid;    // [T]        bit a set = agent a valid at step t (64-bit words)
  int cs;       // [2][T+1]   cos, sin of theta_j, j = 0..T
  int inc;      // [4][T+1]   inclusive scans over j of cos, sin, j cos, j sin(theta_j) of the current sweep
  int cst;      // [8]        x0, y0, yaw0, goal_yaw, origin x, origin y, final point x, y
  int stepst;   // [4][T]     helper lanes only: robot x, y, velocity x, y at every step (what a pair evaluation needs of it)
  int part;     // [T][kPart] helper lanes only: the partial sums a helper hands to the owner lane of a step
  int hz;       // [4]        the scene's own horizon (kernels with per-scene T): ints T, CH, bl, last block, feasibility
                //            rows, bounded blocks
  int sp;       // [14]       sp kernels only: the scene's smpc_scene_params row (weights, target speed, bounds)
  int lanec;    // [3][T]     per step: path point x, y (path_pts[t+1]) and agent-angle target (kNoTarget = none)
  int lm;       // LM vectors / matrices / scalars
  int gram;     // [(P+1)^2] Gram [J r]^T [J r] of the latest sweep, dense and symmetric
  int scratch;  // polynomial scratch
  int total;
};

// kLayoutSolve: LM state in LDS. kLayoutEval: the stand-alone K1 kernel, a single sweep. kLayoutStage: the staging
// kernel, people block in LDS on its way to the staged records.
enum LayoutKind { kLayoutEval = 0, kLayoutSolve = 1, kLayoutStage = 2 };

constexpr int kPart = 18;  // 6 + 4 + 1 + 4 partial sums, nearest distance, its agent index, redo flag (+ 1 spare)

// Helper lanes. With one scene per wave (W = 64) the lanes beyond the horizon (64 - T of them) idle through the agent loop,
// the longest part of a sweep. They take over the tail of every step's agent list instead: the owner lane of step t walks
// agents 0 .. A-1, one helper walks agents A .. N-1 of step t (a "unit"), helper h taking the units h, h + R, h + 2R, ...
// (R = 64 - T helpers, U = ceil(T / R) units each) and handing the partial sums of each unit to its owner through LDS.
// A is the smallest count with U (N - A) <= A: owners and helpers then finish together after A iterations instead of N
// (BASELINE configs[4]: N = 16, T = 38 -> A = 11; params.yaml shape N = 3 -> A = 2). Returns N when helpers do not
// pay (each unit costs a flush of ~30 instructions, the hand-over another ~40 per step).
__host__ __device__ constexpr int helper_owner_agents(int T, int N, int W) {
  const int R = W - T;
  if (W != 64 || R < 1 || N < 2) return N;
  const int U = (T + R - 1) / R;
  const int A = (U * N + U) / (U + 1);            // ceil(U N / (U + 1))
  if (A >= N) return N;
  // instructions saved per sweep against the hand-over's, with a margin of two: measured, the params.yaml shape (N = 3:
  // one pair saved, two units flushed) gained nothing, BASELINE configs[4] (five pairs saved) 14 %
  return ((N - A) * 250 > 2 * (60 * U + 120)) ? A : N;
}

constexpr int kSceneParamDoubles = sizeof(smpc_scene_params) / sizeof(double);  // 14

// W: the slot width of the kernel the layout is for (32: two scenes per wave, 64: one; slot_width() / solve_slot_width())
// sp: the layout of the sp kernels (per-scene weights and bounds, smpc_scene_batch.scene_params): 14 doubles more per slot
__host__ __device__ inline LdsLayout make_layout(int T, int N, int P, int kind, int W, bool sp = false) {
  LdsLayout L;
  const bool with_lm = kind == kLayoutSolve;
  int o = 0;
  L.ag = o; if (kind == kLayoutStage) o += 4 * T * (N > 0 ? N : 1);
  L.valid = o; o += T;
  L.cs = o; o += 2 * (T + 1);
  L.inc = o; o += 4 * (T + 1);
  if (with_lm) {  // tail of the Gram reduction buffer / LM temporaries, which start at L.cs
    const int want = gram_red_doubles(W) > P * P + 7 * P + 96 ? gram_red_doubles(W) : P * P + 7 * P + 96;
    if (want > 6 * (T + 1)) o += want - 6 * (T + 1);
  }
  L.cst = o; o += 8;
  L.hz = o; o += 4;
  L.sp = o; if (sp) o += kSceneParamDoubles;
  L.stepst = o; L.part = o;
  if (kind != kLayoutStage && helper_owner_agents(T, N, W) < N) { o += 4 * T; L.part = o; o += kPart * T; }
  L.lanec = o; o += 3 * T;
  L.lm = o; if (with_lm) o += P * P + 6 * P + 24;  // Hs, six vectors, scalars: what lives from trip to trip
  L.gram = o; o += (P + 1) * (P + 1);  // dense symmetric [J r]^T [J r] of the latest sweep (VALU back-end)
  L.scratch = o;  // (the generic line-search interpolation fallback borrows the wave's Gram reduction buffer)
  L.total = (o + 3) & ~3;  // 32-byte multiple: records are moved as 4-double vectors
  return L;
}

__host__ __device__ constexpr int slot_width(int T, int N) { return (T + 1 <= 32 && N <= 32) ? 32 : 64; }

// ------------------------------------------------------------------------------------------------
// The shape of a launch: T, N, CH, bl and what follows from them (parameter blocks, feasibility rows, bounded blocks, the
// slot width, every offset of make_layout()). sweep(), load_scene(), get_horizon() and the kernel bodies take it as a
// template parameter and read it through these accessors, `k` being the launch parameters:
//   RuntimeShape      the launch values k.T, k.N, ... : a kernel for every shape (smpc_solve_kernel, smpc_eval_kernel)
//   FixedShape<...>   literals: the kernels of ONE shape (smpc_solve_fixed_kernel, smpc_eval_fixed_kernel). The values are
//                     the controller's configuration (control_horizon, parameter_block_length, max_time / time_step, the
//                     people cap), the same in every call of a handle's life; as constants they take no scalar registers,
//                     no scalar loads, no sign extensions, and the counts of the rollout are folded.
// Map size, resolution, dt, weights and bounds are launch values in both.
// ------------------------------------------------------------------------------------------------
struct RuntimeShape {
  static constexpr bool kFixed = false;
  static constexpr bool kStageAtFetch = false;  // its solve kernels read a people block the staging kernel has staged
  template <class K> __host__ __device__ static inline int T(const K& k) { return k.T; }
  template <class K> __host__ __device__ static inline int N(const K& k) { return k.N; }
  template <class K> __host__ __device__ static inline int CH(const K& k) { return k.CH; }
  template <class K> __host__ __device__ static inline int bl(const K& k) { return k.bl; }
  template <class K> __host__ __device__ static inline int nfeas(const K& k) { return k.nfeas; }
  template <class K> __host__ __device__ static inline int nbounded(const K& k) { return k.nbounded; }
  template <class K> __host__ __device__ static inline int hp_A(const K& k) { return k.hp_A; }
};

// CH_ and BL_ as smpc_dims() reports them: CH = min(control_horizon, T), bl = min(parameter_block_length, CH)
template <int T_, int N_, int CH_, int BL_> struct FixedShape {
  static_assert(T_ >= 1 && T_ + 1 <= kWave && N_ >= 0 && N_ <= kWave, "a shape the sweep kernels take");
  static_assert(CH_ >= 1 && CH_ <= T_ && BL_ >= 1 && BL_ <= CH_, "CH and bl are the clamped values of smpc_dims()");
  static constexpr bool kFixed = true;
  // The solve kernel of a fixed shape may stage a scene's people block itself where it fetches the scene, instead of a
  // staging kernel ahead of the launch (KParams::stage_at_fetch says whether a launch does; load_scene(), smpc_sweep.hpp).
  // A property of the kernel, so that the kernels of RuntimeShape carry no test for it. K1 never stages.
  static constexpr bool kStageAtFetch = true;
  static constexpr int kNB = (CH_ - 1) / BL_ + 1;     // parameter blocks
  static constexpr int kW = slot_width(T_, N_);       // the slot width its kernels are compiled for
  static constexpr int kNbounded = CH_ / BL_;                                         // src/optimizer.cpp:373
  static constexpr int kNfeas = (CH_ / BL_ < T_ ? CH_ / BL_ : T_) - 1 > 0 ? (CH_ / BL_ < T_ ? CH_ / BL_ : T_) - 1 : 0;  // :364
  template <class K> __host__ __device__ static constexpr int T(const K&) { return T_; }
  template <class K> __host__ __device__ static constexpr int N(const K&) { return N_; }
  template <class K> __host__ __device__ static constexpr int CH(const K&) { return CH_; }
  template <class K> __host__ __device__ static constexpr int bl(const K&) { return BL_; }
  template <class K> __host__ __device__ static constexpr int nfeas(const K&) { return kNfeas; }
  template <class K> __host__ __device__ static constexpr int nbounded(const K&) { return kNbounded; }
  template <class K> __host__ __device__ static constexpr int hp_A(const K&) { return helper_owner_agents(T_, N_, kW); }
};

// The shapes that have fixed-shape kernels: X(T, N, CH, bl), one line per shape. The host picks a shape's kernels when a
// launch has exactly these values and would otherwise run the plain <NB, W, false, false> instantiation of its slot width
// (fixed_shape_index() below is the rule; pick_fixed() in smpc_hip.hip maps its index to the kernels).
// (A shape whose slot width is 64 folds helper_owner_agents() in as well: the host takes no fixed-shape kernel while the
// experiment knob SMPC_NO_HELPERS, which works through the launch value hp_A, is set.)
#define SMPC_FIXED_SHAPES(X) \
  X(28, 8, 18, 6) /* the headline configuration: H18 / bl6 at T = 28 with 8 people -> NB = 3, W = 32 */

// index of (T, N, CH, bl) in SMPC_FIXED_SHAPES, or -1
__host__ __device__ constexpr int fixed_shape_index(int T, int N, int CH, int bl) {
  int i = 0;
#define SMPC_X(t, n, ch, b) \
  if (T == (t) && N == (n) && CH == (ch) && bl == (b)) return i; \
  ++i;
  SMPC_FIXED_SHAPES(SMPC_X)
#undef SMPC_X
  return -1;
}

}  // namespace smpc
