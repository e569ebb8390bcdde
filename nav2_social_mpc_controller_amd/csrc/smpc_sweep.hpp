// smpc_sweep.hpp — the residual/Jacobian sweep of the batched social-MPC solver (the body of K1 and of every trip of
// the solve kernel) and what it works on: the per-slot scene context, load_scene() and the per-scene horizon.
//
// What this restates, MI355X-first (reference files relative to the reference repository's root):
//   * rollout a1 (include/nav2_social_mpc_controller/update_state.hpp:37-63) as ONE shared rollout per sweep
//     plus closed-form sensitivities S_t = d(x,y,theta)_{t+1}/d(params), instead of the reference's per-functor
//     O(t) re-integration on ceres::Jet;
//   * the nine instantiated residual kinds a2..a9 (include/.../critics/*_cost_function.hpp) with analytic
//     state-space gradients (x, y, theta, v_block) chained with S_t — equal to Ceres autodiff in exact arithmetic;
//   * the Gram contraction [J r]^T [J r] (gives J^T J, J^T r and the cost in one pass).
//
// The lane mapping (slots, one lane per horizon step) is described in smpc_launch.hpp.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/smpc.h"
#include "smpc_bicubic.hpp"
#include "smpc_launch.hpp"
#include "smpc_math.hpp"
#include "smpc_social_force.hpp"
#include "smpc_stage.hpp"

namespace smpc {

// The workgroup is ONE wavefront: LDS operations of a wave execute in program order, so cross-lane hand-offs through
// LDS only need the compiler not to reorder them — no s_barrier and, importantly, no s_waitcnt vmcnt(0) that a
// __syncthreads() would add (it would drain unrelated global loads / stores at every hand-off).
__device__ inline void wave_lds_fence() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <int W> __device__ inline double slot_sum(double v) {
#pragma unroll
  for (int off = W / 2; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// What lane ^ 32 holds: the same lane of the wave's other half (the other slot of a two-scenes-per-wave kernel). One LDS
// crossbar operation per 32 bits, nothing on the VALU but the address, which is the same at every call.
__device__ inline int other_half(int v) { return __builtin_amdgcn_ds_bpermute(((int)__lane_id() ^ 32) << 2, v); }
__device__ inline double other_half(double v) {
  return __hiloint2double(other_half(__double2hiint(v)), other_half(__double2loint(v)));
}
__device__ inline unsigned long long other_half(unsigned long long v) {
  return ((unsigned long long)(unsigned)other_half((int)(v >> 32)) << 32) | (unsigned)other_half((int)v);
}

// In-kernel phase stamps (diagnostic build -DSMPC_STAMPS only; the shipped kernel executes none of this).
#ifdef SMPC_STAMPS
#define SMPC_STAMP(ctx, phase) do { const unsigned long long _t = __builtin_amdgcn_s_memtime(); (ctx).acc[phase] += _t - (ctx).t_last; (ctx).t_last = _t; } while (0)
#define SMPC_STAMP2(ctx, phase) do { const unsigned long long _t = __builtin_amdgcn_s_memtime(); (ctx).acc2[phase] += _t - (ctx).t_last; (ctx).acc[5] += _t - (ctx).t_last; (ctx).t_last = _t; } while (0)
#else
#define SMPC_STAMP2(ctx, phase) do { } while (0)
#define SMPC_STAMP(ctx, phase) do { } while (0)
#endif

// ------------------------------------------------------------------------------------------------
// Per-slot scene context (registers; slot-uniform unless noted)
// ------------------------------------------------------------------------------------------------
struct Ctx {
#ifdef SMPC_STAMPS
  unsigned long long t_last;
  unsigned long long acc[8];
  unsigned long long acc2[4];
#endif
  KParamsK kp;  // the launch parameters, read where they lie in the kernel-argument segment
  int scene;   // scene index of this slot
  int sl;      // lane within the slot = horizon step owned by this lane (per-lane)
  int slot;
  bool has_people;
  bool gram_full;  // solve kernel: the latest sweep left the whole Gram in LDS, not only its last column (wave-uniform)
  const uint8_t* map;
  double* lds;       // this slot's LDS block (scene constants, cos/sin block, LM state live here)
  const double* ag;  // staged people records [N][T][4] of this slot's scene (global memory)
  double* wave_lds;  // wave-shared LDS behind the slot blocks (solve: feasibility rows of every slot; K1: row staging blocks)
  const double* atab;  // the wave's copy of the atan2_unit() nodes (LDS)
  LdsLayout L;
};

// every lane of the wave; the caller fences before the first sweep
__device__ inline void load_atan_nodes(KParamsK kp, double* dst, int lane) {
  for (int i = lane; i < kAtanTabDoubles; i += kWave) dst[i] = kp->an.v[i];
}

// Dense symmetric view of the slot's Gram [J r]^T [J r] left in LDS by sweep(): G(a, b), a, b in 0..P (column P = r).
struct GramView {
  const double* base;
  int ld;
  __device__ inline double operator()(int a, int b) const { return base[a * ld + b]; }
};

// The horizon of the slot's scene: rollout steps T, control horizon CH = min(control_horizon, T), block length
// bl = min(parameter_block_length, CH), index of the last parameter block, feasibility rows and bounded blocks
// (src/optimizer.cpp:248-249, 364, 373). kVT = false: one T per batch, everything is a launch constant (scalar
// registers; literals with a FixedShape, smpc_launch.hpp) and the last block is NB - 1. kVT = true (smpc_scene_batch.T_scene): per scene, kept in LDS by load_scene();
// a scene with fewer blocks than the batch's NB keeps its surplus parameters at exactly zero — their Jacobian columns
// are zero, the damped system is block diagonal and every sum gains exact zeros, so the iterates of the real
// parameters are those of the smaller problem bit for bit.
struct Horizon { int T, CH, bl, blast, nfeas, nbounded; };

template <int NB, bool kVT, class Shape = RuntimeShape> __device__ inline Horizon get_horizon(const Ctx& c) {
  static_assert(!(kVT && Shape::kFixed), "a fixed shape has one horizon for every scene");
  Horizon h;
  if (!kVT) {
    const auto& k = *c.kp;
    h.T = Shape::T(k); h.CH = Shape::CH(k); h.bl = Shape::bl(k); h.blast = NB - 1; h.nfeas = Shape::nfeas(k); h.nbounded = Shape::nbounded(k);
  } else {
    const int* z = reinterpret_cast<const int*>(c.lds + c.L.hz);
    h.T = z[0]; h.CH = z[1]; h.bl = z[2]; h.blast = z[3]; h.nfeas = z[4]; h.nbounded = z[5];
  }
  return h;
}

// the block driving step sl: min(sl, CH - 1) / bl, as a count of block starts at or before it (no division)
template <int NB> __device__ inline int block_of_step(int sl, const Horizon& h) {
  const int t = min(sl, h.CH - 1);
  int b = 0;
#pragma unroll
  for (int q = 1; q < NB; ++q) b += (t >= q * h.bl) ? 1 : 0;
  return b;
}

// one past the last step block b drives: the next block's start, the horizon for the last block, nothing beyond it
__device__ inline int block_end(int b, const Horizon& h) {
  return b < h.blast ? (b + 1) * h.bl : (b == h.blast ? h.T : b * h.bl);
}

// Load the slot's scene constants and the per-step side data of its staged people block (valid masks, agent-angle
// tags) into LDS; the records themselves stay in global memory (c.ag). Executed by all W lanes of the slot (other
// slots may be masked off).
// kStage (a solve kernel of a Shape with kStageAtFetch) and a launch with k.stage_at_fetch: no staging kernel ran. The
// slot's lanes stage the scene's people block here, with stage_people() itself — the records to the scene's region of
// k.stage_rec, masks and tags straight into the slot's LDS, nothing through k.people_aux. `stage` = false (the scene a
// slot loads only to have addresses in bounds, its results never stored) stages nothing and walks no agents: that
// scene's region belongs to the slot that fetched it from the queue.
template <int W, bool kVT = false, bool kSP = false, class Shape = RuntimeShape, bool kStage = false>
__device__ inline void load_scene(Ctx& c, int scene, bool stage = true) {
  const auto& k = *c.kp;
  const int T = Shape::T(k), N = Shape::N(k), sl = c.sl;
  if (kSP && sl < kSceneParamDoubles)  // the scene's row of smpc_scene_params, one value per lane
    (c.lds + c.L.sp)[sl] = reinterpret_cast<const double*>(k.scene_params + scene)[sl];
  int Th = T;  // the scene's own horizon
  if (kVT) {
    const int Traw = k.T_scene ? k.T_scene[scene] : T;
    Th = min(max(Traw, 1), T);
    const int CH = min(k.prm.control_horizon, Th);
    const int bl = max(min(k.prm.parameter_block_length, CH), 1);
    int* z = reinterpret_cast<int*>(c.lds + c.L.hz);
    z[0] = Th; z[1] = CH; z[2] = bl; z[3] = (CH - 1) / bl;
    z[4] = max(min(CH / bl, Th) - 1, 0);  // src/optimizer.cpp:364
    z[5] = CH / bl;                       // :373
    z[6] = Traw < 1 ? 1 : 0;              // a path of fewer than two poses: Optimizer::optimize returns false (:158-162)
  }
  const size_t s = scene;
  c.scene = scene;
  c.has_people = (N > 0) && (k.has_people ? k.has_people[s] != 0 : true);
  c.ag = k.people_rec + s * (size_t)4 * T * (N > 0 ? N : 1);
  const double x0 = k.pose0[3 * s], y0 = k.pose0[3 * s + 1], yaw0 = k.pose0[3 * s + 2];
  const size_t cm = (size_t)k.size_x * k.size_y;
  c.map = k.costmap + (k.costmap_shared ? 0 : cm * s);
  const double* path_pts = k.path_pts + s * (T + 1) * 2;
  double* cst = c.lds + c.L.cst;
  cst[0] = x0; cst[1] = y0; cst[2] = yaw0;
  cst[3] = k.goal_yaw[s];
  cst[4] = k.costmap_origin[k.costmap_shared ? 0 : 2 * s];
  cst[5] = k.costmap_origin[k.costmap_shared ? 1 : 2 * s + 1];
  cst[6] = path_pts[2 * Th];  // final trajectorized point (src/optimizer.cpp:234-235)
  cst[7] = path_pts[2 * Th + 1];
  double* lanec = c.lds + c.L.lanec;
  bool staged_here = false;  // masks and tags of this scene are in LDS already
  if constexpr (kStage) {
    if (k.stage_at_fetch) {
      if (!stage) c.has_people = false;
      if (c.has_people) {
        double* rec = k.stage_rec + s * (size_t)4 * T * N;  // 32 T N bytes: whole 128-byte lines, none shared with a neighbour
        stage_people<W, Shape>(c.kp, scene, sl, rec, reinterpret_cast<unsigned long long*>(c.lds + c.L.valid), lanec + 2 * T);
        c.ag = rec;
        // Lane l stored records (a, t) that lane t reads in every sweep, through global memory: program order within a
        // lane says nothing about what another lane's load finds, and a wavefront-scope fence orders LDS traffic only. The
        // release makes the wave's stores complete and visible at the device's L2 before anything behind it, the acquire
        // drops what the CU's vector cache holds, so that no load of the sweeps can be served from a line cached before
        // the stores (the region's previous contents: an earlier launch of this handle). Once per scene fetch; nothing
        // waits on another wave, the records have one writer and one reader, this slot.
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        staged_here = true;
      }
    }
  }
  if (sl < T) {
    double aa_target = kNoTarget;
    if (c.has_people && !staged_here) {
      const double* aux = k.people_aux + (s * T + sl) * 2;
      (c.lds + c.L.valid)[sl] = aux[0];  // the mask's bits travel in a double-sized slot
      aa_target = aux[1];
    }
    lanec[sl] = path_pts[2 * (sl + 1)];
    lanec[T + sl] = path_pts[2 * (sl + 1) + 1];
    if (!staged_here) lanec[2 * T + sl] = aa_target;
  }
}

// A field of smpc_scene_params where it is used: the slot's own row in LDS (kSP, the sp kernels: written by load_scene();
// with two scenes per wave the two halves hold different rows, so the value is a per-lane operand, read at each use rather
// than held in registers through the sweep) or `prm`, the handle's smpc_params (a launch constant, scalar loads).
#define SMPC_SCENE_PRM(c, kSP, prm, field) \
  ((kSP) ? (c).lds[(c).L.sp + offsetof(smpc_scene_params, field) / sizeof(double)] : (prm).field)

// ------------------------------------------------------------------------------------------------
// The sweep (kernel K1's body): residuals + Jacobian rows + Gram at the slot's parameters xp[P] (LDS or global,
// slot-uniform). All 64 lanes of the wave call it together (each slot on its own scene). The Gram is returned
// reduced over the slot in every lane of the slot.
// When out_r / out_J are non-null (stand-alone K1) the rows are also written to HBM in the reference order.
// ------------------------------------------------------------------------------------------------
// kRows = false: the solve kernel's sweep, full Gram [J r]^T [J r] (structured, on the VALU), nothing written.
// kRows = true: the stand-alone K1 sweep; rows go to HBM, and of the Gram only its last column (J^T r and r^T r: the
// gradient and the cost smpc_eval_batch reports) is accumulated, on the VALU — c.wave_lds is then the row staging
// area of the critic-major store path (2 x T x P doubles per slot).
// need_rest (solve kernel only): called by every lane once the LAST column of the Gram — J^T r and r^T r: gradient and
// cost — is reduced and visible in LDS; the other columns (J^T J) are formed and reduced only if it returns true in some
// lane of the wave. A line-search sample that fails the Armijo test needs no more than that column (Ceres evaluates cost
// and gradient there, LineSearchFunction::Evaluate), and most sweeps of a solve are such samples. c.gram_full tells
// the caller what it got (wave-uniform). Every entry is summed in the same order whichever way it is produced.
struct NeedAll { __device__ inline bool operator()() const { return true; } };
// Shape: where T, N, CH, bl and what follows from them come from — the launch values (RuntimeShape) or the literals of a
// FixedShape (smpc_launch.hpp). The arithmetic on doubles and the order of every sum are the same in both.
// kLone (the solve kernels of lone_trip_kernel()): a trip the caller marks lone — one slot of the wave idle for good, the
// other live with people and N >= 2; trip_mode() — walks the agents two at a time. Both halves evaluate pair_force() in
// the same instructions, the owner lanes (the live slot) for agent 2i, their mirror lanes of the idle half (the helpers)
// for agent 2i + 1 at the owner's pose; the owner lane then accumulates its own Force and, fetched across the halves,
// the mirror lane's, with the statements of the paired loop in the order of the paired loop: agents 0, 1, ..., N - 1.
// Every operand of every sum is the value the owner's own evaluation would have produced, so a scene's result does not
// depend on whether, or from which sweep on, its trips were lone. The idle half's own sums are junk and go nowhere, as
// ever.
// The trip's mode travels in a word of the slot's LDS (the spare eighth integer of the horizon block, which only the
// kernels with a horizon per scene fill, and those have no lone trips), written by the solve kernel before the sweep and
// read where the sweep needs it: held in scalar registers from the trip's head to the agent loop it spilled four of them.
enum TripMode { kTripPaired = 0, kTripOwner = 1, kTripHelper = 2 };
__device__ inline int* trip_mode(const Ctx& c) { return reinterpret_cast<int*>(c.lds + c.L.hz) + 7; }

template <int NB, int W, bool kRows, bool kVT = false, bool kSP = false, class Shape = RuntimeShape, bool kLone = false,
          class NeedRest = NeedAll>
__device__ inline GramView sweep(Ctx& c, const double* xp, double* out_r, double* out_J, NeedRest need_rest = NeedRest()) {
  constexpr int P = 2 * NB;
  const auto& k = *c.kp;
  const int T = Shape::T(k), N = Shape::N(k), sl = c.sl;  // T: the batch's T = the stride of every per-step array
  const Horizon hz = get_horizon<NB, kVT, Shape>(c);
  const int Th = hz.T, CH = hz.CH, bl = hz.bl;  // Th: the scene's own rollout steps (== T unless kVT)
  const double dt = k.dt;
  double* cs_ = c.lds + c.L.cs;
  double* sn_ = cs_ + (T + 1);
  const double* cst = c.lds + c.L.cst;
  const int tl = min(sl, Th - 1);
  const int myb = block_of_step<NB>(sl, hz);  // block driving step sl
  const double vb = xp[2 * myb], wb = xp[2 * myb + 1];

  // staged people records of this lane's step: agent a at agr[a * T]; the first two are requested now, so that their
  // latency (HBM in the stand-alone K1 kernel) passes behind the rollout
  const v4d* agr = reinterpret_cast<const v4d*>(c.ag) + tl;
  v4d rec0 = {0.0, 0.0, 0.0, 0.0}, rec1 = {0.0, 0.0, 0.0, 0.0};
  bool lone = false, hlp = false;  // kLone: a lone trip (wave-uniform); this lane is a helper
  if constexpr (kLone) {
    const int mode = *trip_mode(c);
    lone = __builtin_amdgcn_readfirstlane(mode) != kTripPaired;
    hlp = mode == kTripHelper;
  }
  if (kLone && lone) {
    // a lone trip: the helper lanes read the owner's records, agents 1, 3, ... where the owner takes 0, 2, ... (their own
    // scene's pointer is not needed again: the proxemics fetch behind the loop is in bounds in either scene)
    // (every exchange across the halves is executed by all lanes: a lane switched off hands nothing over)
    const v4d* owner_agr = reinterpret_cast<const v4d*>(other_half(reinterpret_cast<unsigned long long>(agr)));
    agr = hlp ? owner_agr : agr;
    rec0 = agr[(hlp ? 1 : 0) * T];  // (the lone-trip kernels' agent loop fetches one unit ahead: no second record)
  } else
  if (c.has_people) {
    rec0 = agr[0];
    if constexpr (!kLone) rec1 = agr[(N > 1 ? 1 : 0) * T];
  }

  // ---- a1 rollout (update_state.hpp:37-63), block-structured. The recurrences are sums, so they are evaluated as
  // sums: theta_t = yaw0 + sum_b (w_b dt) * (steps of block b before t), and the positions through inclusive prefix
  // sums over the lanes, restarted at every block boundary, of cos / sin(theta_j) and (j - block start) cos / sin:
  // every partial sum the pose and its sensitivities need is then one scan entry (the lane's own for its block, the
  // entry of a block's last step for the blocks before it) — no differences of long sums. (The reference adds the
  // terms one step at a time; the orders differ by rounding only, a few ulp.)
  double th = cst[2];
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    const int start = b * bl;
    const int len = block_end(b, hz) - start;
    const int cnt = min(max(sl - start, 0), len);  // steps j < sl that block b drives
    th = fma(xp[2 * b + 1] * dt, (double)cnt, th);
  }
  const double th1 = th + wb * dt;  // theta_{sl+1}
  double* scan_ = c.lds + c.L.inc;  // [4][T+1]: block-wise inclusive scans C, S, JC, JS over j = 0..T
  const int seg_start = myb * bl;
  {
    double sn, cs;
    // headings of a rollout are modest numbers; the library routine (Payne-Hanek reduction) only for a lane that holds a
    // heading beyond the two-part Cody-Waite range (an unbounded last parameter block can produce one)
    if (__builtin_expect(!(fabs(th) <= 1e5), 0)) sincos(th, &sn, &cs);
    else sincos_tab(&k.mt, th, &sn, &cs);
    const double fj = (double)(sl - seg_start);
    double sC = cs, sS = sn, sJC = fj * cs, sJS = fj * sn;
#pragma unroll
    for (int off = 1; off < W; off <<= 1) {
      const double uC = __shfl_up(sC, off, W), uS = __shfl_up(sS, off, W);
      const double uJC = __shfl_up(sJC, off, W), uJS = __shfl_up(sJS, off, W);
      const double m = (sl - off >= seg_start) ? 1.0 : 0.0;  // the source lane belongs to this lane's block
      sC = fma(m, uC, sC); sS = fma(m, uS, sS); sJC = fma(m, uJC, sJC); sJS = fma(m, uJS, sJS);
    }
    if (sl <= T) {
      cs_[sl] = cs; sn_[sl] = sn;
      scan_[sl] = sC; scan_[(T + 1) + sl] = sS; scan_[2 * (T + 1) + sl] = sJC; scan_[3 * (T + 1) + sl] = sJS;
    }
  }
  wave_lds_fence();
  SMPC_STAMP(c, 1);
  // x, y of pose_{sl+1} = pose0 + sum_b v_b dt * (sum of cos / sin(theta_j) over the steps j <= sl of block b)
  double X = cst[0], Y = cst[1];
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    const int end = block_end(b, hz);
    const int idx = (b < myb) ? end - 1 : tl;   // a finished block: its last step; the lane's own block: the lane
    const double m = (b <= myb) ? 1.0 : 0.0;
    const double vdt = xp[2 * b] * dt * m;
    X = fma(vdt, scan_[idx], X); Y = fma(vdt, scan_[(T + 1) + idx], Y);
  }
  const int t1 = min(sl + 1, Th);
  const double c1 = cs_[t1], s1 = sn_[t1];  // heading of the residual's pose
  // a5 obstacle: the costmap patch under the front point is requested now and used after the agent loop
  // cell coordinates of the front point: (front - origin) / resolution (critics/obstacle_cost_function.hpp:154-158) as a
  // product with the host-rounded reciprocal (within an ulp of the quotient; the interpolant is C1, so an ulp of its
  // argument is an ulp of its value)
  const bool wide_map = k.size_x >= 4;
  CostPatch patch;
  bool patch_interior = false;  // wave-uniform
  if (wide_map) {
    const double ob_ic = (X + 0.25 * c1 - cst[4]) * k.inv_resolution, ob_ir = (Y + 0.25 * s1 - cst[5]) * k.inv_resolution;
    patch_interior = __all(bicubic_interior(k.size_x, k.size_y, ob_ir, ob_ic));
    if (patch_interior) bicubic_fetch<true>(c.map, k.size_x, k.size_y, ob_ir, ob_ic, patch);
    else bicubic_fetch<false>(c.map, k.size_x, k.size_y, ob_ir, ob_ic, patch);
  }

  SMPC_STAMP(c, 2);
  // ---- a3 social work + a4 proxemics: walk the agents of step sl
  // what leaves this block is the finished social-work critic (residual and state-space gradient) and the nearest
  // valid agent of the proxemics critic: eight values across the divergent branch instead of the 23 running sums
  double sw_r = 0.0, sw_gx = 0.0, sw_gy = 0.0, sw_gt = 0.0, sw_gv = 0.0;
  double pbest = 1.7976931348623157e308, pdx = 0.0, pdy = 0.0;
  if constexpr (kLone) {  // (read again rather than kept)
    const int mode = *trip_mode(c);
    lone = __builtin_amdgcn_readfirstlane(mode) != kTripPaired;
    hlp = mode == kTripHelper;
  }
  if (c.has_people || (kLone && hlp)) {
    double soc[kSoc];
#pragma unroll
    for (int i = 0; i < kSoc; ++i) soc[i] = 0.0;
    double su[4] = {0.0, 0.0, 0.0, 0.0};  // sums over valid agents of dF/du: (fx,ux) (fy,ux) (fx,uy) (fy,uy)
    double qh[4] = {0.0, 0.0, 0.0, 0.0};  // sums over pairs of F . dF/d(x, y, ux, uy), agent side
    const MathTabP mt = &k.mt;
    const double* atab = c.atab;
    const unsigned long long* vmask = reinterpret_cast<const unsigned long long*>(c.lds + c.L.valid);
    unsigned long long vm = vmask[tl];
    double rvx = vb * c1, rvy = vb * s1;  // meVel, social_work:170-171
    int pidx = 0;  // proxemics: index of the nearest valid agent (first minimum wins: std::min on duals)
    bool redo = false;  // some pair of this lane is not a regular one
    // One robot-agent pair: the robot of a step at (px, py) with velocity (pvx, pvy) against agent a of that step.
    // One evaluation serves both directions: the force on the robot from the agent (:125; valid agents only, :175)
    // is F(diff, u), diff = robot - agent, u = robotVel - agentVel; the force on the agent from the robot
    // (:137-143; every column, phantoms included) is F(-diff, -u) = -F with the same derivatives, so |.|^2 and its
    // gradient are those of F.
    // (the nearest-agent test and the sums as text: a lone trip's loop runs the same statements, on a Force that may have
    // been evaluated in the other half of the wave)
#define SMPC_PAIR_NEAREST(d2, a, valid) \
      const bool nearer = valid & (d2 < pbest); \
      pbest = nearer ? d2 : pbest; \
      pidx = nearer ? a : pidx;
    // |diff| < 1e-6 -> diff := (1e-6, 0), :181-184, breaks the symmetry above: redo.
    // Derivatives with respect to the robot's (theta, v) are one rotation of the u-derivatives that is the same for every
    // agent of this step (u = v (cos theta, sin theta) - agentVel): sum the u-derivatives, rotate once after the loop.
#define SMPC_PAIR_ADD(F, special, d2, valid) \
      redo |= special | (d2 < 1e-12); \
      const double m = valid ? 1.0 : 0.0; \
      soc[0] = fma(m, F.fx, soc[0]); soc[1] = fma(m, F.fy, soc[1]); \
      soc[2] = fma(m, F.dfx_dx, soc[2]); soc[3] = fma(m, F.dfy_dx, soc[3]); \
      soc[4] = fma(m, F.dfx_dy, soc[4]); soc[5] = fma(m, F.dfy_dy, soc[5]); \
      su[0] = fma(m, F.dfx_dux, su[0]); su[1] = fma(m, F.dfy_dux, su[1]); \
      su[2] = fma(m, F.dfx_duy, su[2]); su[3] = fma(m, F.dfy_duy, su[3]); \
      soc[10] = fma(F.fx, F.fx, fma(F.fy, F.fy, soc[10])); \
      qh[0] = fma(F.fx, F.dfx_dx, fma(F.fy, F.dfy_dx, qh[0])); \
      qh[1] = fma(F.fx, F.dfx_dy, fma(F.fy, F.dfy_dy, qh[1])); \
      qh[2] = fma(F.fx, F.dfx_dux, fma(F.fy, F.dfy_dux, qh[2])); \
      qh[3] = fma(F.fx, F.dfx_duy, fma(F.fy, F.dfy_duy, qh[3]));
    auto pair = [&](const v4d& rec, int a, bool valid, double px, double py, double pvx, double pvy) {
      const double apx = rec[0], apy = rec[1], awx = rec[2], awy = rec[3];
      const double dx = px - apx, dy = py - apy;
      const double d2 = fma(dx, dx, dy * dy);
      SMPC_PAIR_NEAREST(d2, a, valid)
      const Force F = pair_force(mt, atab, dx, dy, pvx - awx, pvy - awy);
      SMPC_PAIR_ADD(F, F.special, d2, valid)
    };
    const int A = (W == 64) ? Shape::hp_A(k) : N;  // agents the owner lane walks itself (helper_owner_agents(): N without helpers)
    if (W == 64 && A < N) {
      // ---- with helper lanes (see helper_owner_agents()): lanes sl >= T walk agents A .. N-1 of the steps h, h + R, ...
      const int NA = N - A, R = W - T;
      double* stp = c.lds + c.L.stepst;
      double* part = c.lds + c.L.part;
      const bool helper = sl >= T;
      if (sl < Th) { stp[sl] = X; stp[T + sl] = Y; stp[2 * T + sl] = rvx; stp[3 * T + sl] = rvy; }
      wave_lds_fence();
      // the step this lane currently works for, and what a pair evaluation needs of it
      int t_cur = helper ? sl - T : tl;
      bool unit_ok = helper ? (t_cur < Th) : (sl < Th);
      double cX = X, cY = Y, cvx = rvx, cvy = rvy;
      unsigned long long cvm = vm;
      if (helper) {
        const int ts = min(t_cur, Th - 1);
        cX = stp[ts]; cY = stp[T + ts]; cvx = stp[2 * T + ts]; cvy = stp[3 * T + ts]; cvm = vmask[ts];
      }
      int a_cur = helper ? A : 0, k_in = 0;
      const v4d* recs = reinterpret_cast<const v4d*>(c.ag);  // record of agent a at step t: recs[a * T + t]
      v4d rec_next = recs[a_cur * T + min(t_cur, Th - 1)];
      for (int it = 0; it < A; ++it) {
        const v4d rec = rec_next;
        // where this lane goes next (a helper that has finished a unit moves R steps on), fetched one pair ahead
        const bool unit_end = helper && (k_in + 1 == NA);
        const int t_next = unit_end ? t_cur + R : t_cur;
        const int a_next = unit_end ? A : a_cur + 1;
        rec_next = recs[min(a_next, N - 1) * T + min(t_next, Th - 1)];
        if (unit_ok) pair(rec, a_cur, (cvm >> a_cur) & 1ull, cX, cY, cvx, cvy);
        if (unit_end) {
          if (unit_ok) {  // hand the unit's sums to the owner lane of its step
            double* pr = part + t_cur * kPart;
#pragma unroll
            for (int i = 0; i < 6; ++i) pr[i] = soc[i];
#pragma unroll
            for (int i = 0; i < 4; ++i) { pr[6 + i] = su[i]; pr[11 + i] = qh[i]; }
            pr[10] = soc[10];
            pr[15] = pbest;
            pr[16] = (double)(pidx + (redo ? 4096 : 0));
          }
#pragma unroll
          for (int i = 0; i < 6; ++i) soc[i] = 0.0;
#pragma unroll
          for (int i = 0; i < 4; ++i) { su[i] = 0.0; qh[i] = 0.0; }
          soc[10] = 0.0; pbest = 1.7976931348623157e308; pidx = 0; redo = false;
          unit_ok = t_next < Th;
          const int ts = min(t_next, Th - 1);
          cX = stp[ts]; cY = stp[T + ts]; cvx = stp[2 * T + ts]; cvy = stp[3 * T + ts]; cvm = vmask[ts];
          k_in = 0;
        } else {
          k_in += helper ? 1 : 0;
        }
        t_cur = t_next; a_cur = a_next;
      }
      wave_lds_fence();
      if (!helper && sl < Th) {  // the owner adds what the helper found for its step
        const double* pr = part + sl * kPart;
#pragma unroll
        for (int i = 0; i < 6; ++i) soc[i] += pr[i];
#pragma unroll
        for (int i = 0; i < 4; ++i) { su[i] += pr[6 + i]; qh[i] += pr[11 + i]; }
        soc[10] += pr[10];
        const int tag = (int)pr[16];
        // the helper's agents come after the owner's: a tie stays with the owner (std::min keeps the first minimum)
        if (pr[15] < pbest) { pbest = pr[15]; pidx = tag & 4095; }
        redo |= tag >= 4096;
      }
    } else if constexpr (kLone) {
      // ---- the kernels with lone trips (see the head of sweep()): one loop for both kinds of trip — a second copy of
      // pair_force() in the kernel costs registers the sweep does not have. A paired trip walks agent a per iteration, as
      // the loop below does; a lone trip agents a (owner half) and a + 1 (helper half).
      // A helper lane's own pose and velocity wait in LDS (behind the scans, in the part of the Gram reduction buffer that is
      // idle until the critics are done): its critics below rely on them for addresses in bounds.
      double* keep = c.lds + c.L.cs + 6 * (T + 1) + 4 * sl;
      int mine = 0, step = 1;
      if (lone) {
        keep[0] = X; keep[1] = Y; keep[2] = rvx; keep[3] = rvy;
        const unsigned long long ovm = other_half(vm);  // selects behind the exchanges: every lane hands over
        const double oX = other_half(X), oY = other_half(Y), ovx = other_half(rvx), ovy = other_half(rvy);
        vm = hlp ? ovm : vm; X = hlp ? oX : X; Y = hlp ? oY : Y; rvx = hlp ? ovx : rvx; rvy = hlp ? ovy : rvy;
        mine = hlp ? 1 : 0;
        step = 2;
      }
      for (int a = 0; a < N; a += step) {
        // rec0: of agent a + mine (the helper's last unit of an odd N: some record, its Force is not used). A record is dead
        // four subtractions into the body, and the next unit's is fetched over it: one record in flight, nothing to rotate
        // at the back edge (two in flight were eight 64-bit moves per pair). A body is some 800 cycles of VALU, enough for
        // the L2 hit a solve's records are; K1 and the helper-lane loop, whose first touch comes from HBM, keep two.
        double dx = X - rec0[0], dy = Y - rec0[1], ux = rvx - rec0[2], uy = rvy - rec0[3];
        // (the differences are formed before the fetch is issued — left to itself the compiler fetches first, into other
        // registers, and copies at the back edge; the index stays inside the list, as in the fetch ahead of the rollout)
        asm volatile("" : "+v"(dx), "+v"(dy), "+v"(ux), "+v"(uy));
        rec0 = agr[min(a + mine + step, N - 1) * T];
        double d2 = fma(dx, dx, dy * dy);
        Force F = pair_force(mt, atab, dx, dy, ux, uy);
        int special = F.special ? 1 : 0;
        {
          const bool valid = (vm >> a) & 1ull;
          SMPC_PAIR_NEAREST(d2, a, valid)
          SMPC_PAIR_ADD(F, (special != 0), d2, valid)
        }
        if (step == 2 && a + 1 < N) {  // (wave-uniform) agent a + 1: the mirror lane's evaluation
          // the Force crosses in the registers it has, behind the sums that read it (the scheduler would start the exchange
          // early and hold both copies)
          __builtin_amdgcn_sched_barrier(0);
          F.fx = other_half(F.fx); F.fy = other_half(F.fy);
          F.dfx_dx = other_half(F.dfx_dx); F.dfy_dx = other_half(F.dfy_dx);
          F.dfx_dy = other_half(F.dfx_dy); F.dfy_dy = other_half(F.dfy_dy);
          F.dfx_dux = other_half(F.dfx_dux); F.dfy_dux = other_half(F.dfy_dux);
          F.dfx_duy = other_half(F.dfx_duy); F.dfy_duy = other_half(F.dfy_duy);
          d2 = other_half(d2);
          special = other_half(special);
          __builtin_amdgcn_sched_barrier(0);
          const bool valid = (vm >> (a + 1)) & 1ull;
          SMPC_PAIR_NEAREST(d2, (a + 1), valid)
          SMPC_PAIR_ADD(F, (special != 0), d2, valid)
        }
      }
      if (step == 2) {  // (step and mine, not the flags they came from: two scalar registers fewer through the loop)
        redo = redo & (mine == 0);  // the re-walk in the general form is the owner's alone
        X = keep[0]; Y = keep[1]; rvx = keep[2]; rvy = keep[3];  // (an owner lane reads back what it wrote)
      }
    } else {
      for (int a = 0; a < N; ++a) {
        // records are fetched two agents ahead (the first two before the rollout, above): HBM latency in K1, L2 in a solve
        const v4d rec = rec0;
        rec0 = rec1;
        if (a + 2 < N) rec1 = agr[(a + 2) * T];
        pair(rec, a, (vm >> a) & 1ull, X, Y, rvx, rvy);
      }
    }
    {  // the constant factors pair_force() leaves out, once per step instead of once per pair
      const double kk = kPairForceK, kl = kPairForceK * kPairForceLambda, k2 = kPairForceK * kPairForceK,
                   k2l = kPairForceK * kPairForceK * kPairForceLambda;
#pragma unroll
      for (int i = 0; i < 6; ++i) soc[i] *= kk;
#pragma unroll
      for (int i = 0; i < 4; ++i) su[i] *= kl;
      soc[10] *= k2; qh[0] *= k2; qh[1] *= k2; qh[2] *= k2l; qh[3] *= k2l;
    }
    if (__builtin_expect(redo, 0)) {
      // Rare: this lane met a pair the fast form does not cover. It walks its agents again in the general form (both
      // directions evaluated where the symmetry does not hold), from cleared sums. Decided per lane: the result of a
      // scene must not depend on which other scene shares its wave.
#pragma unroll
      for (int i = 0; i < kSoc; ++i) soc[i] = 0.0;
#pragma unroll
      for (int i = 0; i < 4; ++i) { su[i] = 0.0; qh[i] = 0.0; }
      for (int a = 0; a < N; ++a) {
        const v4d rec = agr[a * T];
        const double apx = rec[0], apy = rec[1], awx = rec[2], awy = rec[3];
        const bool valid = (vm >> a) & 1ull;
        const double dx = X - apx, dy = Y - apy;
        const double d2 = dx * dx + dy * dy;
        const bool degenerate = d2 < 1e-12;
        if (valid) {
          const Force F = social_force_general(dx, dy, rvx - awx, rvy - awy);
          soc[0] += F.fx; soc[1] += F.fy;
          soc[2] += F.dfx_dx; soc[3] += F.dfy_dx; soc[4] += F.dfx_dy; soc[5] += F.dfy_dy;
          su[0] += F.dfx_dux; su[1] += F.dfy_dux; su[2] += F.dfx_duy; su[3] += F.dfy_duy;
          if (!degenerate) {
            soc[10] = fma(F.fx, F.fx, fma(F.fy, F.fy, soc[10]));
            qh[0] = fma(F.fx, F.dfx_dx, fma(F.fy, F.dfy_dx, qh[0]));
            qh[1] = fma(F.fx, F.dfx_dy, fma(F.fy, F.dfy_dy, qh[1]));
            qh[2] = fma(F.fx, F.dfx_dux, fma(F.fy, F.dfy_dux, qh[2]));
            qh[3] = fma(F.fx, F.dfx_duy, fma(F.fy, F.dfy_duy, qh[3]));
          }
        }
        if (!valid || degenerate) {
          const Force G = social_force_general(-dx, -dy, awx - rvx, awy - rvy);
          soc[10] += G.fx * G.fx + G.fy * G.fy;
          // d/d(robot x, y) = -d/d(diff), d/d(robot u) = -d/d(u): entered with the sign, rotated with the rest below
          qh[0] -= G.fx * G.dfx_dx + G.fy * G.dfy_dx;
          qh[1] -= G.fx * G.dfx_dy + G.fy * G.dfy_dy;
          qh[2] -= G.fx * G.dfx_dux + G.fy * G.dfy_dux;
          qh[3] -= G.fx * G.dfx_duy + G.fy * G.dfy_duy;
        }
      }
    }
    {
      const v4d prec = agr[pidx * T];
      pdx = X - prec[0]; pdy = Y - prec[1];
    }
    soc[6] = vb * (-s1 * su[0] + c1 * su[2]); soc[7] = vb * (-s1 * su[1] + c1 * su[3]);  // d(sum F)/d theta
    soc[8] = c1 * su[0] + s1 * su[2]; soc[9] = c1 * su[1] + s1 * su[3];                  // d(sum F)/d v
    soc[11] += 2.0 * qh[0];
    soc[12] += 2.0 * qh[1];
    soc[13] += 2.0 * (vb * (-s1 * qh[2] + c1 * qh[3]));
    soc[14] += 2.0 * (c1 * qh[2] + s1 * qh[3]);
    // a3 social work: w (|sum F|^2 + sum |G|^2 + 1e-6), critics/social_work_cost_function.hpp:125-147
    const double wsoc = SMPC_SCENE_PRM(c, kSP, k.prm, socialwork_w);
    const double wr = soc[0] * soc[0] + soc[1] * soc[1];
    sw_r = wsoc * (wr + soc[10] + 1e-6);
    sw_gx = wsoc * (2.0 * (soc[0] * soc[2] + soc[1] * soc[3]) + soc[11]);
    sw_gy = wsoc * (2.0 * (soc[0] * soc[4] + soc[1] * soc[5]) + soc[12]);
    sw_gt = wsoc * (2.0 * (soc[0] * soc[6] + soc[1] * soc[7]) + soc[13]);
    sw_gv = wsoc * (2.0 * (soc[0] * soc[8] + soc[1] * soc[9]) + soc[14]);
  }

  SMPC_STAMP(c, 3);
  // ---- sensitivities S of pose_{sl+1}, from the scans. K1 needs them for every row it forms, so right after the agent
  // loop; the solve kernel only for the final M^T A M, so after the critics (they stay out of the critics' register
  // budget, as the critics' sums stay out of theirs).
  double Sxv[NB], Syv[NB], Sxw[NB], Syw[NB], Sthw[NB];
  auto compute_sensitivities = [&]() {
  #pragma unroll
    for (int b = 0; b < NB; ++b) {
      const int start = b * bl;
      const int end = block_end(b, hz);
      const int idx = (b < myb) ? end - 1 : tl;
      const double m = (b <= myb) ? 1.0 : 0.0;
      const double aC = m * scan_[idx], aS = m * scan_[(T + 1) + idx];
      const double aJC = m * scan_[2 * (T + 1) + idx], aJS = m * scan_[3 * (T + 1) + idx];  // sums of (j - start) cos / sin
      const double vdt = xp[2 * b] * dt;
      Sxv[b] = dt * aC;
      Syv[b] = dt * aS;
      // d theta_j / d w_b = dt (j - start) inside block b; = dt * bl for every later step
      Sxw[b] = -vdt * dt * aJS;
      Syw[b] = vdt * dt * aJC;
  #pragma unroll
      for (int q = 0; q < b; ++q) {
        Sxw[q] = fma(-vdt * dt * (double)bl, aS, Sxw[q]);
        Syw[q] = fma(vdt * dt * (double)bl, aC, Syw[q]);
      }
      const int cnt = min(max(sl + 1 - start, 0), end - start);
      Sthw[b] = dt * (double)max(cnt, 0);
    }
  };
  if (kRows) compute_sensitivities();
  // K1 with seven or more parameter blocks: the 5 NB sensitivities of a lane (100 registers at NB = 10) are parked in LDS
  // behind the row staging blocks, lane index fastest, and read back entry by entry while the rows are formed — with
  // them in registers the kernel needed 256 VGPRs plus up to 110 AGPR copies
  constexpr bool kSensInLds = kRows && NB > kSensInRegsMaxBlocks;
  double* sens_lds = c.wave_lds + (kWave / W) * (2 * T * P) + c.slot * (5 * NB * W) + sl;
  if (kSensInLds) {
#pragma unroll
    for (int q = 0; q < NB; ++q) {
      sens_lds[(0 * NB + q) * W] = Sxv[q]; sens_lds[(1 * NB + q) * W] = Syv[q]; sens_lds[(2 * NB + q) * W] = Sxw[q];
      sens_lds[(3 * NB + q) * W] = Syw[q]; sens_lds[(4 * NB + q) * W] = Sthw[q];
    }
    wave_lds_fence();
  }

  SMPC_STAMP(c, 4);
  // ---- per-step critics: residual r and its state-space gradient (gx, gy, gth; gv = direct derivative with respect
  // to the linear velocity of block myb). Row of the Jacobian = gradient x M, M = [S; selector] (4 x P), the same M
  // for every critic of the step.
  //   kRows (K1): the rows are formed and written to HBM; of the Gram only the last column is kept (VALU).
  //   solve:      rows are never formed. Per lane A = sum_k g_k^T g_k (4 x 4), b = sum_k g_k r_k, cc = sum_k r_k^2 are
  //               accumulated over the step's critics (most gradients have one to three non-zero components), then
  //               the lane's share of [J r]^T [J r] is M^T A M, M^T b, cc — 1/3 of the multiply-adds of forming and
  //               contracting eight P-wide rows, and no FP64 MFMA (on this part it runs at the FP64 VALU rate on the
  //               same pipe: measured slower than plain VALU accumulation).
  constexpr int Q = P + 1;
  const auto& w = k.prm;
#define SPRM(f) SMPC_SCENE_PRM(c, kSP, w, f)  // the weights and the target speed of this slot's scene
  const bool lane_live = sl < Th;
  const bool people = c.has_people;
  const int rows_per_step = people ? 8 : 5;
  const int row_base = rows_per_step * sl + min(max(sl - 1, 0), hz.nfeas);
  double gcol[Q];      // kRows: last column of the Gram only
  double Axx = 0.0, Axy = 0.0, Axt = 0.0, Axv = 0.0, Ayy = 0.0, Ayt = 0.0, Ayv = 0.0, Att = 0.0, Atv = 0.0, Avv = 0.0;
  double bx = 0.0, by = 0.0, bt = 0.0, bv = 0.0, cc = 0.0;
  double* stage = c.wave_lds + c.slot * (2 * T * P);  // kRows: two row blocks of this slot, used alternately
  const bool critic_major = kRows && k.e_row_order == 1;
  if (kRows) {
#pragma unroll
    for (int q = 0; q < Q; ++q) gcol[q] = 0.0;
  }
  // One row of the Jacobian = gradient x M, formed two entries (one parameter block) at a time: each pair goes to its
  // destination and into the last Gram column at once, so no whole row is ever held in registers (with ten parameter
  // blocks a row is 40 registers on top of the 100 of the sensitivities).
  auto emit = [&](int local, bool live, bool slot_on, double r, double gx, double gy, double gth, double gv) {  // kRows only
    const double rl = live ? r : 0.0;
    double* blk = stage + (local & 1) * (T * P);
    const int rowi = row_base + local;
    const bool to_lds = critic_major && sl < T && slot_on;   // every row of the block, the all-zero rows of steps beyond
                                                             // the scene's horizon included
    const bool to_mem = !critic_major && live && out_J;
#pragma unroll
    for (int q = 0; q < NB; ++q) {
      const double sxv = kSensInLds ? sens_lds[(0 * NB + q) * W] : Sxv[q], syv = kSensInLds ? sens_lds[(1 * NB + q) * W] : Syv[q];
      const double sxw = kSensInLds ? sens_lds[(2 * NB + q) * W] : Sxw[q], syw = kSensInLds ? sens_lds[(3 * NB + q) * W] : Syw[q];
      const double sthw = kSensInLds ? sens_lds[(4 * NB + q) * W] : Sthw[q];
      double e0 = gx * sxv + gy * syv + ((q == myb) ? gv : 0.0);
      double e1 = gx * sxw + gy * syw + gth * sthw;
      e0 = live ? e0 : 0.0; e1 = live ? e1 : 0.0;
      gcol[2 * q] = fma(e0, rl, gcol[2 * q]);
      gcol[2 * q + 1] = fma(e1, rl, gcol[2 * q + 1]);
      v2d pr = {e0, e1};
      // critic-major: row (critic `local`, step sl) lives at index local * T + sl, the T rows of one critic are one
      // contiguous block of T * P doubles. They pass through LDS so that every store instruction writes whole runs of
      // consecutive 16-byte pieces (lane-strided 48-byte rows touch 64 different lines per instruction and leave
      // partially written lines behind: measured 1.49 x write amplification in round 1).
      if (to_lds) reinterpret_cast<v2d*>(blk + sl * P)[q] = pr;
      if (to_mem) reinterpret_cast<v2d*>(out_J + (size_t)rowi * P)[q] = pr;
    }
    gcol[P] = fma(rl, rl, gcol[P]);
    if (critic_major) {
      wave_lds_fence();
      if (out_J && slot_on) {
        v2d* dst = reinterpret_cast<v2d*>(out_J + (size_t)local * T * P);
        const v2d* src = reinterpret_cast<const v2d*>(blk);
        for (int i = sl; i < T * NB; i += W) dst[i] = src[i];
      }
      if (out_r && sl < T && slot_on) out_r[local * T + sl] = rl;
      // no second fence: the next critic writes the other block, and the one after that comes behind this
      // critic's reads in program order with a fence in between
    } else if (live && out_r) {
      out_r[rowi] = r;
    }
  };
  if (__any(people)) {
    const bool live = lane_live && people;
    // a7 agent angle
    {
      double r = 0.0, gth = 0.0;
      const double aa_target = (c.lds + c.L.lanec)[2 * T + tl];
      if (aa_target != kNoTarget) {
        const double ad = wrap_angle(th1 - aa_target);
        r = SPRM(agent_angle_w) * (ad * ad);
        gth = SPRM(agent_angle_w) * 2.0 * ad;
      }
      if (kRows) emit(0, live, people, r, 0.0, 0.0, gth, 0.0);
      else {  // (a slot without people beside one with people has no steering target: r = gth = 0 already)
        Att = fma(gth, gth, Att); bt = fma(gth, r, bt); cc = fma(r, r, cc);
      }
    }
    // a3 social work (finished inside the agent block above; zero for a slot without people)
    {
      const double r = sw_r, gx = sw_gx, gy = sw_gy, gt = sw_gt, gv = sw_gv;
      if (kRows) emit(1, live, people, r, gx, gy, gt, gv);
      else {
        Axx = fma(gx, gx, Axx); Axy = fma(gx, gy, Axy); Axt = fma(gx, gt, Axt); Axv = fma(gx, gv, Axv);
        Ayy = fma(gy, gy, Ayy); Ayt = fma(gy, gt, Ayt); Ayv = fma(gy, gv, Ayv);
        Att = fma(gt, gt, Att); Atv = fma(gt, gv, Atv); Avv = fma(gv, gv, Avv);
        bx = fma(gx, r, bx); by = fma(gy, r, by); bt = fma(gt, r, bt); bv = fma(gv, r, bv); cc = fma(r, r, cc);
      }
    }
    // a4 proxemics: w alpha exp(-min_a d^2 / d0^2) over valid agents
    {
      const double e = 3.0 * exp_tab(&k.mt, -pbest / (0.5 * 0.5));
      double r = SPRM(proxemics_w) * e;
      double gx = r * (-2.0 * pdx / (0.5 * 0.5)), gy = r * (-2.0 * pdy / (0.5 * 0.5));
      if (people && pbest == 1.7976931348623157e308) {
        // no valid agent: the reference's dual evaluation gives (-max / d0^2) = -inf and inf * 0 = NaN tangents
        // (critics/proxemics_cost_function.hpp:127,147) -> Ceres rejects the evaluation. Mirror it.
        gx = gy = __longlong_as_double(0x7ff8000000000000ll);
      }
      if (kRows) emit(2, live, people, r, gx, gy, 0.0, 0.0);
      else {  // (a slot without people: pbest is still the largest double, exp gives r = 0 and with it gx = gy = 0)
        Axx = fma(gx, gx, Axx); Axy = fma(gx, gy, Axy); Ayy = fma(gy, gy, Ayy);
        bx = fma(gx, r, bx); by = fma(gy, r, by); cc = fma(r, r, cc);
      }
    }
  }
  SMPC_STAMP2(c, 0);  // people critics (agent angle, social combine, proxemics)
  const int o5 = people ? 3 : 0;
  // a6 velocity
  {
    double r = 0.0, gv = 0.0;
    if (sl < CH) { const double d = SPRM(desired_linear_vel) - vb; r = SPRM(velocity_w) * d * d; gv = -2.0 * SPRM(velocity_w) * d; }
    if (kRows) emit(o5 + 0, lane_live, true, r, 0.0, 0.0, 0.0, gv);
    else { Avv = fma(gv, gv, Avv); bv = fma(gv, r, bv); cc = fma(r, r, cc); }
  }
  // a8 goal align
  {
    const double a = wrap_angle(cst[3] - th1);
    const double r = SPRM(goal_align_w) * a * a, gth = -2.0 * SPRM(goal_align_w) * a;
    if (kRows) emit(o5 + 1, lane_live, true, r, 0.0, 0.0, gth, 0.0);
    else { Att = fma(gth, gth, Att); bt = fma(gth, r, bt); cc = fma(r, r, cc); }
  }
  // a2 distance (path follow -> final point; path align -> point sl+1)
  {
    const double ddx = X - cst[6], ddy = Y - cst[7], q2 = ddx * ddx + ddy * ddy;
    const double r = SPRM(distance_w) * q2 * q2, gx = 4.0 * SPRM(distance_w) * q2 * ddx, gy = 4.0 * SPRM(distance_w) * q2 * ddy;
    if (kRows) emit(o5 + 2, lane_live, true, r, gx, gy, 0.0, 0.0);
    else {
      Axx = fma(gx, gx, Axx); Axy = fma(gx, gy, Axy); Ayy = fma(gy, gy, Ayy);
      bx = fma(gx, r, bx); by = fma(gy, r, by); cc = fma(r, r, cc);
    }
  }
  {
    const double* lanec = c.lds + c.L.lanec;
    const double ddx = X - lanec[tl], ddy = Y - lanec[T + tl], q2 = ddx * ddx + ddy * ddy;
    const double r = SPRM(angle_w) * q2 * q2, gx = 4.0 * SPRM(angle_w) * q2 * ddx, gy = 4.0 * SPRM(angle_w) * q2 * ddy;
    if (kRows) emit(o5 + 3, lane_live, true, r, gx, gy, 0.0, 0.0);
    else {
      Axx = fma(gx, gx, Axx); Axy = fma(gx, gy, Axy); Ayy = fma(gy, gy, Ayy);
      bx = fma(gx, r, bx); by = fma(gy, r, by); cc = fma(r, r, cc);
    }
  }
  SMPC_STAMP2(c, 1);  // velocity, goal, 2 x distance
  // a5 obstacle
  {
    const double inv_res = k.inv_resolution;
    // the same expressions as at the fetch (recomputed rather than kept in registers across the agent loop)
    const double ob_ic = (X + 0.25 * c1 - cst[4]) * inv_res, ob_ir = (Y + 0.25 * s1 - cst[5]) * inv_res;
    double f, dfdr, dfdc;
    if (patch_interior) bicubic_eval<true>(patch, k.size_x, ob_ir, ob_ic, f, dfdr, dfdc);
    else if (wide_map) bicubic_eval<false>(patch, k.size_x, ob_ir, ob_ic, f, dfdr, dfdc);
    else bicubic(c.map, k.size_x, k.size_y, ob_ir, ob_ic, f, dfdr, dfdc);  // maps narrower than one patch: byte by byte
    const double r = SPRM(obstacle_w) * f;
    const double gx = SPRM(obstacle_w) * dfdc * inv_res, gy = SPRM(obstacle_w) * dfdr * inv_res;
    const double gth = SPRM(obstacle_w) * (dfdc * (-0.25 * s1) + dfdr * (0.25 * c1)) * inv_res;
    if (kRows) emit(o5 + 4, lane_live, true, r, gx, gy, gth, 0.0);
    else {
      Axx = fma(gx, gx, Axx); Axy = fma(gx, gy, Axy); Axt = fma(gx, gth, Axt);
      Ayy = fma(gy, gy, Ayy); Ayt = fma(gy, gth, Ayt); Att = fma(gth, gth, Att);
      bx = fma(gx, r, bx); by = fma(gy, r, by); bt = fma(gth, r, bt); cc = fma(r, r, cc);
    }
  }
  SMPC_STAMP2(c, 2);  // obstacle (bicubic gather)
  GramView view;
  double* gt = c.lds + c.L.gram;
  view.base = gt;
  view.ld = Q;
  if (kRows) {
    // a9 velocity feasibility between blocks sl and sl-1 (src/optimizer.cpp:364-370); the row follows step sl
    if (Shape::nfeas(k) > 0) {
      const bool live = lane_live && sl >= 1 && sl <= hz.nfeas;
      double row[P];
#pragma unroll
      for (int q = 0; q < P; ++q) row[q] = 0.0;
      double r = 0.0;
#pragma unroll
      for (int q = 1; q < NB; ++q) {
        if (q == sl) {
          const double lin = xp[2 * q] - xp[2 * q - 2], ang = xp[2 * q + 1] - xp[2 * q - 1];
          r = SPRM(velocity_feasibility_w) * lin * lin + SPRM(velocity_feasibility_w) * ang * ang;
          row[2 * q] = 2.0 * SPRM(velocity_feasibility_w) * lin;
          row[2 * q - 2] = -2.0 * SPRM(velocity_feasibility_w) * lin;
          row[2 * q + 1] = 2.0 * SPRM(velocity_feasibility_w) * ang;
          row[2 * q - 1] = -2.0 * SPRM(velocity_feasibility_w) * ang;
        }
      }
      if (live) {
        const int rowi = critic_major ? rows_per_step * T + (sl - 1) : row_base + rows_per_step;
        if (out_r) out_r[rowi] = r;
        if (out_J) {
#pragma unroll
          for (int q = 0; q < P; ++q) out_J[(size_t)rowi * P + q] = row[q];
        }
      }
      {
        const double rl = live ? r : 0.0;
#pragma unroll
        for (int q = 0; q < P; ++q) gcol[q] = fma(live ? row[q] : 0.0, rl, gcol[q]);
        gcol[P] = fma(rl, rl, gcol[P]);
      }
    }
#pragma unroll
    for (int a = 0; a < Q; ++a) {
      const double v = slot_sum<W>(gcol[a]);
      gt[a * Q + P] = v;
      gt[P * Q + a] = v;
    }
  } else {
    compute_sensitivities();
    // ---- the lane's share of the Gram: H = M^T A M, g = M^T b, cc; summed over the slot's lanes through LDS.
    if (!lane_live) {  // lanes beyond the horizon carry nothing (their A may hold anything, NaN included)
      Axx = Axy = Axt = Axv = Ayy = Ayt = Ayv = Att = Atv = Avv = 0.0;
      bx = by = bt = bv = cc = 0.0;
    }
    // a9 velocity feasibility rows (src/optimizer.cpp:364-370): row q (between blocks q and q-1, 1 <= q <= nfeas) has
    // four non-zero entries; the rows go to LDS as they are and their outer products are added after the lane sum.
    double* frow = c.wave_lds + c.slot * ((NB > 1 ? NB - 1 : 1) * Q);
    if (sl >= 1 && sl <= hz.nfeas) {
      const double lin = xp[2 * sl] - xp[2 * sl - 2], ang = xp[2 * sl + 1] - xp[2 * sl - 1];
      const double wf = SPRM(velocity_feasibility_w);
      double* fr = frow + (sl - 1) * Q;
#pragma unroll
      for (int q = 0; q < Q; ++q) fr[q] = 0.0;
      fr[2 * sl - 2] = -2.0 * wf * lin; fr[2 * sl - 1] = -2.0 * wf * ang;
      fr[2 * sl] = 2.0 * wf * lin; fr[2 * sl + 1] = 2.0 * wf * ang;
      fr[P] = wf * lin * lin + wf * ang * ang;
    }
    double* red_base = c.lds + c.L.cs;  // over the cos / sin block and the scans (dead by now) and the tail behind them
    double* red = red_base + sl * (kGramChunk + 1);
    double hv[kGramChunk];
    int cnt = 0, chunk_base = 0;  // compile-time after unrolling
    auto flush = [&](int n, int base, int col_lo, int col_hi) {
      wave_lds_fence();  // the previous chunk's sums have been read
#pragma unroll
      for (int i = 0; i < kGramChunk; ++i) if (i < n) red[i] = hv[i];
      wave_lds_fence();
      // two levels: lane (part, v) = (sl / 16, sl % 16) adds up value v of the 16 lanes of its part, then the W / 16
      // parts are combined by butterfly shuffles — W / 16 times fewer additions per lane than one lane per value
      const int vsel = sl & (kGramChunk - 1), part = sl / kGramChunk;
      double tot = 0.0;
      {
        const double* col = red_base + (part * kGramChunk) * (kGramChunk + 1) + vsel;
#pragma unroll
        for (int l = 0; l < kGramChunk; ++l) tot += col[l * (kGramChunk + 1)];
      }
#pragma unroll
      for (int off = kGramChunk; off < W; off <<= 1) tot += __shfl_xor(tot, off, W);
      if (sl < n) {
        // packed (column-major upper triangle) index -> (a, b)
        const int pidx = base + sl;
        int bcol = col_lo;
#pragma unroll
        for (int cb = 1; cb < Q; ++cb) if (cb > col_lo && cb <= col_hi) bcol = (pidx >= cb * (cb + 1) / 2) ? cb : bcol;
        const int arow = pidx - bcol * (bcol + 1) / 2;
        for (int q = 0; q < hz.nfeas; ++q) tot = fma(frow[q * Q + arow], frow[q * Q + bcol], tot);
        gt[arow * Q + bcol] = tot;
        gt[bcol * Q + arow] = tot;
      }
    };
    int col_lo = 0;
    auto column = [&](int bq) {  // column bq of [J r]: 2q = v_q, 2q+1 = w_q, P = r; entries 0 .. bq (upper triangle)
      double Wx, Wy, Wt, Wv;  // column bq of A M (for bq = P: b itself)
      if (bq == P) { Wx = bx; Wy = by; Wt = bt; Wv = bv; }
      else if ((bq & 1) == 0) {
        const int q = bq >> 1;
        const double mq = (q == myb) ? 1.0 : 0.0;
        Wx = fma(Axx, Sxv[q], fma(Axy, Syv[q], Axv * mq));
        Wy = fma(Axy, Sxv[q], fma(Ayy, Syv[q], Ayv * mq));
        Wt = fma(Axt, Sxv[q], fma(Ayt, Syv[q], Atv * mq));
        Wv = fma(Axv, Sxv[q], fma(Ayv, Syv[q], Avv * mq));
      } else {
        const int q = bq >> 1;
        Wx = fma(Axx, Sxw[q], fma(Axy, Syw[q], Axt * Sthw[q]));
        Wy = fma(Axy, Sxw[q], fma(Ayy, Syw[q], Ayt * Sthw[q]));
        Wt = fma(Axt, Sxw[q], fma(Ayt, Syw[q], Att * Sthw[q]));
        Wv = fma(Axv, Sxw[q], fma(Ayv, Syw[q], Atv * Sthw[q]));
      }
#pragma unroll
      for (int aq = 0; aq <= bq; ++aq) {
        double h;
        if (aq == P) h = cc;
        else if ((aq & 1) == 0) {
          const int q = aq >> 1;
          const double mq = (q == myb) ? 1.0 : 0.0;
          h = fma(Sxv[q], Wx, fma(Syv[q], Wy, mq * Wv));
        } else {
          const int q = aq >> 1;
          h = fma(Sxw[q], Wx, fma(Syw[q], Wy, Sthw[q] * Wt));
        }
        if (cnt == 0) col_lo = bq;
        hv[cnt++] = h;
        if (cnt == kGramChunk) { flush(cnt, chunk_base, col_lo, bq); chunk_base += cnt; cnt = 0; }  // a full chunk
      }
    };
    // the last column first: gradient and cost, enough for a line-search sample that fails the Armijo test
    chunk_base = P * (P + 1) / 2;
    column(P);
    if (cnt > 0) { flush(cnt, chunk_base, col_lo, P); cnt = 0; }
    wave_lds_fence();
    c.gram_full = __any(need_rest());
    if (c.gram_full) {
      chunk_base = 0;
#pragma unroll
      for (int bq = 0; bq < P; ++bq) column(bq);
      if (cnt > 0) flush(cnt, chunk_base, col_lo, P - 1);
    }
  }
  wave_lds_fence();  // Gram visible to every lane of the slot; the cos/sin block may be rewritten by the next sweep
  SMPC_STAMP(c, 5);
  return view;
#undef SPRM
#undef SMPC_PAIR_NEAREST
#undef SMPC_PAIR_ADD
}

// A sweep result is usable iff every residual and Jacobian entry was finite: a non-finite entry makes the
// corresponding diagonal entry of the Gram (a sum of squares) non-finite.
template <int P> __device__ inline bool gram_finite(const GramView& g) {
  bool ok = true;
#pragma unroll
  for (int q = 0; q <= P; ++q) ok = ok && isfinite(g(q, q));
  return ok;
}

}  // namespace smpc
