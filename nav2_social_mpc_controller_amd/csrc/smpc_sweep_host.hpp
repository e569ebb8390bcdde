// smpc_sweep_host.hpp — the host side of a launch of the sweep kernels (solve, K1) and of the staging pass: the checks of a
// scene batch, the plan of the call (smpc_plan.hpp) from the handle, plan -> kernel function, the launch parameters, the
// people block, the launch itself, and sweep_call(), the one course both smpc_solve_batch and smpc_eval_batch take.
#pragma once

#include <cmath>
#include <cstdio>

#include "../../include/smpc_fixed_shapes.h"
#include "smpc_eval_kernel.hpp"
#include "smpc_host.hpp"
#include "smpc_plan.hpp"
#include "smpc_solve_kernel.hpp"
#include "smpc_stage_kernel.hpp"

namespace smpc {
// n rows of smpc_scene_params, all equal to `row` (neutral_rows(), below)
__global__ void smpc_fill_scene_params_kernel(smpc_scene_params* rows, int n, const smpc_scene_params row) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) rows[i] = row;
}
}  // namespace smpc

namespace {

using smpc::Sweep;

struct Dims { int CH, bl, nb, P, M, nbounded, nfeas; };

Dims make_dims(const smpc_params& p, int T, bool has_people) {
  Dims d;
  d.CH = p.control_horizon < T ? p.control_horizon : T;                 // src/optimizer.cpp:248
  d.bl = p.parameter_block_length < d.CH ? p.parameter_block_length : d.CH;  // :249
  if (d.bl < 1) d.bl = 1;
  d.nb = (d.CH - 1) / d.bl + 1;
  d.P = 2 * d.nb;
  d.nbounded = d.CH / d.bl;                                             // :373
  int nf = (d.CH / d.bl < T ? d.CH / d.bl : T) - 1;                      // :364
  d.nfeas = nf > 0 ? nf : 0;
  d.M = (has_people ? 8 : 5) * T + d.nfeas;
  return d;
}

// The plan of a launch of `kind` on this handle (smpc_scene_batch.T_scene / .scene_params: vt, sp).
smpc::SweepPlan plan_for(const smpc_handle* h, Sweep kind, int B, int T, int N, const Dims& d, bool vt, bool sp, const smpc::Knobs& kn) {
  return smpc::plan_sweep({kind, B, T, N, d.CH, d.bl, d.nb, vt, sp, h->num_cu, h->share, h->fixed_shapes}, kn);
}

// ---- plan -> kernel function ----
using KernelFn = void (*)(const smpc::KParams);

template <int NB, int W, bool kVT, bool kSP> KernelFn pick_fn(Sweep kind) {
  return kind == Sweep::Eval ? smpc::smpc_eval_kernel<NB, W, kVT, kSP> : smpc::smpc_solve_kernel<NB, W, kVT, kSP>;
}

template <int NB> KernelFn pick_w(int W, Sweep kind, bool vt, bool sp) {
  if (kind == Sweep::Trace) return W == 32 ? smpc::smpc_solve_kernel<NB, 32, true, true, true> : smpc::smpc_solve_kernel<NB, 64, true, true, true>;
  if (W == 32) return sp ? pick_fn<NB, 32, true, true>(kind) : vt ? pick_fn<NB, 32, true, false>(kind) : pick_fn<NB, 32, false, false>(kind);
  return sp ? pick_fn<NB, 64, true, true>(kind) : vt ? pick_fn<NB, 64, true, false>(kind) : pick_fn<NB, 64, false, false>(kind);
}

KernelFn pick(int nb, int W, Sweep kind, bool vt, bool sp) {
#ifdef SMPC_ONLY_NB  // development builds: one instantiation only (seconds instead of a minute to compile)
  return nb == SMPC_ONLY_NB ? pick_w<SMPC_ONLY_NB>(W, kind, vt, sp) : nullptr;
#else
  switch (nb) {
    case 1: return pick_w<1>(W, kind, vt, sp);
    case 2: return pick_w<2>(W, kind, vt, sp);
    case 3: return pick_w<3>(W, kind, vt, sp);
    case 4: return pick_w<4>(W, kind, vt, sp);
    case 5: return pick_w<5>(W, kind, vt, sp);
    case 6: return pick_w<6>(W, kind, vt, sp);
    case 7: return pick_w<7>(W, kind, vt, sp);
    case 8: return pick_w<8>(W, kind, vt, sp);
    case 9: return pick_w<9>(W, kind, vt, sp);
    case 10: return pick_w<10>(W, kind, vt, sp);
    default: return nullptr;
  }
#endif
}

template <class Shape> KernelFn fixed_fn(Sweep kind) {
#ifdef SMPC_ONLY_NB
  if constexpr (Shape::kNB != SMPC_ONLY_NB) return nullptr; else
#endif
  return kind == Sweep::Eval ? smpc::smpc_eval_fixed_kernel<Shape> : smpc::smpc_solve_fixed_kernel<Shape>;
}

// The kernels of shape `index` of SMPC_FIXED_SHAPES (the rule that gives the index: plan_sweep(); here only the table)
KernelFn pick_fixed(int index, Sweep kind) {
  int i = 0;
#define SMPC_X(t, n, ch, b) \
  if (index == i++) return fixed_fn<smpc::FixedShape<t, n, ch, b>>(kind);
  SMPC_FIXED_SHAPES(SMPC_X)
#undef SMPC_X
  return nullptr;
}

// The kernel a plan's launch runs; null only for an nb without kernels (validate() refuses those).
KernelFn kernel_of(const smpc::SweepPlan& p) {
  return p.fixed >= 0 ? pick_fixed(p.fixed, p.kind) : pick(p.nb, p.W, p.kind, p.vt, p.sp);
}

int validate(const smpc_handle* h, const smpc_scene_batch* sb, Dims* d) {
  if (!h || !sb) { set_error("null handle or scene batch"); return SMPC_ERR_INVALID_ARG; }
  if (sb->B < 0 || sb->T < 1 || sb->N < 0) { set_error("bad B/T/N"); return SMPC_ERR_INVALID_ARG; }
  if (h->prm.control_horizon < 1 || h->prm.parameter_block_length < 1) { set_error("control_horizon and parameter_block_length must be >= 1"); return SMPC_ERR_INVALID_ARG; }
  if (!sb->pose0 || !sb->init_params || !sb->path_pts || !sb->goal_yaw || !sb->costmap || !sb->costmap_origin) { set_error("null input array"); return SMPC_ERR_INVALID_ARG; }
  if ((sb->people_records != nullptr) != (sb->people_aux != nullptr)) { set_error("people_records and people_aux go together"); return SMPC_ERR_INVALID_ARG; }
  if (sb->N > 0 && !sb->people && !sb->people_records) { set_error("people is null with N > 0"); return SMPC_ERR_INVALID_ARG; }
  if (sb->size_x < 1 || sb->size_y < 1 || !(sb->resolution > 0.0)) { set_error("bad costmap geometry"); return SMPC_ERR_INVALID_ARG; }
  *d = make_dims(h->prm, sb->T, true);
  if (sb->T + 1 > smpc::kWave) { set_error("T + 1 > 64 rollout poses is not supported by the one-wave-per-scene mapping"); return SMPC_ERR_UNSUPPORTED; }
  if (sb->N > smpc::kWave) { set_error("N > 64 agents is not supported"); return SMPC_ERR_UNSUPPORTED; }
  if (!smpc::nb_has_kernels(d->nb)) { set_error("more than SMPC_MAX_BLOCKS parameter blocks (nb must be 1..10)"); return SMPC_ERR_UNSUPPORTED; }
  return SMPC_OK;
}

void fill_kparams(const smpc_handle* h, const smpc_scene_batch* sb, const Dims& d, const smpc::SweepPlan& plan, smpc::KParams* k) {
  std::memset(k, 0, sizeof(*k));
  k->B = sb->B; k->T = sb->T; k->N = sb->N;
  k->CH = d.CH; k->bl = d.bl; k->nb = d.nb; k->P = d.P; k->nbounded = d.nbounded; k->nfeas = d.nfeas;
  k->size_x = sb->size_x; k->size_y = sb->size_y; k->costmap_shared = sb->costmap_shared;
  k->dt = sb->dt; k->resolution = sb->resolution; k->inv_resolution = 1.0 / sb->resolution;
  k->prm = h->prm;
  k->e_M = d.M;
  k->hp_A = plan.hp_A;
  smpc::fill_math_table(&k->mt);
  smpc::fill_atan_nodes(&k->an);
}

// Room in LDS for a launch of `fn` with `shmem` dynamic bytes, or the refusal `too_large`.
int reserve_lds(KernelFn fn, size_t shmem, const char* too_large) {
  if (shmem > 160 * 1024) { set_error(too_large); return SMPC_ERR_UNSUPPORTED; }
  if (shmem > 64 * 1024) SMPC_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem));
  return SMPC_OK;
}

// The staging pass: k.people (+ pose0, has_people) -> records / aux at the given device pointers (in its own copy of k).
int launch_stage(smpc_handle* h, const smpc::KParams& k, double* rec, double* aux) {
  if (k.B == 0 || k.N == 0) return SMPC_OK;
  const smpc::StagePlan plan = smpc::plan_stage(k.T, k.N);
  KernelFn fn = (plan.W == 32) ? smpc::smpc_stage_kernel<32> : smpc::smpc_stage_kernel<64>;
  SMPC_TRY(reserve_lds(fn, plan.shmem, "people block does not fit the 160 KiB LDS of one CU"));
  smpc::KParams ks = k;
  ks.stage_rec = rec; ks.stage_aux = aux;
  hipLaunchKernelGGL(fn, dim3((k.B + plan.S - 1) / plan.S), dim3(smpc::kWave), plan.shmem, h->stream, ks);
  SMPC_HIP_CHECK(hipGetLastError());
  return SMPC_OK;
}

// Makes the people block of the plan's launch readable by its kernel: the caller's staged block; or, where the kernel
// stages each scene as it fetches it (plan.stages: the fixed-shape solve kernel), room for the records and
// k.stage_at_fetch — no staging kernel, no aux array, and smpc_last_kernel_ms() then covers the staging; or the
// library's own staging pass into the handle's buffers (timed separately: smpc_last_kernel_ms() reports the solve /
// sweep kernel alone).
int bind_people(smpc_handle* h, const smpc_scene_batch* sb, const smpc::SweepPlan& plan, smpc::KParams& k, Staging* st) {
  if (sb->N == 0) return SMPC_OK;
  const size_t nrec = (size_t)sb->B * sb->N * sb->T * 4, naux = (size_t)sb->B * sb->T * 2;
  if (sb->people_records) {
    SMPC_TRY(st->in(k.people_rec, sb->people_records, nrec));
    return st->in(k.people_aux, sb->people_aux, naux);
  }
  SMPC_TRY(grow(&h->stage_rec, &h->stage_rec_bytes, nrec * sizeof(double), h->stream));
  if (plan.stages) {
    k.stage_at_fetch = 1;
    k.stage_rec = h->stage_rec;
    k.people_rec = h->stage_rec;
    return SMPC_OK;
  }
  SMPC_TRY(grow(&h->stage_aux, &h->stage_aux_bytes, naux * sizeof(double), h->stream));
  SMPC_TRY(st->flush_up());
  SMPC_TRY(launch_stage(h, k, h->stage_rec, h->stage_aux));
  k.people_rec = h->stage_rec; k.people_aux = h->stage_aux;
  return SMPC_OK;
}

// Diagnostic build: per-wave phase cycle sums, dumped to stderr after the launch.
#ifdef SMPC_STAMPS
int stamps_attach(smpc::KParams& k, int grid) {
  static unsigned long long* d_stamps = nullptr; static int cap = 0;
  if (grid > cap) { if (d_stamps) (void)hipFree(d_stamps); SMPC_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&d_stamps), (size_t)grid * 12 * sizeof(unsigned long long))); cap = grid; }
  k.stamps = d_stamps;
  return SMPC_OK;
}

int stamps_dump(smpc_handle* h, const smpc::KParams& k, int grid, bool eval) {
  SMPC_HIP_CHECK(hipStreamSynchronize(h->stream));
  std::vector<unsigned long long> hs((size_t)grid * 12);
  SMPC_HIP_CHECK(hipMemcpy(hs.data(), k.stamps, hs.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  double tot[12] = {0};
  for (int g = 0; g < grid; ++g) for (int i = 0; i < 12; ++i) tot[i] += (double)hs[(size_t)g * 12 + i];
  double all = 0; for (int i = 0; i < 8; ++i) all += tot[i];
  static const char* names[8] = {"fetch+load_scene", "theta+sincos", "xy-loop", "agent-loop", "sens-loop", "critics+gram", "lm+output", "ls-interpolation"};
  std::fprintf(stderr, "[stamps %s] grid=%d mean cycles/wave=%.0f:", eval ? "K1" : "solve", grid, all / grid);
  for (int i = 0; i < 8; ++i) std::fprintf(stderr, " %s=%.1f%%", names[i], 100.0 * tot[i] / all);
  std::fprintf(stderr, " | rows split: people-critics=%.1f%% vel/goal/dist=%.1f%% obstacle=%.1f%% (rest of rows = feas + gram out)\n",
               100.0 * tot[8] / all, 100.0 * tot[9] / all, 100.0 * tot[10] / all);
  if (!eval) {
    unsigned long long dbg[8] = {0};
    (void)hipMemcpyFromSymbol(dbg, HIP_SYMBOL(smpc::g_ls_dbg), sizeof(dbg));
    std::fprintf(stderr, "[ls counters, cumulative] root4 calls %llu trips %llu | root3 calls %llu trips %llu | cubic fits %llu quintic fits %llu "
                 "(monotone shortcut %llu) generic fallback %llu\n", dbg[0], dbg[1], dbg[2], dbg[3], dbg[4], dbg[5], dbg[6], dbg[7]);
  }
  return SMPC_OK;
}
#else
inline int stamps_attach(smpc::KParams&, int) { return SMPC_OK; }
inline int stamps_dump(smpc_handle*, const smpc::KParams&, int, bool) { return SMPC_OK; }
#endif

// The plan's launch. Sweep::Trace: the solve kernel that also writes k.o_trace / k.o_trace_n (k.scene_params is set by then)
int launch(smpc_handle* h, Staging& st, const smpc::SweepPlan& plan, const smpc::Knobs& kn, smpc::KParams& k) {
  const bool eval = plan.kind == Sweep::Eval;
  const int S = plan.S;
  const size_t shmem = plan.shmem;
  KernelFn fn = kernel_of(plan);
  SMPC_TRY(reserve_lds(fn, shmem, "scene does not fit the 160 KiB LDS of one CU"));
  if (k.B == 0) return SMPC_OK;
  int grid = (k.B + S - 1) / S;
  if (!eval) {
    // persistent sweep engine: no more waves than can be resident; scenes come from the queue
    int per_cu = 0;
    SMPC_HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, reinterpret_cast<const void*>(fn), smpc::kWave, shmem));
    if (h->share > 1) per_cu /= h->share;  // room for the other launches of smpc_set_solve_share
    if (per_cu < 1) per_cu = 1;
    if (kn.max_waves_per_cu && kn.max_waves_per_cu < per_cu) per_cu = kn.max_waves_per_cu;
    if (kn.debug_grid) std::fprintf(stderr, "[smpc] solve kernel: %zu B LDS per wave, %d waves per CU\n", shmem, per_cu);
    const int resident = per_cu * h->num_cu;
    // A launch alone on the GPU finishes soonest with two waves per SIMD (two scenes per slot at the headline batch:
    // a third wave per SIMD lengthens every trip more than it shortens the queue, and the tail of long scenes grows);
    // the third wave's registers and LDS then stay free for the launches of other streams, which is where the extra
    // occupancy pays. Only a batch with many scenes per slot takes every resident wave for itself.
    const int two_per_simd = kn.lone_waves_per_cu * h->num_cu < resident ? kn.lone_waves_per_cu * h->num_cu : resident;
    if (grid > two_per_simd) grid = (grid >= 4 * resident) ? resident : two_per_simd;
    k.queue = h->queue;
    k.full_gram = kn.full_gram ? 1 : 0;
    k.prio_step = kn.prio_step;
    k.lone_trips = (kn.no_lone_help ? 0 : smpc::kLoneHelp) | (kn.debug_grid ? smpc::kLoneCount : 0);
    // the trip counters behind the scene counter are zeroed only for the launch that reports them: every other launch
    // issues the one four-byte memset it always issued (the captured tick graphs of the sharded episodes hold this node)
    if (kn.debug_grid) SMPC_HIP_CHECK(hipMemsetAsync(h->queue + 1, 0, (smpc::kQueueWords - 1) * sizeof(int), h->stream));
    SMPC_HIP_CHECK(hipMemsetAsync(h->queue, 0, sizeof(int), h->stream));
  }
  SMPC_TRY(stamps_attach(k, grid));
  SMPC_TRY(st.timed([&] { hipLaunchKernelGGL(fn, dim3(grid), dim3(smpc::kWave), shmem, h->stream, k); return SMPC_OK; }));
  if (kn.debug_grid && !eval) {  // what the kernel counted (zeros from a kernel without lone trips, lone_trip_kernel())
    int words[smpc::kQueueWords];
    SMPC_HIP_CHECK(hipStreamSynchronize(h->stream));
    SMPC_HIP_CHECK(hipMemcpy(words, h->queue, sizeof(words), hipMemcpyDeviceToHost));
    std::fprintf(stderr, "[smpc] solve kernel: %d trips, %d with one slot idle for good, %d helped\n", words[2], words[1], words[3]);
  }
  return stamps_dump(h, k, grid, eval);
}

// Host rows of smpc_scene_batch.scene_params: every value finite, v_min <= v_max, w_min <= w_max.
int check_scene_params(const smpc_scene_params* sp, size_t B) {
  for (size_t i = 0; i < B; ++i) {
    const double* v = reinterpret_cast<const double*>(sp + i);
    for (int j = 0; j < smpc::kSceneParamDoubles; ++j)
      if (!std::isfinite(v[j])) { set_error("scene_params[" + std::to_string(i) + "]: every value must be finite"); return SMPC_ERR_INVALID_ARG; }
    if (!(sp[i].v_min <= sp[i].v_max) || !(sp[i].w_min <= sp[i].w_max)) {
      set_error("scene_params[" + std::to_string(i) + "]: needs v_min <= v_max and w_min <= w_max"); return SMPC_ERR_INVALID_ARG;
    }
  }
  return SMPC_OK;
}

// k.scene_params for a trace solve of a batch that brings none: B rows of the handle's own values in device memory.
int neutral_rows(smpc_handle* h, smpc::KParams& k) {
  const size_t have = h->neutral_sp_bytes, need = (size_t)k.B * sizeof(smpc_scene_params);
  if (need > have) {
    SMPC_TRY(grow(&h->neutral_sp, &h->neutral_sp_bytes, need + need / 4, h->stream));
    const smpc_params& p = h->prm;
    const smpc_scene_params row = {p.distance_w, p.socialwork_w, p.velocity_w, p.angle_w, p.agent_angle_w, p.proxemics_w,
                                   p.velocity_feasibility_w, p.obstacle_w, p.goal_align_w, p.desired_linear_vel,
                                   p.v_min, p.v_max, p.w_min, p.w_max};
    const int n = (int)(h->neutral_sp_bytes / sizeof(smpc_scene_params));
    hipLaunchKernelGGL(smpc::smpc_fill_scene_params_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream,
                       reinterpret_cast<smpc_scene_params*>(h->neutral_sp), n, row);
    SMPC_HIP_CHECK(hipGetLastError());
    // the rows outlive this call, and a later one may run on another stream (smpc_set_stream): written before they are kept
    SMPC_HIP_CHECK(hipStreamSynchronize(h->stream));
  }
  k.scene_params = reinterpret_cast<const smpc_scene_params*>(h->neutral_sp);
  return SMPC_OK;
}

int bind_inputs(const smpc_scene_batch* sb, const Dims& d, smpc::KParams* k, Staging* st) {
  const size_t B = sb->B, T = sb->T, N = sb->N;
  const size_t nmaps = sb->costmap_shared ? 1 : B;
  // host rows are checked here; device arrays are trusted (the caller's responsibility, include/smpc.h: the kernel
  // clamps every T_scene entry into 1..T)
  if (!sb->on_device && sb->T_scene)
    for (size_t i = 0; i < B; ++i)
      if (sb->T_scene[i] < 1 || sb->T_scene[i] > sb->T) { set_error("T_scene entries must lie in 1..T"); return SMPC_ERR_INVALID_ARG; }
  if (!sb->on_device && sb->scene_params) SMPC_TRY(check_scene_params(sb->scene_params, B));
  SMPC_TRY(st->in(k->T_scene, sb->T_scene, B));
  SMPC_TRY(st->in(k->scene_params, sb->scene_params, B));
  SMPC_TRY(st->in(k->pose0, sb->pose0, B * 3));
  SMPC_TRY(st->in(k->init_params, sb->init_params, B * d.P));
  SMPC_TRY(st->in(k->path_pts, sb->path_pts, B * (T + 1) * 2));
  SMPC_TRY(st->in(k->goal_yaw, sb->goal_yaw, B));
  if (!sb->people_records) SMPC_TRY(st->in(k->people, sb->people, B * (T + 1) * 6 * N));  // else read by no kernel
  SMPC_TRY(st->in(k->has_people, sb->has_people, B));
  SMPC_TRY(st->in(k->costmap, sb->costmap, nmaps * (size_t)sb->size_x * sb->size_y));
  return st->in(k->costmap_origin, sb->costmap_origin, nmaps * 2);
}

// The course of smpc_solve_batch / smpc_solve_trace_batch / smpc_eval_batch: the batch is checked, then the entry point's
// own arguments (bad_args: the refusal's text, or null), the plan is made, the scene arrays and the people block are bound,
// `own(d, k, st)` binds the entry point's own arrays, and the plan's kernel runs.
template <typename F> int sweep_call(smpc_handle* h, const smpc_scene_batch* sb, Sweep kind, const char* bad_args, F&& own) {
  Dims d;
  SMPC_TRY(validate(h, sb, &d));
  if (bad_args) { set_error(bad_args); return SMPC_ERR_INVALID_ARG; }
  SMPC_HIP_CHECK(hipSetDevice(h->device));
  const smpc::Knobs kn = smpc::read_knobs();
  const smpc::SweepPlan plan = plan_for(h, kind, sb->B, sb->T, sb->N, d, sb->T_scene != nullptr, sb->scene_params != nullptr, kn);
  smpc::KParams k;
  fill_kparams(h, sb, d, plan, &k);
  Staging st(h, sb->on_device);
  SMPC_TRY(bind_inputs(sb, d, &k, &st));
  SMPC_TRY(bind_people(h, sb, plan, k, &st));
  SMPC_TRY(own(d, k, st));
  SMPC_TRY(launch(h, st, plan, kn, k));
  return st.finish();
}

}  // namespace
