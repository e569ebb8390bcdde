// smpc_hip.hip — the C ABI of include/smpc.h (libsmpc_hip.so): the entry points, one translation unit with the kernels
// and the host code they include. gfx950 only, no CPU fallback.
//
// Host side: smpc_host.hpp (the handle, errors, the staging of host-pointer calls), smpc_plan.hpp (what a sweep launch
// will be: width, variant, fixed shape, LDS; pure host code), smpc_sweep_host.hpp (checks, plan -> kernel, the launch).
// Kernels (one 64-lane wavefront per workgroup, split into 64/W scene slots; lane mapping and LDS layout: smpc_launch.hpp):
//   smpc_solve_kernel<NB,W,kVT,kSP,kTrace>  persistent sweep engine: whole ceres::Solve-equivalent (reference
//                            src/optimizer.cpp:241-446) per scene, LM state resident in registers / LDS for all
//                            <= max_iterations iterations, scenes pulled from a device-side queue (smpc_solve_kernel.hpp);
//                            kTrace (<NB,W,true,true,true> only): one row per LM iteration as well (smpc_solve_trace_batch);
//   smpc_eval_kernel<NB,W,kVT,kSP>   K1: one residual + Jacobian sweep, rows written to HBM (parity + roofline runs;
//                            smpc_eval_kernel.hpp);
//                            kVT: per-scene horizons; kSP (with kVT): per-scene weights and velocity bounds as well
//                            (smpc_scene_batch.scene_params);
//   smpc_stage_kernel<W>     the staging pass of the people block (smpc_stage_kernel.hpp);
//   the probe kernels (smpc_probes.hpp);
//   and the kernels of the tick around the solve, one header each (projection, distance, format, trajectorize, window,
//   metrics, crowd, local costmap, global plan, visibility, nearest agents, pool crowd, sensed costmap, obstacle memory,
//   people tracks, people detections, robot plant, collision monitor, people detections from the scan, plan repair).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "smpc_host.hpp"
#include "smpc_sweep_host.hpp"
#include "smpc_probes.hpp"
#include "smpc_project.hpp"
#include "smpc_distance.hpp"
#include "smpc_format.hpp"
#include "smpc_trajectorize.hpp"
#include "smpc_path_window.hpp"
#include "smpc_metrics.hpp"
#include "smpc_crowd.hpp"
#include "smpc_local_costmap.hpp"
#include "../../include/smpc_local_costmap.h"
#include "smpc_global_plan.hpp"
#include "smpc_visibility.hpp"
#include "../../include/smpc_visibility.h"
#include "smpc_nearest.hpp"
#include "../../include/smpc_nearest.h"
#include "smpc_crowd_pool.hpp"
#include "../../include/smpc_crowd_pool.h"
#include "smpc_sensed_costmap.hpp"
#include "../../include/smpc_sensed_costmap.h"
#include "smpc_obstacle_memory.hpp"
#include "../../include/smpc_obstacle_memory.h"
#include "smpc_tracker.hpp"
#include "../../include/smpc_tracker.h"
#include "smpc_detector.hpp"
#include "../../include/smpc_detector.h"
#include "smpc_plant.hpp"
#include "../../include/smpc_plant.h"
#include "smpc_collision_monitor.hpp"
#include "../../include/smpc_collision_monitor.h"
#include "smpc_scan_people.hpp"
#include "../../include/smpc_scan_people.h"
#include "smpc_plan_repair.hpp"
#include "smpc_plan_smoother.hpp"

extern "C" {

int smpc_abi_version(void) { return SMPC_ABI_VERSION; }

const char* smpc_last_error(void) { return g_last_error.c_str(); }

void smpc_params_default(smpc_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  // code defaults of OptimizerParams::get, reference src/optimizer.cpp:26-82
  p->distance_w = 3.0; p->socialwork_w = 1.0; p->velocity_w = 0.5; p->angle_w = 0.0; p->agent_angle_w = 0.5;
  p->proxemics_w = 90.0; p->velocity_feasibility_w = 0.5; p->obstacle_w = 0.0; p->goal_align_w = 0.0;
  p->control_horizon = 5; p->parameter_block_length = 5; p->max_iterations = 100;
  p->linear_solver_type = SMPC_SPARSE_NORMAL_CHOLESKY;
  p->fn_tol = 1e-7; p->gradient_tol = 1e-10; p->param_tol = 1e-15;
  // literals of Optimizer::optimize, src/optimizer.cpp:238,375-378
  p->desired_linear_vel = 0.6; p->v_min = 0.0; p->v_max = 0.6; p->w_min = -1.4; p->w_max = 1.4;
  p->fixed_iterations = 0; p->tol_needs_successful_step = 0;
}

int smpc_dims(const smpc_params* p, int T, int has_people, int* CH, int* bl, int* nb, int* P, int* M, int* n_bounded_blocks) {
  if (!p || T < 1 || p->control_horizon < 1 || p->parameter_block_length < 1) { set_error("bad arguments to smpc_dims"); return SMPC_ERR_INVALID_ARG; }
  const Dims d = make_dims(*p, T, has_people != 0);
  if (CH) *CH = d.CH;
  if (bl) *bl = d.bl;
  if (nb) *nb = d.nb;
  if (P) *P = d.P;
  if (M) *M = d.M;
  if (n_bounded_blocks) *n_bounded_blocks = d.nbounded;
  return SMPC_OK;
}

smpc_handle* smpc_create(const smpc_params* p, int device) {
  if (!p) { set_error("null params"); return nullptr; }
  if (p->linear_solver_type < SMPC_DENSE_SCHUR || p->linear_solver_type > SMPC_SPARSE_NORMAL_CHOLESKY) {
    set_error("Invalid parameter: linear_solver_type");  // same message as reference src/optimizer.cpp:44
    return nullptr;
  }
  if (p->max_iterations < 0 || p->max_iterations > SMPC_MAX_LM_ITERATIONS) {
    set_error("Invalid parameter: max_iterations (0 .. SMPC_MAX_LM_ITERATIONS)");
    return nullptr;
  }
  int count = 0;
  hipError_t e = hipGetDeviceCount(&count);
  if (e != hipSuccess || count <= 0) { set_error("no HIP device available (this library has no CPU fallback)"); return nullptr; }
  if (device < 0 || device >= count) { set_error("device index out of range"); return nullptr; }
  if (hipSetDevice(device) != hipSuccess) { set_error("hipSetDevice failed"); return nullptr; }
  smpc_handle* h = new smpc_handle();
  h->prm = *p;
  h->device = device;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) != hipSuccess) { set_error("hipGetDeviceProperties failed"); delete h; return nullptr; }
  h->num_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  if (hipEventCreate(&h->ev0) != hipSuccess || hipEventCreate(&h->ev1) != hipSuccess) { set_error("hipEventCreate failed"); delete h; return nullptr; }
  if (hipMalloc(reinterpret_cast<void**>(&h->queue), smpc::kQueueWords * sizeof(int)) != hipSuccess) { set_error("hipMalloc(queue) failed"); delete h; return nullptr; }
  return h;
}

void smpc_destroy(smpc_handle* h) {
  if (!h) return;
  (void)hipEventDestroy(h->ev0);
  (void)hipEventDestroy(h->ev1);
  if (h->queue) (void)hipFree(h->queue);
  if (h->stage_rec) (void)hipFree(h->stage_rec);
  if (h->stage_aux) (void)hipFree(h->stage_aux);
  if (h->neutral_sp) (void)hipFree(h->neutral_sp);
  if (h->gp_fail) (void)hipFree(h->gp_fail);
  if (h->stage) (void)hipFree(h->stage);
  if (h->pin) (void)hipHostFree(h->pin);
  delete h;
}

int smpc_set_stream(smpc_handle* h, void* hip_stream) {
  if (!h) { set_error("null handle"); return SMPC_ERR_INVALID_ARG; }
  h->stream = static_cast<hipStream_t>(hip_stream);
  return SMPC_OK;
}

double smpc_last_kernel_ms(smpc_handle* h) {
  if (!h || !h->timed) return -1.0;
  if (hipEventSynchronize(h->ev1) != hipSuccess) return -1.0;
  float ms = 0.f;
  if (hipEventElapsedTime(&ms, h->ev0, h->ev1) != hipSuccess) return -1.0;
  return (double)ms;
}

int smpc_set_solve_share(smpc_handle* h, int32_t n) {
  if (!h || n < 1) { set_error("null handle or share < 1"); return SMPC_ERR_INVALID_ARG; }
  h->share = n;
  return SMPC_OK;
}

// the arguments of the two queries about a solve launch
static int check_solve_shape(const smpc_handle* h, int32_t B, int32_t T, int32_t N) {
  if (!h || B < 0 || T < 1 || N < 0) { set_error("null handle or bad B/T/N"); return SMPC_ERR_INVALID_ARG; }
  if (T + 1 > smpc::kWave || N > smpc::kWave) { set_error("T + 1 > 64 rollout poses or N > 64 agents"); return SMPC_ERR_UNSUPPORTED; }
  return SMPC_OK;
}

int smpc_solve_slot_width(const smpc_handle* h, int32_t B, int32_t T, int32_t N) {
  SMPC_TRY(check_solve_shape(h, B, T, N));
  return plan_for(h, Sweep::Solve, B, T, N, make_dims(h->prm, T, true), false, false, smpc::read_knobs()).W;
}

int smpc_set_fixed_shapes(smpc_handle* h, int32_t enable) {
  if (!h) { set_error("null handle"); return SMPC_ERR_INVALID_ARG; }
  h->fixed_shapes = enable != 0;
  return SMPC_OK;
}

int smpc_solve_shape_is_fixed(const smpc_handle* h, int32_t B, int32_t T, int32_t N) {
  SMPC_TRY(check_solve_shape(h, B, T, N));
  if (h->prm.control_horizon < 1 || h->prm.parameter_block_length < 1) { set_error("control_horizon and parameter_block_length must be >= 1"); return SMPC_ERR_INVALID_ARG; }
  return plan_for(h, Sweep::Solve, B, T, N, make_dims(h->prm, T, true), false, false, smpc::read_knobs()).fixed >= 0 ? 1 : 0;
}

int smpc_eval_shape_is_fixed(const smpc_handle* h, int32_t T, int32_t N) {
  if (!h || T < 1 || N < 0) { set_error("null handle or bad T/N"); return SMPC_ERR_INVALID_ARG; }
  if (T + 1 > smpc::kWave || N > smpc::kWave) { set_error("T + 1 > 64 rollout poses or N > 64 agents"); return SMPC_ERR_UNSUPPORTED; }
  if (h->prm.control_horizon < 1 || h->prm.parameter_block_length < 1) { set_error("control_horizon and parameter_block_length must be >= 1"); return SMPC_ERR_INVALID_ARG; }
  return plan_for(h, Sweep::Eval, 0, T, N, make_dims(h->prm, T, true), false, false, smpc::read_knobs()).fixed >= 0 ? 1 : 0;
}

}  // extern "C"

namespace {

// smpc_solve_batch (trace == nullptr) and smpc_solve_trace_batch
int solve_batch(smpc_handle* h, const smpc_scene_batch* sb, smpc_result_batch* out, const smpc_trace_out* trace) {
  const Sweep kind = trace ? Sweep::Trace : Sweep::Solve;
  return sweep_call(h, sb, kind, out ? nullptr : "null result batch", [&](const Dims& d, smpc::KParams& k, Staging& st) -> int {
    const size_t B = sb->B, T = sb->T;
    if (sb->order && !sb->on_device) {  // queue order hint
      std::vector<uint8_t> seen(B, 0);
      for (size_t i = 0; i < B; ++i) {
        const int32_t v = sb->order[i];
        if (v < 0 || (size_t)v >= B || seen[v]) { set_error("order is not a permutation of 0..B-1"); return SMPC_ERR_INVALID_ARG; }
        seen[v] = 1;
      }
    }
    SMPC_TRY(st.in(k.order, sb->order, B));
    SMPC_TRY(st.out(k.o_params, out->params, B * d.P));
    SMPC_TRY(st.out(k.o_cmds, out->cmds, B * (T + 1) * 2));
    SMPC_TRY(st.out(k.o_path, out->path, B * (T + 1) * 3));
    SMPC_TRY(st.out(k.o_status, out->status, B));
    SMPC_TRY(st.out(k.o_reason, out->reason, B));
    SMPC_TRY(st.out(k.o_iterations, out->iterations, B));
    SMPC_TRY(st.out(k.o_evaluations, out->evaluations, B));
    SMPC_TRY(st.out(k.o_initial_cost, out->initial_cost, B));
    SMPC_TRY(st.out(k.o_final_cost, out->final_cost, B));
    // a device-side order cannot be checked here: should it not be a permutation, the scenes it leaves out must not keep
    // the status of an earlier call — every status starts as SMPC_NOT_SOLVED (-1) and is overwritten by the scene's solve
    if (sb->on_device && k.order && k.o_status && B > 0) SMPC_HIP_CHECK(hipMemsetAsync(k.o_status, 0xFF, B * sizeof(int32_t), h->stream));
    if (trace) {
      k.trace_rows = trace->max_rows;
      // read and written: the rows a solve does not produce keep the caller's bytes on the way through device memory too
      SMPC_TRY(st.inout(k.o_trace, trace->rows, B * (size_t)trace->max_rows * SMPC_TRACE_COLS));
      SMPC_TRY(st.out(k.o_trace_n, trace->n_rows, B));
      if (!k.scene_params && B > 0) SMPC_TRY(neutral_rows(h, k));
    }
    return SMPC_OK;
  });
}

}  // namespace

extern "C" {

int smpc_solve_batch(smpc_handle* h, const smpc_scene_batch* sb, smpc_result_batch* out) { return solve_batch(h, sb, out, nullptr); }

int smpc_solve_trace_batch(smpc_handle* h, const smpc_scene_batch* sb, smpc_result_batch* out, const smpc_trace_out* trace) {
  if (!trace || trace->max_rows < 0 || (trace->max_rows > 0 && !trace->rows)) {
    set_error("null trace, max_rows < 0 or null rows with max_rows > 0"); return SMPC_ERR_INVALID_ARG;
  }
  return solve_batch(h, sb, out, trace);
}

int smpc_project_people_batch(smpc_handle* h, const smpc_projection_batch* in, double* people_proj, int32_t* error) {
  if (!h || !in || !people_proj) { set_error("null handle / input / output"); return SMPC_ERR_INVALID_ARG; }
  if (in->B < 0 || in->T < 1 || in->N < 1) { set_error("bad B/T/N"); return SMPC_ERR_INVALID_ARG; }
  if (in->N + 1 > smpc::kWave) { set_error("N + 1 > 64 agents is not supported"); return SMPC_ERR_UNSUPPORTED; }
  if (!in->init_people || !in->robot_path || !in->od_origin) { set_error("null input array"); return SMPC_ERR_INVALID_ARG; }
  // the reference throws for an empty / malformed ObstacleDistance grid (src/optimizer.cpp:676-687)
  if (!in->od_indexes) { set_error("ObstacleDistance grid is empty"); return SMPC_ERR_INVALID_ARG; }
  if (in->od_width <= 0 || in->od_height <= 0) { set_error("ObstacleDistance grid has invalid size"); return SMPC_ERR_INVALID_ARG; }
  if (!(in->od_resolution > 0.0f)) { set_error("ObstacleDistance grid has invalid resolution"); return SMPC_ERR_INVALID_ARG; }
  SMPC_HIP_CHECK(hipSetDevice(h->device));
  smpc::ProjParams p;
  std::memset(&p, 0, sizeof(p));
  p.B = in->B; p.T = in->T; p.N = in->N;
  int G = 2;
  while (G < in->N + 1) G *= 2;
  p.G = G;
  p.H = (2 * G <= smpc::kWave) ? 2 : 1;  // two copies of a scene split the partner rounds while they fit in the wavefront
  smpc::fill_math_table(&p.mt);
  p.max_time = in->max_time; p.time_step = in->time_step; p.od_resolution = in->od_resolution;
  p.od_shared = in->od_shared; p.od_width = in->od_width; p.od_height = in->od_height;
  const size_t B = in->B, T = in->T, N = in->N;
  const size_t ngrid = in->od_shared ? 1 : B;
  Staging st(h, in->on_device);
  SMPC_TRY(st.in(p.init_people, in->init_people, B * N * 6));
  SMPC_TRY(st.in(p.robot_path, in->robot_path, B * (T + 1) * 6));
  SMPC_TRY(st.in(p.od_indexes, in->od_indexes, ngrid * (size_t)in->od_width * in->od_height));
  SMPC_TRY(st.in(p.od_origin, in->od_origin, ngrid * 2));
  SMPC_TRY(st.out(p.people_proj, people_proj, B * (T + 1) * 6 * N));
  SMPC_TRY(st.out(p.error, error, B));
  if (B > 0) {
    const int per_wave = smpc::kWave / (G * p.H);
    const int grid = (int)((B + per_wave - 1) / per_wave);
    SMPC_TRY(st.timed([&] { hipLaunchKernelGGL(smpc::smpc_project_kernel, dim3(grid), dim3(smpc::kWave), 0, h->stream, p); return SMPC_OK; }));
  }
  return st.finish();
}

int smpc_obstacle_distance_batch(smpc_handle* h, const smpc_obstacle_distance_in* in, smpc_obstacle_distance_out* out) {
  if (!h || !in || !out || !out->indexes) { set_error("null handle / input / output"); return SMPC_ERR_INVALID_ARG; }
  if (in->B < 0) { set_error("bad B"); return SMPC_ERR_INVALID_ARG; }
  if (!in->costmap || in->size_x < 1 || in->size_y < 1) { set_error("costmap grid is empty"); return SMPC_ERR_INVALID_ARG; }
  if (in->obstacle_min_cost < 1) { set_error("obstacle_min_cost must be 1..255"); return SMPC_ERR_INVALID_ARG; }
  if (!(in->resolution > 0.0)) { set_error("costmap resolution must be > 0"); return SMPC_ERR_INVALID_ARG; }
  if (in->size_x > smpc::kOdMaxW || in->size_y > smpc::kOdMaxH) {
    set_error("costmap larger than 4096 x 32768 cells is not supported"); return SMPC_ERR_UNSUPPORTED;
  }
  SMPC_HIP_CHECK(hipSetDevice(h->device));
  smpc::DistParams p;
  std::memset(&p, 0, sizeof(p));
  p.W = in->size_x; p.H = in->size_y;
  p.min_cost = in->obstacle_min_cost; p.unknown_is_obstacle = in->unknown_is_obstacle ? 1 : 0;
  p.resolution = (float)in->resolution;
  const size_t ngrid = in->costmap_shared ? 1 : (size_t)in->B, cells = ngrid * (size_t)in->size_x * in->size_y;
  Staging st(h, in->on_device);
  SMPC_TRY(st.in(p.costmap, in->costmap, cells));
  SMPC_TRY(st.out(p.indexes, out->indexes, cells));
  SMPC_TRY(st.out(p.distances, out->distances, cells));
  SMPC_TRY(st.out(p.n_obstacles, out->n_obstacles, ngrid));
  if (ngrid > 0) {
    SMPC_TRY(st.timed([&] {
      hipLaunchKernelGGL(smpc::smpc_obstacle_distance_kernel, dim3((unsigned)ngrid), dim3(smpc::kOdThreads), 0, h->stream, p);
      return SMPC_OK;
    }));
  }
  return st.finish();
}

int smpc_people_to_status_batch(smpc_handle* h, const smpc_people_batch* in, double* init_people, uint8_t* has_people) {
  if (!h || !in || !init_people) { set_error("null handle / input / output"); return SMPC_ERR_INVALID_ARG; }
  if (in->B < 0 || in->Np < 1 || in->N < 1) { set_error("bad B / Np / N"); return SMPC_ERR_INVALID_ARG; }
  if (!in->people || !in->count) { set_error("null input array"); return SMPC_ERR_INVALID_ARG; }
  SMPC_HIP_CHECK(hipSetDevice(h->device));
  const size_t B = in->B, Np = in->Np, N = in->N;
  smpc::PeopleParams p;
  std::memset(&p, 0, sizeof(p));
  p.B = in->B; p.Np = in->Np; p.N = in->N;
  const bool filter = in->robot_pose != nullptr;
  if (filter && (!in->costmap_origin || in->size_x < 1 || in->size_y < 1 || !(in->resolution > 0.0))) {
    set_error("field-of-view filter needs the costmap geometry"); return SMPC_ERR_INVALID_ARG;
  }
  p.fov_angle = in->fov_angle; p.costmap_shared = in->costmap_shared; p.size_x = in->size_x; p.size_y = in->size_y;
  p.resolution = in->resolution;
  Staging st(h, in->on_device);
  SMPC_TRY(st.in(p.people, in->people, B * Np * 5));
  SMPC_TRY(st.in(p.count, in->count, B));
  SMPC_TRY(st.in(p.robot_pose, in->robot_pose, B * 3));
  // read by the field-of-view filter alone
  SMPC_TRY(st.in(p.costmap_origin, filter ? in->costmap_origin : nullptr, (in->costmap_shared ? 1 : B) * 2));
  SMPC_TRY(st.out(p.init_people, init_people, B * N * 6));
  SMPC_TRY(st.out(p.has_people, has_people, B));
  if (B > 0) {
    SMPC_TRY(st.timed([&] {
      hipLaunchKernelGGL(smpc::smpc_people_to_status_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, h->stream, p);
      return SMPC_OK;
    }));
  }
  return st.finish();
}

int smpc_format_to_optimize_batch(smpc_handle* h, const smpc_format_batch* in, smpc_format_out* out) {
  if (!h || !in || !out) { set_error("null handle / input / output"); return SMPC_ERR_INVALID_ARG; }
  if (in->B < 0 || in->T < 1) { set_error("bad B/T"); return SMPC_ERR_INVALID_ARG; }
  if (!in->path || !in->cmds || !in->speed || !in->memory.prev_path || !in->memory.prev_cmds || !in->memory.valid) {
    set_error("null input array / memory record"); return SMPC_ERR_INVALID_ARG;
  }
  if (!out->robot_status || !out->pose0 || !out->init_params || !out->path_pts || !out->goal_yaw) {
    set_error("null output array"); return SMPC_ERR_INVALID_ARG;
  }
  SMPC_HIP_CHECK(hipSetDevice(h->device));
  const Dims d = make_dims(h->prm, in->T, true);
  const size_t B = in->B, Tp = (size_t)in->T + 1;
  smpc::FormatParams p;
  std::memset(&p, 0, sizeof(p));
  const size_t rows = in->path_rows > 0 ? (size_t)in->path_rows : Tp;
  if (rows < Tp) { set_error("path_rows < T + 1"); return SMPC_ERR_INVALID_ARG; }
  p.B = in->B; p.T = in->T; p.nb = d.nb; p.P = d.P; p.rows = (int)rows;
  p.max_poses = in->max_poses > 0 ? in->max_poses : 0;
  p.time_step = in->time_step; p.current_path_w = in->current_path_w; p.current_cmds_w = in->current_cmds_w;
  if (in->n_poses && !in->memory.length) {
    set_error("n_poses needs memory.length: records of scenes with horizons of their own differ in size"); return SMPC_ERR_INVALID_ARG;
  }
  Staging st(h, in->on_device);
  SMPC_TRY(st.in(p.n_poses, in->n_poses, B));
  SMPC_TRY(st.inout(p.length, in->memory.length, B * 2));
  SMPC_TRY(st.out(p.T_scene, out->T_scene, B));
  SMPC_TRY(st.in(p.path, in->path, B * rows * 3));
  SMPC_TRY(st.in(p.cmds, in->cmds, B * rows * 2));
  SMPC_TRY(st.in(p.speed, in->speed, B * 2));
  SMPC_TRY(st.inout(p.prev_path, in->memory.prev_path, B * Tp * 3));
  SMPC_TRY(st.inout(p.prev_cmds, in->memory.prev_cmds, B * Tp * 2));
  SMPC_TRY(st.inout(p.valid, in->memory.valid, B));
  SMPC_TRY(st.out(p.robot_status, out->robot_status, B * Tp * 6));
  SMPC_TRY(st.out(p.pose0, out->pose0, B * 3));
  SMPC_TRY(st.out(p.init_params, out->init_params, B * (size_t)d.P));
  SMPC_TRY(st.out(p.path_pts, out->path_pts, B * Tp * 2));
  SMPC_TRY(st.out(p.goal_yaw, out->goal_yaw, B));
  if (B > 0) {
    const long long n = (long long)B * (long long)Tp;
    SMPC_TRY(st.timed([&] {
      hipLaunchKernelGGL(smpc::smpc_format_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, p);
      SMPC_HIP_CHECK(hipGetLastError());
      hipLaunchKernelGGL(smpc::smpc_format_mark_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, h->stream, p);
      return SMPC_OK;
    }));
  }
  return st.finish();
}

int smpc_memory_store_batch(smpc_handle* h, int32_t B_, int32_t T, int32_t on_device, const int32_t* status,
                            const double* path, const double* cmds, smpc_memory_batch* memory, const int32_t* T_scene) {
  if (!h || !status || !path || !cmds || !memory || !memory->prev_path || !memory->prev_cmds || !memory->valid) {
    set_error("null handle / array / memory record"); return SMPC_ERR_INVALID_ARG;
  }
  if (B_ < 0 || T < 1) { set_error("bad B/T"); return SMPC_ERR_INVALID_ARG; }
  if (T_scene && !memory->length) {
    set_error("T_scene needs memory.length: records of scenes with horizons of their own differ in size"); return SMPC_ERR_INVALID_ARG;
  }
  SMPC_HIP_CHECK(hipSetDevice(h->device));
  const size_t B = B_, Tp = (size_t)T + 1;
  smpc::StoreParams p;
  std::memset(&p, 0, sizeof(p));
  p.B = B_; p.T = T;
  Staging st(h, on_device);
  SMPC_TRY(st.in(p.T_scene, T_scene, B));
  SMPC_TRY(st.inout(p.length, memory->length, B * 2));
  SMPC_TRY(st.in(p.status, status, B));
  SMPC_TRY(st.in(p.path, path, B * Tp * 3));
  SMPC_TRY(st.in(p.cmds, cmds, B * Tp * 2));
  SMPC_TRY(st.inout(p.prev_path, memory->prev_path, B * Tp * 3));
  SMPC_TRY(st.inout(p.prev_cmds, memory->prev_cmds, B * Tp * 2));
  SMPC_TRY(st.inout(p.valid, memory->valid, B));
  if (B > 0) {
    const long long n = (long long)B * (long long)Tp;
    SMPC_TRY(st.timed([&] {
      hipLaunchKernelGGL(smpc::smpc_memory_store_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, p);
      return SMPC_OK;
    }));
  }
  return st.finish();
}

int smpc_trajectorize_path_batch(smpc_handle* h, const smpc_trajectorize_batch* in, smpc_trajectorize_out* out) {
  if (!h || !in || !out) { set_error("null handle / input / output"); return SMPC_ERR_INVALID_ARG; }
  if (in->B < 0 || in->L < 1 || in->max_steps < 0) { set_error("bad B / L / max_steps"); return SMPC_ERR_INVALID_ARG; }
  if (!in->plan || !in->plan_len || !in->robot_pose) { set_error("null input array"); return SMPC_ERR_INVALID_ARG; }
  if (!out->path || !out->cmds || !out->n_poses) { set_error("null output array"); return SMPC_ERR_INVALID_ARG; }
  SMPC_HIP_CHECK(hipSetDevice(h->device));
  const size_t B = in->B, L = in->L, S1 = (size_t)in->max_steps + 1;
  smpc::TrajParams p;
  std::memset(&p, 0, sizeof(p));
  p.B = in->B; p.L = in->L; p.max_steps = in->max_steps; p.omnidirectional = in->omnidirectional;
  p.desired_linear_vel = in->desired_linear_vel; p.lookahead_dist = in->lookahead_dist;
  p.max_angular_vel = in->max_angular_vel; p.time_step = in->time_step;
  smpc::fill_math_table(&p.mt);
  Staging st(h, in->on_device);
  SMPC_TRY(st.in(p.plan, in->plan, B * L * 2));
  SMPC_TRY(st.in(p.plan_len, in->plan_len, B));
  SMPC_TRY(st.in(p.robot_pose, in->robot_pose, B * 3));
  SMPC_TRY(st.out(p.path, out->path, B * S1 * 3));
  SMPC_TRY(st.out(p.cmds, out->cmds, B * S1 * 2));
  SMPC_TRY(st.out(p.cmds_vy, out->cmds_vy, B * S1));
  SMPC_TRY(st.out(p.n_poses, out->n_poses, B));
  SMPC_TRY(st.out(p.error, out->error, B));
  if (B > 0) {
    const int per_wave = smpc::kWave / smpc::kTrajGroup;
    // plans of up to 512 poses stay in registers (kR poses per lane of a 16-lane group); the raw step outputs are parked
    // in LDS (48 bytes per step and plan): four-wavefront blocks while their park fits in 48 KB (64 steps), else
    // one-wavefront blocks (up to 256 steps). Longer plans / horizons take the kernel that searches the plan in memory.
    const size_t park_step = (size_t)smpc::kTrajParkDoubles * sizeof(double);
    const size_t park_wave = (size_t)per_wave * in->max_steps * park_step;
    const int threads = (park_wave * (smpc::kTrajBlock / smpc::kWave) <= 48 * 1024) ? smpc::kTrajBlock : smpc::kWave;
    const int per_block = threads / smpc::kTrajGroup;
    const size_t park = park_wave * (threads / smpc::kWave);
    const dim3 grid((unsigned)((B + per_block - 1) / per_block)), block(threads);
    const int need = (int)((L + smpc::kTrajGroup - 1) / smpc::kTrajGroup);
    // plans over 512 poses: one-wavefront blocks of the 8-slot kernel with the reachable poses compacted into LDS
    const size_t list_wave = (size_t)per_wave * 8 * smpc::kTrajGroup * 2 * sizeof(double);
    SMPC_TRY(st.timed([&] {
      if (need > 32 && park_wave + list_wave <= 48 * 1024) {
        p.compact = 1;
        hipLaunchKernelGGL(smpc::smpc_trajectorize_kernel<8>, dim3((unsigned)((B + per_wave - 1) / per_wave)), dim3(smpc::kWave),
                           park_wave + list_wave, h->stream, p);
      } else if (need > 32 || park > 48 * 1024) {
        hipLaunchKernelGGL(smpc::smpc_trajectorize_long_kernel, dim3((unsigned)((B + per_wave - 1) / per_wave)), dim3(smpc::kWave), 0, h->stream, p);
      } else if (need <= 8) {
        hipLaunchKernelGGL(smpc::smpc_trajectorize_kernel<8>, grid, block, park, h->stream, p);
      } else if (need <= 16) {
        hipLaunchKernelGGL(smpc::smpc_trajectorize_kernel<16>, grid, block, park, h->stream, p);
      } else if (need <= 25) {
        hipLaunchKernelGGL(smpc::smpc_trajectorize_kernel<25>, grid, block, park, h->stream, p);
      } else {
        hipLaunchKernelGGL(smpc::smpc_trajectorize_kernel<32>, grid, block, park, h->stream, p);
      }
      return SMPC_OK;
    }));
  }
  return st.finish();
}

int smpc_transform_global_plan_batch(smpc_handle* h, const smpc_plan_window_batch* in, double* window, int32_t* window_len,
                                     int32_t* error) {
  if (!h || !in || !window || !window_len) { set_error("null handle / input / output"); return SMPC_ERR_INVALID_ARG; }
  if (in->B < 0 || in->L < 1) { set_error("bad B / L"); return SMPC_ERR_INVALID_ARG; }
  if (!in->plan || !in->plan_len || !in->plan_start || !in->robot_pose) { set_error("null input array"); return SMPC_ERR_INVALID_ARG; }
  SMPC_HIP_CHECK(hipSetDevice(h->device));
  const size_t B = in->B, L = in->L;
  smpc::WindowParams p;
  std::memset(&p, 0, sizeof(p));
  p.B = in->B; p.L = in->L; p.search_dist = in->max_robot_pose_search_dist; p.dist_threshold = in->dist_threshold;
  Staging st(h, in->on_device);
  SMPC_TRY(st.in(p.plan, in->plan, B * L * 2));
  SMPC_TRY(st.in(p.plan_len, in->plan_len, B));
  SMPC_TRY(st.inout(p.plan_start, in->plan_start, B));
  SMPC_TRY(st.in(p.robot_pose, in->robot_pose, B * 3));
  SMPC_TRY(st.in(p.to_local, in->to_local, B * 3));
  SMPC_TRY(st.out(p.window, window, B * L * 2));
  SMPC_TRY(st.out(p.window_len, window_len, B));
  SMPC_TRY(st.out(p.error, error, B));
  if (B > 0) {
    SMPC_TRY(st.timed([&] {
      hipLaunchKernelGGL(smpc::smpc_plan_window_kernel, dim3((unsigned)B), dim3(smpc::kWave), 0, h->stream, p);
      return SMPC_OK;
    }));
  }
  return st.finish();
}

int smpc_select_command_batch(smpc_handle* h, int32_t B_, int32_t T, int32_t traj_rows, int32_t on_device, const int32_t* traj_n_poses,
                              const double* traj_cmds, const int32_t* status, const double* cmds, double* cmd_vel, int32_t* source,
                              const int32_t* window_error) {
  if (!h || !traj_cmds || !status || !cmds || !cmd_vel) { set_error("null handle / array"); return SMPC_ERR_INVALID_ARG; }
  if (B_ < 0 || T < 1 || traj_rows < 1) { set_error("bad B / T / traj_rows"); return SMPC_ERR_INVALID_ARG; }
  SMPC_HIP_CHECK(hipSetDevice(h->device));
  const size_t B = B_;
  smpc::SelectParams p;
  std::memset(&p, 0, sizeof(p));
  p.B = B_; p.T = T; p.rows = traj_rows;
  Staging st(h, on_device);
  SMPC_TRY(st.in(p.window_error, window_error, B));
  SMPC_TRY(st.in(p.traj_n, traj_n_poses, B));
  SMPC_TRY(st.in(p.traj_cmds, traj_cmds, B * (size_t)traj_rows * 2));
  SMPC_TRY(st.in(p.status, status, B));
  SMPC_TRY(st.in(p.cmds, cmds, B * ((size_t)T + 1) * 2));
  SMPC_TRY(st.out(p.cmd_vel, cmd_vel, B * 2));
  SMPC_TRY(st.out(p.source, source, B));
  if (B > 0) {
    SMPC_TRY(st.timed([&] {
      hipLaunchKernelGGL(smpc::smpc_select_command_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, h->stream, p);
      return SMPC_OK;
    }));
  }
  return st.finish();
}

int smpc_episode_metrics_batch(smpc_handle* h, const smpc_metrics_batch* in, double* acc) {
  if (!h || !in || !acc) { set_error("null handle / input / acc"); return SMPC_ERR_INVALID_ARG; }
  if (in->B < 1 || in->Np < 1 || !(in->dt > 0.0)) { set_error("bad B / Np / dt"); return SMPC_ERR_INVALID_ARG; }
  if (!(in->goal_tolerance >= 0.0) || !(in->robot_radius >= 0.0) || !(in->person_radius >= 0.0) || !(in->intimate_radius >= 0.0) ||
      !(in->personal_radius >= 0.0) || !(in->social_radius >= 0.0)) {
    set_error("negative radius or tolerance"); return SMPC_ERR_INVALID_ARG;
  }
  if (!in->robot_pose || !in->robot_twist || !in->people || !in->count) { set_error("null input array"); return SMPC_ERR_INVALID_ARG; }
  if (in->od_distances && (!in->od_origin || in->od_width < 1 || in->od_height < 1 || !(in->od_resolution > 0.0f))) {
    set_error("distance grid without origin or with a non-positive size or resolution"); return SMPC_ERR_INVALID_ARG;
  }
  if (in->Np > SMPC_MAX_AGENTS) { set_error("Np > 64 persons is not supported"); return SMPC_ERR_UNSUPPORTED; }
  if (!in->on_device)
    for (int32_t b = 0; b < in->B; ++b)
      if (in->count[b] < 0 || in->count[b] > in->Np) { set_error("count outside 0..Np"); return SMPC_ERR_INVALID_ARG; }
  SMPC_HIP_CHECK(hipSetDevice(h->device));
  smpc::MetricsParams p;
  std::memset(&p, 0, sizeof(p));
  p.B = in->B; p.Np = in->Np;
  int G = 1;
  while (G < in->Np) G *= 2;
  p.G = G;
  p.dt = in->dt; p.goal_tolerance = in->goal_tolerance; p.robot_radius = in->robot_radius; p.person_radius = in->person_radius;
  p.intimate_radius = in->intimate_radius; p.personal_radius = in->personal_radius; p.social_radius = in->social_radius;
  const bool grid = in->od_distances != nullptr;
  p.od_shared = in->od_shared ? 1 : 0; p.od_width = in->od_width; p.od_height = in->od_height; p.od_resolution = in->od_resolution;
  const size_t B = in->B, Np = in->Np, ngrid = in->od_shared ? 1 : B;
  Staging st(h, in->on_device);
  SMPC_TRY(st.in(p.pose, in->robot_pose, B * 3));
  SMPC_TRY(st.in(p.twist, in->robot_twist, B * 2));
  SMPC_TRY(st.in(p.people, in->people, B * Np * 5));
  SMPC_TRY(st.in(p.count, in->count, B));
  SMPC_TRY(st.in(p.goal, in->goal, B * 2));
  SMPC_TRY(st.in(p.od_distances, in->od_distances, grid ? ngrid * (size_t)in->od_width * in->od_height : 0));
  SMPC_TRY(st.in(p.od_origin, grid ? in->od_origin : nullptr, ngrid * 2));
  SMPC_TRY(st.in(p.status, in->status, B));
  SMPC_TRY(st.in(p.source, in->source, B));
  SMPC_TRY(st.inout(p.acc, acc, B * SMPC_METRIC_COLS));
  const size_t per_block = smpc::kMetricsThreads / G;
  SMPC_TRY(st.timed([&] {
    hipLaunchKernelGGL(smpc::smpc_episode_metrics_kernel, dim3((unsigned)((B + per_block - 1) / per_block)), dim3(smpc::kMetricsThreads), 0,
                       h->stream, p);
    return SMPC_OK;
  }));
  return st.finish();
}

// smpc_crowd_step_batch (groups == nullptr) and smpc_crowd_step_groups_batch with a group_id array: one validation, one
// staging path, the kernel by the presence of groups
static int crowd_step(smpc_handle* h, const smpc_crowd_batch* in, const smpc_crowd_groups* groups, double* people, int32_t* cursor) {
  if (!h || !in || !people || !cursor) { set_error("null handle / input / people / cursor"); return SMPC_ERR_INVALID_ARG; }
  if (in->B < 1 || in->Np < 1 || in->K < 1 || !(in->dt > 0.0)) { set_error("bad B / Np / K / dt"); return SMPC_ERR_INVALID_ARG; }
  if (!(in->goal_radius >= 0.0) || !(in->person_radius >= 0.0) || !(in->desired_speed > 0.0)) {
    set_error("negative radius or non-positive desired_speed"); return SMPC_ERR_INVALID_ARG;
  }
  if (!in->robot_pose || !in->robot_twist || !in->count || !in->waypoints || !in->n_waypoints) { set_error("null input array"); return SMPC_ERR_INVALID_ARG; }
  if (in->od_indexes && (!in->od_origin || in->od_width < 1 || in->od_height < 1 || !(in->od_resolution > 0.0f))) {
    set_error("obstacle grid without origin or with a non-positive size or resolution"); return SMPC_ERR_INVALID_ARG;
  }
  if (in->Np > SMPC_MAX_AGENTS) { set_error("Np > 64 persons is not supported"); return SMPC_ERR_UNSUPPORTED; }
  if (in->K > SMPC_MAX_WAYPOINTS) { set_error("K > 8 waypoints is not supported"); return SMPC_ERR_UNSUPPORTED; }
  if (!in->on_device)
    for (int32_t b = 0; b < in->B; ++b)
      if (in->count[b] < 0 || in->count[b] > in->Np) { set_error("count outside 0..Np"); return SMPC_ERR_INVALID_ARG; }
  SMPC_HIP_CHECK(hipSetDevice(h->device));
  smpc::CrowdGroupsParams gp;
  std::memset(&gp, 0, sizeof(gp));
  smpc::CrowdParams& p = gp.c;
  p.B = in->B; p.Np = in->Np; p.K = in->K;
  while ((1 << p.lgG) < in->Np) ++p.lgG;
  p.cyclic = in->cyclic ? 1 : 0; p.robot_visible = in->robot_visible ? 1 : 0;
  p.dt = in->dt; p.goal_radius = in->goal_radius; p.person_radius = in->person_radius; p.desired_speed = in->desired_speed;
  smpc::fill_math_table(&p.mt);
  const bool grid = in->od_indexes != nullptr;
  p.od_shared = in->od_shared ? 1 : 0; p.od_width = in->od_width; p.od_height = in->od_height; p.od_resolution = in->od_resolution;
  const size_t B = in->B, Np = in->Np, K = in->K, ngrid = in->od_shared ? 1 : B;
  Staging st(h, in->on_device);
  SMPC_TRY(st.in(p.pose, in->robot_pose, B * 3));
  SMPC_TRY(st.in(p.twist, in->robot_twist, B * 2));
  SMPC_TRY(st.in(p.count, in->count, B));
  SMPC_TRY(st.in(p.waypoints, in->waypoints, B * Np * K * 2));
  SMPC_TRY(st.in(p.n_waypoints, in->n_waypoints, B * Np));
  SMPC_TRY(st.in(p.desired_speeds, in->desired_speeds, B * Np));
  SMPC_TRY(st.in(p.od_indexes, in->od_indexes, grid ? ngrid * (size_t)in->od_width * in->od_height : 0));
  SMPC_TRY(st.in(p.od_origin, grid ? in->od_origin : nullptr, ngrid * 2));
  SMPC_TRY(st.inout(p.people, people, B * Np * 5));
  SMPC_TRY(st.inout(p.cursor, cursor, B * Np));
  if (groups) {
    SMPC_TRY(st.in(gp.group_id, groups->group_id, B * Np));
    gp.factor_gaze = groups->factor_gaze; gp.factor_coherence = groups->factor_coherence; gp.factor_repulsion = groups->factor_repulsion;
  }
  const size_t per_block = smpc::kCrowdThreads >> p.lgG;
  const dim3 blocks((unsigned)((B + per_block - 1) / per_block)), threads(smpc::kCrowdThreads);
  SMPC_TRY(st.timed([&] {
    if (groups) hipLaunchKernelGGL((smpc::smpc_crowd_step_kernel<true, smpc::CrowdGroupsParams>), blocks, threads, 0, h->stream, gp);
    else hipLaunchKernelGGL((smpc::smpc_crowd_step_kernel<false, smpc::CrowdParams>), blocks, threads, 0, h->stream, p);
    return SMPC_OK;
  }));
  return st.finish();
}

int smpc_crowd_step_batch(smpc_handle* h, const smpc_crowd_batch* in, double* people, int32_t* cursor) {
  return crowd_step(h, in, nullptr, people, cursor);
}

int smpc_crowd_step_groups_batch(smpc_handle* h, const smpc_crowd_batch* in, const smpc_crowd_groups* groups, double* people,
                                 int32_t* cursor) {
  if (groups) {
    const double f[3] = {groups->factor_gaze, groups->factor_coherence, groups->factor_repulsion};
    for (double v : f)
      if (!(v >= 0.0) || !std::isfinite(v)) { set_error("negative or non-finite group force factor"); return SMPC_ERR_INVALID_ARG; }
  }
  return crowd_step(h, in, groups && groups->group_id ? groups : nullptr, people, cursor);
}

int smpc_local_costmap_batch(smpc_handle* h, const smpc_local_costmap_in* in, int32_t* cell, uint8_t* costmap, double* costmap_origin,
                             int32_t* moved) {
  if (!h || !in || !cell || !costmap || !costmap_origin) { set_error("null handle / input / cell / costmap / costmap_origin"); return SMPC_ERR_INVALID_ARG; }
  if (!in->world || !in->world_origin || !in->pose) { set_error("null input array"); return SMPC_ERR_INVALID_ARG; }
  if (in->B < 0 || in->size_x < 1 || in->size_y < 1 || in->world_x < 1 || in->world_y < 1) {
    set_error("bad B or a non-positive window / world size"); return SMPC_ERR_INVALID_ARG;
  }
  if (!std::isfinite(in->resolution) || !(in->resolution > 0.0)) { set_error("resolution must be finite and > 0"); return SMPC_ERR_INVALID_ARG; }
  const int64_t cells = (int64_t)in->size_x * in->size_y, world_cells = (int64_t)in->world_x * in->world_y;
  if (world_cells >= (int64_t)1 << 31 || cells >= (int64_t)1 << 31 || in->size_x >= 1 << 30 || in->size_y >= 1 << 30) {
    set_error("world or window of 2^31 cells or more, or a window side of 2^30 cells or more, is not supported"); return SMPC_ERR_UNSUPPORTED;
  }
  SMPC_HIP_CHECK(hipSetDevice(h->device));
  smpc::LocalCostmapParams p;
  std::memset(&p, 0, sizeof(p));
  p.B = in->B; p.size_x = in->size_x; p.size_y = in->size_y; p.world_x = in->world_x; p.world_y = in->world_y;
  p.world_shared = in->world_shared ? 1 : 0; p.force = in->force ? 1 : 0; p.outside = 0x01010101u * in->outside_cost;
  p.resolution = in->resolution;
  const size_t B = in->B, nworld = in->world_shared ? 1 : B;
  Staging st(h, in->on_device);
  SMPC_TRY(st.in(p.world, in->world, nworld * (size_t)world_cells));
  SMPC_TRY(st.in(p.world_origin, in->world_origin, nworld * 2));
  SMPC_TRY(st.in(p.pose, in->pose, B * 3));
  SMPC_TRY(st.inout(p.cell, cell, B * 2));
  // read and written: the windows and origins of the robots that stay keep the caller's bytes on the way through device memory too
  SMPC_TRY(st.inout(p.costmap, costmap, B * (size_t)cells));
  SMPC_TRY(st.inout(p.costmap_origin, costmap_origin, B * 2));
  SMPC_TRY(st.out(p.moved, moved, B));
  if (B > 0) {
    // 16-byte stores need every window to start on a 16-byte boundary and every 8-byte half to lie in one window row
    p.wide = (in->size_x % 8 == 0 && cells % 16 == 0 && reinterpret_cast<uintptr_t>(p.costmap) % 16 == 0) ? 1 : 0;
    const size_t grid = B < (size_t)h->num_cu * 8 ? B : (size_t)h->num_cu * 8;  // a fixed grid that strides over the robots
    SMPC_TRY(st.timed([&] {
      hipLaunchKernelGGL(smpc::smpc_local_costmap_kernel, dim3((unsigned)grid), dim3(smpc::kLcThreads), 0, h->stream, p);
      return SMPC_OK;
    }));
  }
  return st.finish();
}

// what smpc_goal_field_batch and smpc_extract_plan_batch check alike: the world, the resolution and the cost parameters
static int check_plan_world(int32_t world_x, int32_t world_y, double resolution, const smpc_plan_cost_params& c, smpc::GpCost* cost) {
  if (world_x < 1 || world_y < 1) { set_error("a non-positive world size"); return SMPC_ERR_INVALID_ARG; }
  if (!std::isfinite(resolution) || !(resolution > 0.0)) { set_error("resolution must be finite and > 0"); return SMPC_ERR_INVALID_ARG; }
  if (c.neutral_cost < 1 || c.cost_weight < 0) { set_error("neutral_cost must be >= 1 and cost_weight >= 0"); return SMPC_ERR_INVALID_ARG; }
  const int64_t w_max = (int64_t)c.neutral_cost + 255 * (int64_t)c.cost_weight;
  if (w_max > 65535) { set_error("neutral_cost + 255 * cost_weight must be <= 65535"); return SMPC_ERR_INVALID_ARG; }
  const int64_t cells = (int64_t)world_x * world_y;
  if (cells >= (int64_t)1 << 31) { set_error("a world of 2^31 cells or more is not supported"); return SMPC_ERR_UNSUPPORTED; }
  if (cells * 7 * w_max >= ((int64_t)1 << 32) - 1) {  // < 2^31 * 2^19
    set_error("world_x * world_y * 7 * (neutral_cost + 255 * cost_weight) must stay below 2^32 - 1: potentials are 32 bits"); return SMPC_ERR_UNSUPPORTED;
  }
  cost->neutral = c.neutral_cost; cost->weight = c.cost_weight;
  cost->lethal_min = c.lethal_min_cost; cost->allow_unknown = c.allow_unknown ? 1u : 0u;
  return SMPC_OK;
}

int smpc_goal_field_batch(smpc_handle* h, const smpc_goal_field_in* in, uint32_t* field, int32_t* status) {
  if (!h || !in || !field) { set_error("null handle / input / field"); return SMPC_ERR_INVALID_ARG; }
  if (!in->world || !in->world_origin || !in->goal) { set_error("null input array"); return SMPC_ERR_INVALID_ARG; }
  if (in->G < 0) { set_error("bad G"); return SMPC_ERR_INVALID_ARG; }
  smpc::GoalFieldParams p;
  std::memset(&p, 0, sizeof(p));
  SMPC_TRY(check_plan_world(in->world_x, in->world_y, in->resolution, in->cost, &p.cost));
  SMPC_HIP_CHECK(hipSetDevice(h->device));
  p.G = in->G; p.world_x = in->world_x; p.world_y = in->world_y; p.world_shared = in->world_shared ? 1 : 0;
  p.resolution = in->resolution;
  p.tiles_x = (in->world_x + smpc::kGfTile - 1) / smpc::kGfTile;
  p.n_tiles = p.tiles_x * ((in->world_y + smpc::kGfTile - 1) / smpc::kGfTile);  // < 2^31 cells: fits
  p.tiles_per_flag = (p.n_tiles + smpc::kGfFlagCap - 1) / smpc::kGfFlagCap;
  p.n_flags = (p.n_tiles + p.tiles_per_flag - 1) / p.tiles_per_flag;
  const size_t G = in->G, cells = (size_t)in->world_x * in->world_y, nworld = in->world_shared ? 1 : G;
  if (G > 0 && !h->gp_fail) SMPC_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&h->gp_fail), sizeof(uint32_t)));  // once per handle
  p.fail = h->gp_fail;
  Staging st(h, in->on_device);
  SMPC_TRY(st.in(p.world, in->world, nworld * cells));
  SMPC_TRY(st.in(p.world_origin, in->world_origin, nworld * 2));
  SMPC_TRY(st.in(p.goal, in->goal, G * 2));
  SMPC_TRY(st.out(p.field, field, G * cells));
  SMPC_TRY(st.out(p.status, status, G));
  uint32_t failed = 0;
  if (G > 0) {
    SMPC_HIP_CHECK(hipMemsetAsync(h->gp_fail, 0, sizeof(uint32_t), h->stream));
    SMPC_TRY(st.timed([&] {
      hipLaunchKernelGGL(smpc::smpc_goal_field_kernel, dim3((unsigned)G), dim3(smpc::kGfThreads), 0, h->stream, p);
      return SMPC_OK;
    }));
    // the one word this call reads back, with device pointers too: did every field settle within its bound?
    SMPC_HIP_CHECK(hipMemcpyAsync(&failed, h->gp_fail, sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    SMPC_HIP_CHECK(hipStreamSynchronize(h->stream));
  }
  SMPC_TRY(st.finish());
  if (failed) { set_error("a goal field did not settle within world_x * world_y sweeps"); return SMPC_ERR_DEVICE; }
  return SMPC_OK;
}

int smpc_extract_plan_batch(smpc_handle* h, const smpc_extract_plan_in* in, double* plan, int32_t* plan_len, int32_t* error) {
  if (!h || !in || !plan || !plan_len) { set_error("null handle / input / plan / plan_len"); return SMPC_ERR_INVALID_ARG; }
  if (!in->world || !in->world_origin || !in->field || !in->goal || !in->robot_goal || !in->pose) { set_error("null input array"); return SMPC_ERR_INVALID_ARG; }
  if (in->B < 0 || in->G < 0 || in->L < 2 || in->stride < 1) { set_error("bad B / G, L < 2 or stride < 1"); return SMPC_ERR_INVALID_ARG; }
  smpc::ExtractPlanParams p;
  std::memset(&p, 0, sizeof(p));
  SMPC_TRY(check_plan_world(in->world_x, in->world_y, in->resolution, in->cost, &p.cost));
  SMPC_HIP_CHECK(hipSetDevice(h->device));
  p.B = in->B; p.G = in->G; p.L = in->L; p.stride = in->stride;
  p.world_x = in->world_x; p.world_y = in->world_y; p.world_shared = in->world_shared ? 1 : 0;
  p.resolution = in->resolution;
  const size_t B = in->B, G = in->G, cells = (size_t)in->world_x * in->world_y, nworld = in->world_shared ? 1 : G;
  Staging st(h, in->on_device);
  SMPC_TRY(st.in(p.world, in->world, nworld * cells));
  SMPC_TRY(st.in(p.world_origin, in->world_origin, nworld * 2));
  SMPC_TRY(st.in(p.field, in->field, G * cells));
  SMPC_TRY(st.in(p.goal, in->goal, G * 2));
  SMPC_TRY(st.in(p.robot_goal, in->robot_goal, B));
  SMPC_TRY(st.in(p.pose, in->pose, B * 3));
  // read and written: the rows the kernel leaves alone keep the caller's bytes on the way through device memory too
  SMPC_TRY(st.inout(p.plan, plan, B * (size_t)in->L * 2));
  SMPC_TRY(st.out(p.plan_len, plan_len, B));
  SMPC_TRY(st.out(p.error, error, B));
  if (B > 0) {
    const size_t per_block = smpc::kEpThreads / 8;
    SMPC_TRY(st.timed([&] {
      hipLaunchKernelGGL(smpc::smpc_extract_plan_kernel, dim3((unsigned)((B + per_block - 1) / per_block)), dim3(smpc::kEpThreads), 0, h->stream, p);
      return SMPC_OK;
    }));
  }
  return st.finish();
}

int smpc_visible_people_batch(smpc_handle* h, const smpc_visibility_in* in, double* visible, int32_t* visible_count, uint8_t* seen) {
  if (!h || !in || !visible || !visible_count) { set_error("null handle / input / visible / visible_count"); return SMPC_ERR_INVALID_ARG; }
  if (!in->world || !in->world_origin || !in->robot_pose || !in->people || !in->count) { set_error("null input array"); return SMPC_ERR_INVALID_ARG; }
  if (in->B < 0 || in->Np < 1 || in->world_x < 1 || in->world_y < 1) { set_error("bad B, Np < 1 or a non-positive world size"); return SMPC_ERR_INVALID_ARG; }
  if (!std::isfinite(in->resolution) || !(in->resolution > 0.0)) { set_error("resolution must be finite and > 0"); return SMPC_ERR_INVALID_ARG; }
  if (!std::isfinite(in->max_range) || !(in->max_range > 0.0)) { set_error("max_range must be finite and > 0"); return SMPC_ERR_INVALID_ARG; }
  // a ray of at most 32769 cells per axis: every product of the column rule fits 32 unsigned bits
  if (!(in->max_range / in->resolution <= 32768.0)) { set_error("max_range / resolution must not exceed 32768 cells"); return SMPC_ERR_UNSUPPORTED; }
  const int64_t cells = (int64_t)in->world_x * in->world_y;
  if (cells >= (int64_t)1 << 31) { set_error("a world of 2^31 cells or more is not supported"); return SMPC_ERR_UNSUPPORTED; }
  SMPC_HIP_CHECK(hipSetDevice(h->device));
  smpc::VisibilityParams p;
  std::memset(&p, 0, sizeof(p));
  p.B = in->B; p.Np = in->Np; p.world_x = in->world_x; p.world_y = in->world_y; p.world_shared = in->world_shared ? 1 : 0;
  p.occ.min_cost = in->occlusion_min_cost; p.occ.unknown = in->unknown_occludes ? 1u : 0u;
  p.resolution = in->resolution; p.max_range = in->max_range;
  const size_t B = in->B, Np = in->Np, nworld = in->world_shared ? 1 : B;
  Staging st(h, in->on_device);
  SMPC_TRY(st.in(p.world, in->world, nworld * (size_t)cells));
  SMPC_TRY(st.in(p.world_origin, in->world_origin, nworld * 2));
  SMPC_TRY(st.in(p.robot_pose, in->robot_pose, B * 3));
  SMPC_TRY(st.in(p.people, in->people, B * Np * 5));
  SMPC_TRY(st.in(p.count, in->count, B));
  // read and written: the rows and flags the kernel leaves alone keep the caller's bytes on the way through device memory too
  SMPC_TRY(st.inout(p.visible, visible, B * Np * 5));
  SMPC_TRY(st.out(p.visible_count, visible_count, B));
  SMPC_TRY(st.inout(p.seen, seen, B * Np));
  if (B > 0) {
    const size_t per_block = smpc::kVisThreads / 64;
    SMPC_TRY(st.timed([&] {
      hipLaunchKernelGGL(smpc::smpc_visible_people_kernel, dim3((unsigned)((B + per_block - 1) / per_block)), dim3(smpc::kVisThreads), 0, h->stream, p);
      return SMPC_OK;
    }));
  }
  return st.finish();
}

static_assert(smpc::kSensedReach == SMPC_SENSED_MAX_REACH && smpc::kScSide == SMPC_SENSED_MAX_SIZE && smpc::kScMaxD2 == SMPC_SENSED_MAX_D2,
              "smpc_sensed_costmap.h and the kernel disagree on a limit");

// floor(sqrt(v)) for 0 <= v < 2^31
static int32_t isqrt_i32(int32_t v) {
  int64_t r = (int64_t)std::sqrt((double)v);
  while (r * r > v) --r;
  while ((r + 1) * (r + 1) <= v) ++r;
  return (int32_t)r;
}

// the refusals of smpc_sensed_costmap_batch on its input struct (smpc_obstacle_memory_batch has the same on `scan`)
static int sensed_check(const smpc_sensed_costmap_in* in) {
  if (!in->world || !in->world_origin || !in->robot_pose || !in->people || !in->count || !in->cell || !in->beam_cells || !in->inflation_cost) {
    set_error("null input array"); return SMPC_ERR_INVALID_ARG;
  }
  if (in->B < 0 || in->Np < 1 || in->size_x < 1 || in->size_y < 1 || in->world_x < 1 || in->world_y < 1) {
    set_error("bad B, Np < 1 or a non-positive window / world size"); return SMPC_ERR_INVALID_ARG;
  }
  if (!std::isfinite(in->resolution) || !(in->resolution > 0.0)) { set_error("resolution must be finite and > 0"); return SMPC_ERR_INVALID_ARG; }
  if (in->n_beams < 1 || in->agent_d2 < 0 || in->d2_max < 0 || in->base > 1) {
    set_error("n_beams < 1, a negative agent_d2 or d2_max, or base > 1"); return SMPC_ERR_INVALID_ARG;
  }
  if (in->size_x > SMPC_SENSED_MAX_SIZE || in->size_y > SMPC_SENSED_MAX_SIZE) { set_error("a window side of more than 256 cells is not supported"); return SMPC_ERR_UNSUPPORTED; }
  if (in->d2_max > SMPC_SENSED_MAX_D2) { set_error("d2_max > 1024 is not supported"); return SMPC_ERR_UNSUPPORTED; }
  if (in->n_beams > SMPC_SENSED_MAX_BEAMS) { set_error("more than 4096 beams are not supported"); return SMPC_ERR_UNSUPPORTED; }
  if ((int64_t)in->world_x * in->world_y >= (int64_t)1 << 31) { set_error("a world of 2^31 cells or more is not supported"); return SMPC_ERR_UNSUPPORTED; }
  return SMPC_OK;
}

// the kernel's view of a checked input struct with B > 0: scalars, staged arrays and the store path
static int sensed_params(Staging& st, const smpc_sensed_costmap_in* in, uint8_t* costmap, uint8_t* beam_kind, int32_t* beam_cell,
                         smpc::SensedCostmapParams& p) {
  std::memset(&p, 0, sizeof(p));
  p.B = in->B; p.Np = in->Np; p.size_x = in->size_x; p.size_y = in->size_y; p.world_x = in->world_x; p.world_y = in->world_y;
  p.world_shared = in->world_shared ? 1 : 0; p.n_beams = in->n_beams;
  p.agent_d2 = in->agent_d2; p.agent_r = isqrt_i32(in->agent_d2); p.d2_max = in->d2_max; p.r = isqrt_i32(in->d2_max);
  p.base = in->base; p.outside = 0x01010101u * in->outside_cost;
  p.occ.min_cost = in->occlusion_min_cost; p.occ.unknown = in->unknown_occludes ? 1u : 0u;
  p.resolution = in->resolution;
  const size_t B = in->B, Np = in->Np, nworld = in->world_shared ? 1 : B, cells = (size_t)in->size_x * (size_t)in->size_y, K = in->n_beams;
  const size_t world_cells = (size_t)in->world_x * (size_t)in->world_y;
  SMPC_TRY(st.in(p.world, in->world, nworld * world_cells));
  SMPC_TRY(st.in(p.world_origin, in->world_origin, nworld * 2));
  SMPC_TRY(st.in(p.robot_pose, in->robot_pose, B * 3));
  SMPC_TRY(st.in(p.people, in->people, B * Np * 5));
  SMPC_TRY(st.in(p.count, in->count, B));
  SMPC_TRY(st.in(p.cell, in->cell, B * 2));
  SMPC_TRY(st.in(p.beam_cells, in->beam_cells, K * 2));
  SMPC_TRY(st.in(p.inflation_cost, in->inflation_cost, (size_t)in->d2_max + 1));
  SMPC_TRY(st.out(p.costmap, costmap, B * cells));
  SMPC_TRY(st.out(p.beam_kind, beam_kind, B * K));
  SMPC_TRY(st.out(p.beam_cell, beam_cell, B * K * 2));
  // 16-byte stores need every window to start on a 16-byte boundary and every 8-byte half to lie in one window row
  p.wide = (in->size_x % 8 == 0 && cells % 16 == 0 && reinterpret_cast<uintptr_t>(p.costmap) % 16 == 0) ? 1 : 0;
  return SMPC_OK;
}

int smpc_sensed_costmap_batch(smpc_handle* h, const smpc_sensed_costmap_in* in, uint8_t* costmap, uint8_t* beam_kind, int32_t* beam_cell) {
  if (!h || !in || !costmap) { set_error("null handle / input / costmap"); return SMPC_ERR_INVALID_ARG; }
  SMPC_TRY(sensed_check(in));
  if (in->B == 0) return SMPC_OK;
  SMPC_HIP_CHECK(hipSetDevice(h->device));
  smpc::SensedCostmapParams p;
  Staging st(h, in->on_device);
  SMPC_TRY(sensed_params(st, in, costmap, beam_kind, beam_cell, p));
  // one workgroup per robot (a loop over the robots inside the kernel kept every argument alive and spilled SGPRs); the
  // grid is folded so that no dimension exceeds 2^15 x 2^16 workgroups
  const size_t B = in->B, gx = B < 32768 ? B : 32768, gy = (B + gx - 1) / gx;
  SMPC_TRY(st.timed([&] {
    hipLaunchKernelGGL(smpc::smpc_sensed_costmap_kernel, dim3((unsigned)gx, (unsigned)gy), dim3(smpc::kScThreads), 0, h->stream, p);
    return SMPC_OK;
  }));
  return st.finish();
}

int smpc_obstacle_memory_batch(smpc_handle* h, const smpc_obstacle_memory_in* in, uint32_t* memory, int32_t* memory_cell, uint8_t* costmap,
                               uint8_t* beam_kind, int32_t* beam_cell) {
  if (!h || !in || !costmap) { set_error("null handle / input / costmap"); return SMPC_ERR_INVALID_ARG; }
  if (!memory || !memory_cell) { set_error("null memory / memory_cell"); return SMPC_ERR_INVALID_ARG; }
  SMPC_TRY(sensed_check(&in->scan));
  if (in->mark_d2 < 0 || in->footprint_d2 < -1) { set_error("mark_d2 < 0 or footprint_d2 < -1"); return SMPC_ERR_INVALID_ARG; }
  if (in->scan.B == 0) return SMPC_OK;
  SMPC_HIP_CHECK(hipSetDevice(h->device));
  smpc::ObstacleMemoryParams p;
  std::memset(&p, 0, sizeof(p));
  Staging st(h, in->scan.on_device);
  SMPC_TRY(sensed_params(st, &in->scan, costmap, beam_kind, beam_cell, p.sc));
  p.mark_d2 = in->mark_d2; p.footprint_d2 = in->footprint_d2;
  p.footprint_r = in->footprint_d2 >= 0 ? isqrt_i32(in->footprint_d2) : -1;
  const size_t B = in->scan.B, words = ((size_t)in->scan.size_x + 31) / 32;
  SMPC_TRY(st.inout(p.memory, memory, B * (size_t)in->scan.size_y * words));
  SMPC_TRY(st.inout(p.memory_cell, memory_cell, B * 2));
  const size_t gx = B < 32768 ? B : 32768, gy = (B + gx - 1) / gx;  // one workgroup per robot, folded as above
  SMPC_TRY(st.timed([&] {
    hipLaunchKernelGGL(smpc::smpc_obstacle_memory_kernel, dim3((unsigned)gx, (unsigned)gy), dim3(smpc::kScThreads), 0, h->stream, p);
    return SMPC_OK;
  }));
  return st.finish();
}

int smpc_track_people_batch(smpc_handle* h, const smpc_tracker_in* in, double* tracks, int32_t* track_meta, int32_t* next_id, double* people,
                            int32_t* count, int32_t* out_track) {
  if (!h || !in || !tracks || !track_meta || !next_id || !people || !count) {
    set_error("null handle / input / tracks / track_meta / next_id / people / count"); return SMPC_ERR_INVALID_ARG;
  }
  if (!in->detections || !in->det_count || !in->robot_pose) { set_error("null input array"); return SMPC_ERR_INVALID_ARG; }
  if (in->B < 0 || in->Nd < 1 || in->Nt < 1 || in->Np < 1) { set_error("bad B, or Nd, Nt or Np < 1"); return SMPC_ERR_INVALID_ARG; }
  if (in->confirm_hits < 1 || in->max_missed < 0) { set_error("confirm_hits < 1 or max_missed < 0"); return SMPC_ERR_INVALID_ARG; }
  if (!std::isfinite(in->dt) || !(in->dt > 0.0)) { set_error("dt must be finite and > 0"); return SMPC_ERR_INVALID_ARG; }
  if (!std::isfinite(in->gate) || !(in->gate > 0.0)) { set_error("gate must be finite and > 0"); return SMPC_ERR_INVALID_ARG; }
  if (!std::isfinite(in->alpha) || !(in->alpha >= 0.0) || !std::isfinite(in->gain) || !(in->gain >= 0.0)) {
    set_error("alpha and gain must be finite and >= 0"); return SMPC_ERR_INVALID_ARG;
  }
  // the kernel's bounds: lane i owns slot i, detection i and output rank i of one wavefront
  if (in->Nd > SMPC_MAX_AGENTS || in->Nt > SMPC_MAX_AGENTS || in->Np > SMPC_MAX_AGENTS) {
    set_error("Nd, Nt or Np > 64 is not supported"); return SMPC_ERR_UNSUPPORTED;
  }
  if (in->B == 0) return SMPC_OK;
  SMPC_HIP_CHECK(hipSetDevice(h->device));
  smpc::TrackerParams p;
  std::memset(&p, 0, sizeof(p));
  p.B = in->B; p.Nd = in->Nd; p.Nt = in->Nt; p.Np = in->Np; p.confirm_hits = in->confirm_hits; p.max_missed = in->max_missed;
  p.dt = in->dt; p.alpha = in->alpha; p.gain = in->gain; p.gate = in->gate;
  const size_t B = in->B, Nd = in->Nd, Nt = in->Nt, Np = in->Np;
  Staging st(h, in->on_device);
  SMPC_TRY(st.in(p.detections, in->detections, B * Nd * 5));
  SMPC_TRY(st.in(p.det_count, in->det_count, B));
  SMPC_TRY(st.in(p.robot_pose, in->robot_pose, B * 3));
  SMPC_TRY(st.inout(p.tracks, tracks, B * Nt * 4));
  SMPC_TRY(st.inout(p.meta, track_meta, B * Nt * 4));
  SMPC_TRY(st.inout(p.next_id, next_id, B));
  // read and written: the rows the kernel leaves alone keep the caller's bytes on the way through device memory too
  SMPC_TRY(st.inout(p.people, people, B * Np * 5));
  SMPC_TRY(st.out(p.count, count, B));
  SMPC_TRY(st.inout(p.out_track, out_track, B * Np * 2));
  const size_t per_block = smpc::kTkThreads / 64;
  SMPC_TRY(st.timed([&] {
    hipLaunchKernelGGL(smpc::smpc_track_people_kernel, dim3((unsigned)((B + per_block - 1) / per_block)), dim3(smpc::kTkThreads), 0, h->stream, p);
    return SMPC_OK;
  }));
  return st.finish();
}

int smpc_detect_people_batch(smpc_handle* h, const smpc_detector_in* in, uint32_t* draw_state, double* detections, int32_t* det_count,
                             int32_t* det_source, uint8_t* outcome) {
  if (!h || !in || !draw_state || !detections || !det_count) {
    set_error("null handle / input / draw_state / detections / det_count"); return SMPC_ERR_INVALID_ARG;
  }
  if (!in->people || !in->count || !in->robot_pose) { set_error("null input array"); return SMPC_ERR_INVALID_ARG; }
  if (in->B < 0 || in->Np < 1 || in->Nd < 1 || in->Kc < 0) { set_error("bad B, Np or Nd < 1, or Kc < 0"); return SMPC_ERR_INVALID_ARG; }
  for (const double v : {in->body_radius, in->noise_scale, in->noise_growth, in->clutter_scale})
    if (!std::isfinite(v) || !(v >= 0.0)) {
      set_error("body_radius, noise_scale, noise_growth and clutter_scale must be finite and >= 0"); return SMPC_ERR_INVALID_ARG;
    }
  // the kernel's bounds: lane j owns person j, clutter candidate j and at most one output rank of one wavefront
  if (in->Np > SMPC_MAX_AGENTS || in->Nd > SMPC_MAX_AGENTS || in->Kc > SMPC_MAX_AGENTS) {
    set_error("Np, Nd or Kc > 64 is not supported"); return SMPC_ERR_UNSUPPORTED;
  }
  if (in->B == 0) return SMPC_OK;
  SMPC_HIP_CHECK(hipSetDevice(h->device));
  smpc::DetectorParams p;
  std::memset(&p, 0, sizeof(p));
  p.B = in->B; p.Np = in->Np; p.Nd = in->Nd; p.Kc = in->Kc;
  p.seed_lo = in->seed_lo; p.seed_hi = in->seed_hi; p.miss_threshold = in->miss_threshold; p.clutter_threshold = in->clutter_threshold;
  p.body_radius = in->body_radius; p.noise_scale = in->noise_scale; p.noise_growth = in->noise_growth; p.clutter_scale = in->clutter_scale;
  const size_t B = in->B, Np = in->Np, Nd = in->Nd;
  Staging st(h, in->on_device);
  SMPC_TRY(st.in(p.people, in->people, B * Np * 5));
  SMPC_TRY(st.in(p.count, in->count, B));
  SMPC_TRY(st.in(p.robot_pose, in->robot_pose, B * 3));
  SMPC_TRY(st.inout(p.draw_state, draw_state, B * 2));
  // read and written: the rows the kernel leaves alone keep the caller's bytes on the way through device memory too
  SMPC_TRY(st.inout(p.detections, detections, B * Nd * 5));
  SMPC_TRY(st.out(p.det_count, det_count, B));
  SMPC_TRY(st.inout(p.det_source, det_source, B * Nd));
  SMPC_TRY(st.inout(p.outcome, outcome, B * Np));
  const size_t per_block = smpc::kDtThreads / 64;
  SMPC_TRY(st.timed([&] {
    hipLaunchKernelGGL(smpc::smpc_detect_people_kernel, dim3((unsigned)((B + per_block - 1) / per_block)), dim3(smpc::kDtThreads), 0, h->stream, p);
    return SMPC_OK;
  }));
  return st.finish();
}

int smpc_robot_plant_batch(smpc_handle* h, const smpc_plant_in* in, double* pose, double* twist, double* cmd_queue, uint32_t* plant_tick,
                           int32_t* contact, double* heading_cs) {
  if (!h || !in || !pose || !twist || !plant_tick || !contact) {
    set_error("null handle / input / pose / twist / plant_tick / contact"); return SMPC_ERR_INVALID_ARG;
  }
  if (!in->cmd || !in->agents || !in->count) { set_error("null input array"); return SMPC_ERR_INVALID_ARG; }
  if (in->B < 0 || in->Np < 1 || in->S < 1 || in->L < 0 || in->footprint_d2 < -1) {
    set_error("bad B, Np or S < 1, L < 0 or footprint_d2 < -1"); return SMPC_ERR_INVALID_ARG;
  }
  if (in->L > 0 && !cmd_queue) { set_error("null cmd_queue with L > 0"); return SMPC_ERR_INVALID_ARG; }
  for (const double v : {in->dt, in->w_max, in->contact_dist})
    if (!std::isfinite(v) || !(v >= 0.0)) { set_error("dt, w_max and contact_dist must be finite and >= 0"); return SMPC_ERR_INVALID_ARG; }
  if (!std::isfinite(in->v_min) || !std::isfinite(in->v_max) || !(in->v_min <= in->v_max)) {
    set_error("v_min and v_max must be finite with v_min <= v_max"); return SMPC_ERR_INVALID_ARG;
  }
  if (!std::isfinite(in->resolution) || !(in->resolution > 0.0)) { set_error("resolution must be finite and > 0"); return SMPC_ERR_INVALID_ARG; }
  for (const double v : {in->dv_up, in->dv_down, in->dw})
    if (!(v >= 0.0)) { set_error("dv_up, dv_down and dw must be >= 0 (+inf allowed)"); return SMPC_ERR_INVALID_ARG; }
  if (in->world && (in->Hx < 1 || in->Hy < 1)) { set_error("world given with Hx or Hy < 1"); return SMPC_ERR_INVALID_ARG; }
  // the kernel's bounds: lane j owns agent j, the queue has 8 slots, the footprint's square at most 31 x 31 offsets
  if (in->Np > SMPC_MAX_AGENTS || in->S > SMPC_PLANT_MAX_SUBSTEPS || in->L > SMPC_PLANT_MAX_LATENCY ||
      in->footprint_d2 > SMPC_PLANT_MAX_FOOTPRINT_D2) {
    set_error("Np > 64, S > 16, L > 8 or footprint_d2 > 225 is not supported"); return SMPC_ERR_UNSUPPORTED;
  }
  if (in->B == 0) return SMPC_OK;
  SMPC_HIP_CHECK(hipSetDevice(h->device));
  smpc::PlantParams p;
  std::memset(&p, 0, sizeof(p));
  p.B = in->B; p.Np = in->Np; p.S = in->S; p.L = in->L;
  p.dt = in->dt; p.v_min = in->v_min; p.v_max = in->v_max; p.w_max = in->w_max;
  p.dv_up = in->dv_up; p.dv_down = in->dv_down; p.dw = in->dw; p.contact2 = smpc::pl_contact2(in->contact_dist);
  p.res = in->resolution; p.ox = in->world_origin[0]; p.oy = in->world_origin[1];
  const bool walls = in->world != nullptr && in->footprint_d2 >= 0;
  p.walls.Hx = in->Hx; p.walls.Hy = in->Hy; p.walls.footprint_d2 = walls ? in->footprint_d2 : -1;
  p.walls.r = walls ? smpc::pl_isqrt(in->footprint_d2) : 0;
  p.walls.min_cost = in->wall_min_cost; p.walls.unknown = in->unknown_is_wall ? 1 : 0; p.walls.outside = in->outside_is_wall ? 1 : 0;
  smpc::fill_math_table(&p.mt);
  const size_t B = in->B, Np = in->Np;
  Staging st(h, in->on_device);
  SMPC_TRY(st.in(p.walls.world, walls ? in->world : nullptr, (size_t)in->Hx * (size_t)in->Hy));
  SMPC_TRY(st.in(p.cmd, in->cmd, B * 2));
  SMPC_TRY(st.in(p.agents, in->agents, B * Np * 5));
  SMPC_TRY(st.in(p.count, in->count, B));
  SMPC_TRY(st.inout(p.pose, pose, B * 3));
  SMPC_TRY(st.inout(p.twist, twist, B * 2));
  SMPC_TRY(st.inout(p.queue, in->L > 0 ? cmd_queue : nullptr, B * SMPC_PLANT_MAX_LATENCY * 2));
  SMPC_TRY(st.inout(p.tick, plant_tick, B));
  SMPC_TRY(st.out(p.contact, contact, B * 2));
  // read and written: the row of a robot whose state is not finite keeps the caller's bytes on the way through device memory too
  SMPC_TRY(st.inout(p.heading, heading_cs, B * 2));
  const size_t per_block = smpc::kPlThreads / 64;
  SMPC_TRY(st.timed([&] {
    hipLaunchKernelGGL(smpc::smpc_robot_plant_kernel, dim3((unsigned)((B + per_block - 1) / per_block)), dim3(smpc::kPlThreads), 0, h->stream, p);
    return SMPC_OK;
  }));
  return st.finish();
}

int smpc_collision_monitor_batch(smpc_handle* h, const smpc_collision_monitor_in* in, double* cmd_out, int32_t* action, int32_t* zone_points,
                                 double* ratio, double* heading_cs, double* step_cs) {
  if (!h || !in || !cmd_out || !action) { set_error("null handle / input / cmd_out / action"); return SMPC_ERR_INVALID_ARG; }
  if (!in->zones || !in->robot_pose || !in->cmd || !in->beam_kind || !in->beam_cell) { set_error("null input array"); return SMPC_ERR_INVALID_ARG; }
  if (cmd_out == in->cmd) { set_error("cmd_out must not be the buffer of cmd"); return SMPC_ERR_INVALID_ARG; }
  if (in->B < 0 || in->Z < 1 || in->n_beams < 1 || in->M < 0) { set_error("bad B, Z or n_beams < 1, or M < 0"); return SMPC_ERR_INVALID_ARG; }
  if (!std::isfinite(in->resolution) || !(in->resolution > 0.0)) { set_error("resolution must be finite and > 0"); return SMPC_ERR_INVALID_ARG; }
  if (in->M > 0 && (!std::isfinite(in->sim_dt) || !(in->sim_dt > 0.0))) { set_error("sim_dt must be finite and > 0 with M > 0"); return SMPC_ERR_INVALID_ARG; }
  // the kernel's bounds: the zones travel in the kernel arguments, a lane holds 8 points of a chunk, a zone 16 vertices
  if (in->Z > SMPC_MONITOR_MAX_ZONES || in->M > SMPC_MONITOR_MAX_STEPS || in->n_beams > SMPC_SENSED_MAX_BEAMS) {
    set_error("Z > 8, M > 32 or n_beams > 4096 is not supported"); return SMPC_ERR_UNSUPPORTED;
  }
  smpc::MonitorParams p;
  std::memset(&p, 0, sizeof(p));
  for (int zi = 0; zi < in->Z; ++zi) {
    const smpc_monitor_zone& z = in->zones[zi];
    smpc::MonitorZone& k = p.zones[zi];
    if ((z.shape != SMPC_MONITOR_CIRCLE && z.shape != SMPC_MONITOR_POLYGON) || z.action < SMPC_MONITOR_STOP || z.action > SMPC_MONITOR_APPROACH) {
      set_error("zone: unknown shape or action"); return SMPC_ERR_INVALID_ARG;
    }
    if (z.shape == SMPC_MONITOR_POLYGON && (z.n_vertices < 3 || z.n_vertices > SMPC_MONITOR_MAX_VERTICES)) {
      set_error("zone: a polygon has 3..16 vertices"); return SMPC_ERR_INVALID_ARG;
    }
    if (z.min_points < 1) { set_error("zone: min_points < 1"); return SMPC_ERR_INVALID_ARG; }
    if (!std::isfinite(z.radius) || !(z.radius >= 0.0) || !(z.linear_limit >= 0.0) || !(z.angular_limit >= 0.0)) {
      set_error("zone: radius must be finite and >= 0, the limits >= 0"); return SMPC_ERR_INVALID_ARG;
    }
    if (!(z.slowdown_ratio >= 0.0 && z.slowdown_ratio <= 1.0)) { set_error("zone: slowdown_ratio outside [0, 1]"); return SMPC_ERR_INVALID_ARG; }
    if (z.action == SMPC_MONITOR_APPROACH && in->M == 0) { set_error("an APPROACH zone needs M >= 1"); return SMPC_ERR_INVALID_ARG; }
    k.shape = z.shape; k.action = z.action; k.min_points = z.min_points;
    k.n = z.shape == SMPC_MONITOR_POLYGON ? z.n_vertices : 0;
    for (int i = 0; i < k.n; ++i) {
      if (!std::isfinite(z.vertices[i][0]) || !std::isfinite(z.vertices[i][1])) { set_error("zone: vertex not finite"); return SMPC_ERR_INVALID_ARG; }
      k.vx[i] = z.vertices[i][0]; k.vy[i] = z.vertices[i][1];
    }
    k.radius2 = smpc::cm_radius2(z.radius); k.slowdown_ratio = z.slowdown_ratio;
    k.linear_limit = z.linear_limit; k.angular_limit = z.angular_limit;
    k.bound = smpc::cm_bound(k.shape, z.radius, k.n, k.vx, k.vy);
  }
  if (in->B == 0) return SMPC_OK;
  SMPC_HIP_CHECK(hipSetDevice(h->device));
  p.B = in->B; p.n_beams = in->n_beams; p.Z = in->Z; p.M = in->M;
  p.sim_dt = in->M > 0 ? in->sim_dt : 0.0; p.res = in->resolution; p.ox = in->world_origin[0]; p.oy = in->world_origin[1];
  smpc::fill_math_table(&p.mt);
  const size_t B = in->B, n = in->n_beams;
  Staging st(h, in->on_device);
  SMPC_TRY(st.in(p.pose, in->robot_pose, B * 3));
  SMPC_TRY(st.in(p.cmd, in->cmd, B * 2));
  SMPC_TRY(st.in(p.kind, in->beam_kind, B * n));
  SMPC_TRY(st.in(p.cell, in->beam_cell, B * n * 2));
  SMPC_TRY(st.out(p.cmd_out, cmd_out, B * 2));
  SMPC_TRY(st.out(p.action, action, B * 4));
  SMPC_TRY(st.out(p.zone_points, zone_points, B * (size_t)in->Z));
  SMPC_TRY(st.out(p.ratio, ratio, B));
  // read and written: the rows the rule does not write keep the caller's bytes on the way through device memory too
  SMPC_TRY(st.inout(p.heading, heading_cs, B * 2));
  SMPC_TRY(st.inout(p.step, step_cs, B * 2));
  const size_t per_block = smpc::kCmThreads / 64;
  const dim3 grid((unsigned)((B + per_block - 1) / per_block)), block(smpc::kCmThreads);
  SMPC_TRY(st.timed([&] {
    if (in->n_beams <= 64 * smpc::kCmSlots) hipLaunchKernelGGL(smpc::smpc_collision_monitor_kernel<true>, grid, block, 0, h->stream, p);
    else hipLaunchKernelGGL(smpc::smpc_collision_monitor_kernel<false>, grid, block, 0, h->stream, p);
    return SMPC_OK;
  }));
  return st.finish();
}

int smpc_scan_people_batch(smpc_handle* h, const smpc_scan_people_in* in, double* detections, int32_t* det_count, int32_t* det_segment,
                           int32_t* seg_stats) {
  if (!h || !in || !detections || !det_count) { set_error("null handle / input / detections / det_count"); return SMPC_ERR_INVALID_ARG; }
  if (!in->robot_pose || !in->beam_kind || !in->beam_cell) { set_error("null input array"); return SMPC_ERR_INVALID_ARG; }
  if (in->B < 0 || in->n_beams < 1 || in->Nd < 1 || in->min_points < 1) { set_error("bad B, or n_beams, Nd or min_points < 1"); return SMPC_ERR_INVALID_ARG; }
  if (in->link_d2 < 0 || in->width_d2_min < 0 || in->width_d2_max < 0 || in->range_d2 < 0 || in->width_d2_min > in->width_d2_max) {
    set_error("link_d2, width_d2_min, width_d2_max and range_d2 must be >= 0, width_d2_min <= width_d2_max"); return SMPC_ERR_INVALID_ARG;
  }
  if (in->subtract_map < 0 || in->subtract_map > 1) { set_error("subtract_map must be 0 or 1"); return SMPC_ERR_INVALID_ARG; }
  if (!std::isfinite(in->resolution) || !(in->resolution > 0.0)) { set_error("resolution must be finite and > 0"); return SMPC_ERR_INVALID_ARG; }
  if (!std::isfinite(in->world_origin[0]) || !std::isfinite(in->world_origin[1])) { set_error("world_origin must be finite"); return SMPC_ERR_INVALID_ARG; }
  if (!std::isfinite(in->body_offset) || !(in->body_offset >= 0.0)) { set_error("body_offset must be finite and >= 0"); return SMPC_ERR_INVALID_ARG; }
  // the kernel's bounds: an output rank is below 64, the running sums of 4096 offsets fit 32 bits
  if (in->n_beams > SMPC_SENSED_MAX_BEAMS || in->Nd > SMPC_MAX_AGENTS) { set_error("n_beams > 4096 or Nd > 64 is not supported"); return SMPC_ERR_UNSUPPORTED; }
  if (in->B == 0) return SMPC_OK;
  SMPC_HIP_CHECK(hipSetDevice(h->device));
  smpc::ScanPeopleParams p;
  std::memset(&p, 0, sizeof(p));
  p.B = in->B; p.n_beams = in->n_beams; p.Nd = in->Nd; p.subtract_map = in->subtract_map; p.min_points = in->min_points;
  p.link_d2 = in->link_d2; p.width_d2_min = in->width_d2_min; p.width_d2_max = in->width_d2_max; p.range_d2 = in->range_d2;
  p.res = in->resolution; p.ox = in->world_origin[0]; p.oy = in->world_origin[1]; p.body_offset = in->body_offset;
  const size_t B = in->B, n = in->n_beams, Nd = in->Nd;
  Staging st(h, in->on_device);
  SMPC_TRY(st.in(p.pose, in->robot_pose, B * 3));
  SMPC_TRY(st.in(p.kind, in->beam_kind, B * n));
  SMPC_TRY(st.in(p.cell, in->beam_cell, B * n * 2));
  // read and written: the rows the rule does not write keep the caller's bytes on the way through device memory too
  SMPC_TRY(st.inout(p.detections, detections, B * Nd * 5));
  SMPC_TRY(st.out(p.det_count, det_count, B));
  SMPC_TRY(st.inout(p.det_segment, det_segment, B * Nd * 4));
  SMPC_TRY(st.out(p.seg_stats, seg_stats, B * 4));
  const size_t per_block = smpc::kSpThreads / 64;
  SMPC_TRY(st.timed([&] {
    hipLaunchKernelGGL(smpc::smpc_scan_people_kernel, dim3((unsigned)((B + per_block - 1) / per_block)), dim3(smpc::kSpThreads), 0, h->stream, p);
    return SMPC_OK;
  }));
  return st.finish();
}

int smpc_repair_plan_batch(smpc_handle* h, const smpc_plan_repair_in* in, double* plan, int32_t* plan_len, double* workspace, int32_t* status,
                           int32_t* info, uint32_t* field) {
  if (!h || !in || !plan || !plan_len || !workspace || !status) { set_error("null handle / input / plan / plan_len / workspace / status"); return SMPC_ERR_INVALID_ARG; }
  if (!in->costmap || !in->costmap_origin || !in->robot_pose) { set_error("null input array"); return SMPC_ERR_INVALID_ARG; }
  if (in->B < 0 || in->L < 2 || in->size_x < 1 || in->size_y < 1 || in->radius < 1 || in->stride < 1) {
    set_error("bad B, L < 2, or a size, radius or stride < 1"); return SMPC_ERR_INVALID_ARG;
  }
  if (!std::isfinite(in->resolution) || !(in->resolution > 0.0)) { set_error("resolution must be finite and > 0"); return SMPC_ERR_INVALID_ARG; }
  if (!std::isfinite(in->clearance_d2) || !(in->clearance_d2 >= 0.0)) { set_error("clearance_d2 must be finite and >= 0"); return SMPC_ERR_INVALID_ARG; }
  const smpc_plan_cost_params& c = in->cost;
  if (c.neutral_cost < 1 || c.cost_weight < 0) { set_error("neutral_cost must be >= 1 and cost_weight >= 0"); return SMPC_ERR_INVALID_ARG; }
  const int64_t w_max = (int64_t)c.neutral_cost + 255 * (int64_t)c.cost_weight;
  if (w_max > 65535) { set_error("neutral_cost + 255 * cost_weight must be <= 65535"); return SMPC_ERR_INVALID_ARG; }
  if (in->radius > SMPC_REPAIR_MAX_RADIUS) { set_error("radius above SMPC_REPAIR_MAX_RADIUS is not supported"); return SMPC_ERR_UNSUPPORTED; }
  const int64_t S = 2 * (int64_t)in->radius + 1;
  if (S * S * 7 * w_max >= ((int64_t)1 << 32) - 1) {
    set_error("S * S * 7 * (neutral_cost + 255 * cost_weight) must stay below 2^32 - 1: potentials are 32 bits"); return SMPC_ERR_UNSUPPORTED;
  }
  if (in->B == 0) return SMPC_OK;
  SMPC_HIP_CHECK(hipSetDevice(h->device));
  smpc::PlanRepairParams p;
  std::memset(&p, 0, sizeof(p));
  p.B = in->B; p.L = in->L; p.size_x = in->size_x; p.size_y = in->size_y; p.costmap_shared = in->costmap_shared ? 1 : 0;
  p.R = in->radius; p.stride = in->stride; p.res = in->resolution; p.clearance_d2 = in->clearance_d2;
  p.cost.neutral = c.neutral_cost; p.cost.weight = c.cost_weight; p.cost.lethal_min = c.lethal_min_cost; p.cost.allow_unknown = c.allow_unknown ? 1u : 0u;
  const size_t B = in->B, L = in->L, nmap = in->costmap_shared ? 1 : B;
  Staging st(h, in->on_device);
  SMPC_TRY(st.in(p.costmap, in->costmap, nmap * (size_t)in->size_x * in->size_y));
  SMPC_TRY(st.in(p.origin, in->costmap_origin, nmap * 2));
  SMPC_TRY(st.in(p.pose, in->robot_pose, B * 3));
  SMPC_TRY(st.in(p.plan_start, in->plan_start, B));
  // read and written: what the rule leaves alone keeps the caller's bytes on the way through device memory too
  SMPC_TRY(st.inout(p.plan, plan, B * L * 2));
  SMPC_TRY(st.inout(p.plan_len, plan_len, B));
  SMPC_TRY(st.out(p.status, status, B));
  SMPC_TRY(st.out(p.info, info, B * 4));
  SMPC_TRY(st.inout(p.field, field, B * (size_t)(S * S)));
  void* ws = workspace;  // a host-pointer call's workspace is device room of the call's own
  SMPC_TRY(st.scratch(ws, B * L * 2 * sizeof(double)));
  p.workspace = static_cast<double*>(ws);
  const size_t lds = smpc::pr_field_lds_bytes(in->radius);
  if (lds > 64 * 1024) {
    SMPC_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(smpc::smpc_repair_field_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  }
  // a wavefront per row of a colour: R + 1 rows at the most, 16 wavefronts at the most
  const unsigned field_threads = 64u * (unsigned)(in->radius + 1 < smpc::kPrFieldMaxThreads / 64 ? in->radius + 1 : smpc::kPrFieldMaxThreads / 64);
  const size_t field_grid = B < (size_t)h->num_cu * 4 ? B : (size_t)h->num_cu * 4;
  const size_t per_block = smpc::kPrJudgeThreads / 64;
  SMPC_TRY(st.timed([&] {
    hipLaunchKernelGGL(smpc::smpc_repair_judge_kernel, dim3((unsigned)((B + per_block - 1) / per_block)), dim3(smpc::kPrJudgeThreads), 0, h->stream, p);
    hipLaunchKernelGGL(smpc::smpc_repair_field_kernel, dim3((unsigned)field_grid), dim3(field_threads), lds, h->stream, p);
    return SMPC_OK;
  }));
  return st.finish();
}

int smpc_smooth_plan_batch(smpc_handle* h, const smpc_plan_smoother_in* in, double* plan, int32_t* status, int32_t* info, double* change) {
  if (!h || !in || !plan || !status) { set_error("null handle / input / plan / status"); return SMPC_ERR_INVALID_ARG; }
  if (!in->world || !in->world_origin || !in->plan_len) { set_error("null input array"); return SMPC_ERR_INVALID_ARG; }
  if (in->B < 0 || in->L < 2 || in->world_x < 1 || in->world_y < 1) { set_error("bad B, L < 2, or a world side < 1"); return SMPC_ERR_INVALID_ARG; }
  if (!std::isfinite(in->resolution) || !(in->resolution > 0.0)) { set_error("resolution must be finite and > 0"); return SMPC_ERR_INVALID_ARG; }
  if (!std::isfinite(in->w_data) || !(in->w_data > 0.0)) { set_error("w_data must be finite and > 0"); return SMPC_ERR_INVALID_ARG; }
  if (!std::isfinite(in->w_smooth) || !(in->w_smooth >= 0.0)) { set_error("w_smooth must be finite and >= 0"); return SMPC_ERR_INVALID_ARG; }
  {
    const volatile double four = 4.0 * in->w_smooth;  // the product, rounded, then the sum
    const volatile double sum = in->w_data + four;
    if (!(sum < 2.0)) { set_error("w_data + 4 * w_smooth must be < 2: the sweep would not contract"); return SMPC_ERR_INVALID_ARG; }
  }
  if (!(in->tolerance >= 0.0)) { set_error("tolerance must be >= 0"); return SMPC_ERR_INVALID_ARG; }
  if (in->max_its < 1 || in->refinement_num < 0) { set_error("max_its < 1 or refinement_num < 0"); return SMPC_ERR_INVALID_ARG; }
  // the kernel's bounds: a lane holds 16 slots, the sweep counters are 32 bits, a cell index is an int32
  if (in->L > SMPC_SMOOTH_MAX_POSES || in->max_its > SMPC_SMOOTH_MAX_ITS || in->refinement_num > SMPC_SMOOTH_MAX_REFINEMENTS) {
    set_error("L > 1024, max_its > 100000 or refinement_num > 8 is not supported"); return SMPC_ERR_UNSUPPORTED;
  }
  if ((int64_t)in->world_x * in->world_y >= ((int64_t)1 << 31)) { set_error("world_x * world_y must stay below 2^31"); return SMPC_ERR_UNSUPPORTED; }
  if (in->B == 0) return SMPC_OK;
  SMPC_HIP_CHECK(hipSetDevice(h->device));
  smpc::PlanSmootherParams p;
  std::memset(&p, 0, sizeof(p));
  p.B = in->B; p.L = in->L; p.world_x = in->world_x; p.world_y = in->world_y; p.world_shared = in->world_shared ? 1 : 0;
  p.max_its = in->max_its; p.refinement_num = in->refinement_num;
  p.lethal_min = in->lethal_min_cost < 0 ? 0u : (uint32_t)in->lethal_min_cost; p.allow_unknown = in->allow_unknown ? 1u : 0u;
  p.res = in->resolution; p.w_data = in->w_data; p.w_smooth = in->w_smooth; p.tolerance = in->tolerance;
  const size_t B = in->B, L = in->L, nmap = in->world_shared ? 1 : B;
  Staging st(h, in->on_device);
  SMPC_TRY(st.in(p.world, in->world, nmap * (size_t)in->world_x * in->world_y));
  SMPC_TRY(st.in(p.origin, in->world_origin, nmap * 2));
  SMPC_TRY(st.in(p.plan_len, in->plan_len, B));
  SMPC_TRY(st.in(p.range, in->range, B * 2));
  // read and written: the rows the rule leaves alone keep the caller's bytes on the way through device memory too
  SMPC_TRY(st.inout(p.plan, plan, B * L * 2));
  SMPC_TRY(st.out(p.status, status, B));
  SMPC_TRY(st.out(p.info, info, B * 4));
  SMPC_TRY(st.out(p.change, change, B));
  const size_t per_block = smpc::kSmThreads / 64;
  const dim3 grid((unsigned)((B + per_block - 1) / per_block)), block(smpc::kSmThreads);
  SMPC_TRY(st.timed([&] {
    if (in->L <= 64 * smpc::kSmSlotsShort) hipLaunchKernelGGL(smpc::smpc_smooth_plan_kernel<smpc::kSmSlotsShort>, grid, block, 0, h->stream, p);
    else hipLaunchKernelGGL(smpc::smpc_smooth_plan_kernel<smpc::kSmSlotsLong>, grid, block, 0, h->stream, p);
    return SMPC_OK;
  }));
  return st.finish();
}

uint64_t smpc_nearest_workspace_bytes(int32_t A, int32_t grid_x, int32_t grid_y) {
  if (A < 0 || A > SMPC_NEAREST_MAX_ROWS || grid_x < 1 || grid_y < 1 || (int64_t)grid_x * grid_y > SMPC_NEAREST_MAX_BINS) return 0;
  const uint64_t words = 2ull * (uint64_t)grid_x * (uint64_t)grid_y + 1ull + (uint64_t)A;
  return (words * 4ull + 255ull) & ~255ull;
}

int smpc_nearest_people_batch(smpc_handle* h, const smpc_nearest_in* in, double* people, int32_t* count, int32_t* source) {
  if (!h || !in || !people || !count) { set_error("null handle / input / people / count"); return SMPC_ERR_INVALID_ARG; }
  if (!in->robot_pose || (!in->agents && in->A > 0)) { set_error("null robot_pose, or null agents with A > 0"); return SMPC_ERR_INVALID_ARG; }
  if (in->B < 0 || in->A < 0 || in->Np < 1 || in->grid_x < 1 || in->grid_y < 1) { set_error("bad B or A, Np < 1 or a grid side < 1"); return SMPC_ERR_INVALID_ARG; }
  if (!std::isfinite(in->grid_origin[0]) || !std::isfinite(in->grid_origin[1])) { set_error("grid_origin must be finite"); return SMPC_ERR_INVALID_ARG; }
  if (!std::isfinite(in->bin_size) || !(in->bin_size > 0.0)) { set_error("bin_size must be finite and > 0"); return SMPC_ERR_INVALID_ARG; }
  if (!std::isfinite(in->max_range) || !(in->max_range > 0.0)) { set_error("max_range must be finite and > 0"); return SMPC_ERR_INVALID_ARG; }
  {
    const volatile double least = in->max_range * SMPC_NEAREST_BIN_MARGIN;  // the product of the two doubles, rounded once
    if (!(in->bin_size >= least)) { set_error("bin_size must be at least max_range * SMPC_NEAREST_BIN_MARGIN"); return SMPC_ERR_INVALID_ARG; }
  }
  if (in->Np > SMPC_MAX_AGENTS) { set_error("Np > 64 persons is not supported"); return SMPC_ERR_UNSUPPORTED; }
  if ((int64_t)in->grid_x * in->grid_y > SMPC_NEAREST_MAX_BINS) { set_error("more than 65536 bins are not supported"); return SMPC_ERR_UNSUPPORTED; }
  if (in->A > SMPC_NEAREST_MAX_ROWS) { set_error("more than 2^24 agents are not supported"); return SMPC_ERR_UNSUPPORTED; }
  const uint64_t ws_bytes = smpc_nearest_workspace_bytes(in->A, in->grid_x, in->grid_y);
  if (in->on_device && (!in->workspace || in->workspace_bytes < ws_bytes)) { set_error("workspace is null or smaller than smpc_nearest_workspace_bytes()"); return SMPC_ERR_INVALID_ARG; }
  if (in->B == 0) return SMPC_OK;
  SMPC_HIP_CHECK(hipSetDevice(h->device));
  smpc::NearestParams p;
  std::memset(&p, 0, sizeof(p));
  p.B = in->B; p.Np = in->Np; p.A = in->A; p.grid_x = in->grid_x; p.grid_y = in->grid_y;
  p.ox = in->grid_origin[0]; p.oy = in->grid_origin[1]; p.bin_size = in->bin_size; p.max_range = in->max_range;
  const size_t B = in->B, Np = in->Np, A = in->A, G = (size_t)in->grid_x * (size_t)in->grid_y;
  Staging st(h, in->on_device);
  SMPC_TRY(st.in(p.agents, in->agents, A * 5));
  SMPC_TRY(st.in(p.robot_pose, in->robot_pose, B * 3));
  SMPC_TRY(st.in(p.self, in->self, B));
  // read and written: the rows and sources the kernel leaves alone keep the caller's bytes on the way through device memory too
  SMPC_TRY(st.inout(p.people, people, B * Np * 5));
  SMPC_TRY(st.out(p.count, count, B));
  SMPC_TRY(st.inout(p.source, source, B * Np));
  void* ws = in->workspace;
  SMPC_TRY(st.scratch(ws, (size_t)ws_bytes));
  p.offsets = static_cast<int32_t*>(ws);
  p.cursor = p.offsets + G + 1;
  p.rows = p.cursor + G;
  SMPC_TRY(st.timed([&] {
    SMPC_HIP_CHECK(hipMemsetAsync(p.cursor, 0, G * sizeof(int32_t), h->stream));
    const unsigned agent_blocks = (unsigned)((A + smpc::kNnThreads - 1) / smpc::kNnThreads);
    if (A > 0) hipLaunchKernelGGL(smpc::smpc_nearest_count_kernel, dim3(agent_blocks), dim3(smpc::kNnThreads), 0, h->stream, p);
    hipLaunchKernelGGL(smpc::smpc_nearest_scan_kernel, dim3(1), dim3(smpc::kNnScanThreads), 0, h->stream, p);
    if (A > 0) hipLaunchKernelGGL(smpc::smpc_nearest_scatter_kernel, dim3(agent_blocks), dim3(smpc::kNnThreads), 0, h->stream, p);
    const size_t per_block = smpc::kNnThreads / 64;
    hipLaunchKernelGGL(smpc::smpc_nearest_query_kernel, dim3((unsigned)((B + per_block - 1) / per_block)), dim3(smpc::kNnThreads), 0, h->stream, p);
    return SMPC_OK;
  }));
  return st.finish();
}

int smpc_crowd_pool_step_batch(smpc_handle* h, const smpc_crowd_pool_in* in, double* next, int32_t* cursor) {
  if (!h || !in) { set_error("null handle / input"); return SMPC_ERR_INVALID_ARG; }
  if (in->A < 0 || in->M < 0 || in->M > in->A || in->K < 1 || in->grid_x < 1 || in->grid_y < 1) {
    set_error("bad A, M outside 0..A, K < 1 or a grid side < 1"); return SMPC_ERR_INVALID_ARG;
  }
  if (!in->agents && in->A > 0) { set_error("null agents with A > 0"); return SMPC_ERR_INVALID_ARG; }
  if (in->M > 0 && (!next || !cursor || !in->waypoints || !in->n_waypoints)) { set_error("null next / cursor / waypoints / n_waypoints with M > 0"); return SMPC_ERR_INVALID_ARG; }
  if (!std::isfinite(in->grid_origin[0]) || !std::isfinite(in->grid_origin[1])) { set_error("grid_origin must be finite"); return SMPC_ERR_INVALID_ARG; }
  if (!std::isfinite(in->bin_size) || !(in->bin_size > 0.0)) { set_error("bin_size must be finite and > 0"); return SMPC_ERR_INVALID_ARG; }
  if (!std::isfinite(in->interaction_range) || !(in->interaction_range > 0.0)) { set_error("interaction_range must be finite and > 0"); return SMPC_ERR_INVALID_ARG; }
  {
    const volatile double least = in->interaction_range * SMPC_NEAREST_BIN_MARGIN;  // the product of the two doubles, rounded once
    if (!(in->bin_size >= least)) { set_error("bin_size must be at least interaction_range * SMPC_NEAREST_BIN_MARGIN"); return SMPC_ERR_INVALID_ARG; }
  }
  if (!std::isfinite(in->dt) || !(in->dt > 0.0)) { set_error("dt must be finite and > 0"); return SMPC_ERR_INVALID_ARG; }
  if (!(in->goal_radius >= 0.0) || !(in->person_radius >= 0.0) || !(in->desired_speed > 0.0)) {
    set_error("negative radius or non-positive desired_speed"); return SMPC_ERR_INVALID_ARG;
  }
  if (in->od_indexes && (!in->od_origin || in->od_width < 1 || in->od_height < 1 || !(in->od_resolution > 0.0f))) {
    set_error("obstacle grid without origin or with a non-positive size or resolution"); return SMPC_ERR_INVALID_ARG;
  }
  if (in->K > SMPC_MAX_WAYPOINTS) { set_error("K > 8 waypoints is not supported"); return SMPC_ERR_UNSUPPORTED; }
  if ((int64_t)in->grid_x * in->grid_y > SMPC_NEAREST_MAX_BINS) { set_error("more than 65536 bins are not supported"); return SMPC_ERR_UNSUPPORTED; }
  if (in->A > SMPC_NEAREST_MAX_ROWS) { set_error("more than 2^24 agents are not supported"); return SMPC_ERR_UNSUPPORTED; }
  if (in->M > 0) {  // rule 6: the step is synchronous, `next` is no part of the table
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(in->agents), a1 = a0 + (uintptr_t)in->A * 5 * sizeof(double);
    const uintptr_t n0 = reinterpret_cast<uintptr_t>(next), n1 = n0 + (uintptr_t)in->M * 5 * sizeof(double);
    if (n0 < a1 && a0 < n1) { set_error("next overlaps agents"); return SMPC_ERR_INVALID_ARG; }
  }
  const uint64_t ws_bytes = smpc_nearest_workspace_bytes(in->A, in->grid_x, in->grid_y);
  if (in->on_device && (!in->workspace || in->workspace_bytes < ws_bytes)) { set_error("workspace is null or smaller than smpc_nearest_workspace_bytes()"); return SMPC_ERR_INVALID_ARG; }
  if (in->M == 0) return SMPC_OK;
  SMPC_HIP_CHECK(hipSetDevice(h->device));
  smpc::CrowdPoolParams p;
  std::memset(&p, 0, sizeof(p));
  p.M = in->M; p.A = in->A; p.K = in->K; p.cyclic = in->cyclic ? 1 : 0; p.grid_x = in->grid_x; p.grid_y = in->grid_y;
  p.range = in->interaction_range; p.dt = in->dt;
  p.goal_radius = in->goal_radius; p.person_radius = in->person_radius; p.desired_speed = in->desired_speed;
  p.od_width = in->od_width; p.od_height = in->od_height; p.od_resolution = in->od_resolution;
  smpc::fill_math_table(&p.mt);
  smpc::NearestParams b;  // the gather's binning kernels, on the same table and workspace
  std::memset(&b, 0, sizeof(b));
  b.A = in->A; b.grid_x = in->grid_x; b.grid_y = in->grid_y;
  b.ox = in->grid_origin[0]; b.oy = in->grid_origin[1]; b.bin_size = in->bin_size;
  const size_t M = in->M, A = in->A, K = in->K, G = (size_t)in->grid_x * (size_t)in->grid_y;
  const bool grid = in->od_indexes != nullptr;
  Staging st(h, in->on_device);
  SMPC_TRY(st.in(p.agents, in->agents, A * 5));
  SMPC_TRY(st.in(p.waypoints, in->waypoints, M * K * 2));
  SMPC_TRY(st.in(p.n_waypoints, in->n_waypoints, M));
  SMPC_TRY(st.in(p.desired_speeds, in->desired_speeds, M));
  SMPC_TRY(st.in(p.od_indexes, in->od_indexes, grid ? (size_t)in->od_width * in->od_height : 0));
  SMPC_TRY(st.in(p.od_origin, grid ? in->od_origin : nullptr, 2));
  SMPC_TRY(st.out(p.next, next, M * 5));
  // read and written: the cursor of an inert mover keeps the caller's value on the way through device memory too
  SMPC_TRY(st.inout(p.cursor, cursor, M));
  void* ws = in->workspace;
  SMPC_TRY(st.scratch(ws, (size_t)ws_bytes));
  b.agents = p.agents;
  b.offsets = static_cast<int32_t*>(ws);
  b.cursor = b.offsets + G + 1;
  b.rows = b.cursor + G;
  p.offsets = b.offsets; p.rows = b.rows;
  const bool bins_ready = in->on_device && in->bins_ready;
  SMPC_TRY(st.timed([&] {
    if (!bins_ready) {
      SMPC_HIP_CHECK(hipMemsetAsync(b.cursor, 0, G * sizeof(int32_t), h->stream));
      const unsigned agent_blocks = (unsigned)((A + smpc::kNnThreads - 1) / smpc::kNnThreads);
      hipLaunchKernelGGL(smpc::smpc_nearest_count_kernel, dim3(agent_blocks), dim3(smpc::kNnThreads), 0, h->stream, b);
      hipLaunchKernelGGL(smpc::smpc_nearest_scan_kernel, dim3(1), dim3(smpc::kNnScanThreads), 0, h->stream, b);
      hipLaunchKernelGGL(smpc::smpc_nearest_scatter_kernel, dim3(agent_blocks), dim3(smpc::kNnThreads), 0, h->stream, b);
    }
    // one block column per bin, then the blocks that copy the movers that are in no bin
    const unsigned columns = (unsigned)(G + (M + smpc::kCpThreads - 1) / smpc::kCpThreads);
    hipLaunchKernelGGL(smpc::smpc_crowd_pool_step_kernel, dim3(columns, smpc::kCpSplit), dim3(smpc::kCpThreads), 0, h->stream, p);
    return SMPC_OK;
  }));
  return st.finish();
}

int smpc_stage_people_batch(smpc_handle* h, const smpc_scene_batch* sb, double* records, double* aux) {
  if (!h || !sb || !records || !aux) { set_error("null handle / scene batch / output"); return SMPC_ERR_INVALID_ARG; }
  if (sb->B < 0 || sb->T < 1 || sb->N < 1) { set_error("bad B/T/N"); return SMPC_ERR_INVALID_ARG; }
  if (sb->T + 1 > smpc::kWave || sb->N > smpc::kWave) { set_error("T + 1 > 64 or N > 64 is not supported"); return SMPC_ERR_UNSUPPORTED; }
  if (!sb->pose0 || !sb->people) { set_error("null input array"); return SMPC_ERR_INVALID_ARG; }
  SMPC_HIP_CHECK(hipSetDevice(h->device));
  smpc::KParams k;
  std::memset(&k, 0, sizeof(k));
  k.B = sb->B; k.T = sb->T; k.N = sb->N;
  smpc::fill_math_table(&k.mt);
  const size_t B = sb->B, T = sb->T, N = sb->N;
  const size_t nrec = B * N * T * 4, naux = B * T * 2;
  Staging st(h, sb->on_device);
  double *drec = nullptr, *daux = nullptr;
  SMPC_TRY(st.in(k.pose0, sb->pose0, B * 3));
  SMPC_TRY(st.in(k.people, sb->people, B * (T + 1) * 6 * N));
  SMPC_TRY(st.in(k.has_people, sb->has_people, B));
  SMPC_TRY(st.out(drec, records, nrec));
  SMPC_TRY(st.out(daux, aux, naux));
  if (!sb->on_device) {  // scenes without people: defined bytes
    SMPC_HIP_CHECK(hipMemsetAsync(drec, 0, nrec * sizeof(double), h->stream));
    SMPC_HIP_CHECK(hipMemsetAsync(daux, 0, naux * sizeof(double), h->stream));
  }
  SMPC_TRY(st.timed([&] { return launch_stage(h, k, drec, daux); }));
  return st.finish();
}

double smpc_fp64_peak_probe(smpc_handle* h, int32_t iters) {
  if (!h || iters < 1) { set_error("bad arguments to smpc_fp64_peak_probe"); return -1.0; }
  if (hipSetDevice(h->device) != hipSuccess) return -1.0;
  const int blocks = h->num_cu * 8, threads = 256;   // 8 waves per SIMD
  double* out = nullptr;
  if (hipMalloc(reinterpret_cast<void**>(&out), (size_t)blocks * threads * sizeof(double)) != hipSuccess) return -1.0;
  double best = -1.0;
  for (int rep = 0; rep < 3; ++rep) {
    (void)hipEventRecord(h->ev0, h->stream);
    hipLaunchKernelGGL(smpc::smpc_fp64_peak_kernel, dim3(blocks), dim3(threads), 0, h->stream, out, iters);
    (void)hipEventRecord(h->ev1, h->stream);
    if (hipEventSynchronize(h->ev1) != hipSuccess) break;
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, h->ev0, h->ev1) != hipSuccess || ms <= 0.f) break;
    const double flop = 2.0 * 64.0 * (double)iters * (double)blocks * (double)threads;
    const double tf = flop / (ms * 1e-3) / 1e12;
    if (tf > best) best = tf;
  }
  (void)hipFree(out);
  return best;
}

int smpc_math_probe(smpc_handle* h, int32_t fn, int32_t n, const double* a, const double* b, double* out0, double* out1) {
  if (!h || !a || !out0 || n < 0 || fn < 0 || fn > 8) { set_error("bad arguments to smpc_math_probe"); return SMPC_ERR_INVALID_ARG; }
  if ((fn == 1 || fn == 4 || fn == 8) && !b) { set_error("second argument array is null"); return SMPC_ERR_INVALID_ARG; }
  if (fn == 2 && !out1) { set_error("out1 is null for sincos"); return SMPC_ERR_INVALID_ARG; }
  SMPC_HIP_CHECK(hipSetDevice(h->device));
  smpc::ProbeParams p;
  std::memset(&p, 0, sizeof(p));
  p.fn = fn; p.n = n;
  smpc::fill_math_table(&p.mt);
  smpc::fill_atan_nodes(&p.an);
  Staging st(h, false);  // host arrays only
  SMPC_TRY(st.in(p.a, a, (size_t)n * (fn == 7 ? 8 : 1)));
  SMPC_TRY(st.in(p.b, b, (size_t)n));
  SMPC_TRY(st.out(p.o0, out0, (size_t)n));
  SMPC_TRY(st.out(p.o1, out1, (size_t)n));
  if (n > 0) {  // a diagnostic: not timed
    SMPC_TRY(st.flush_up());
    hipLaunchKernelGGL(smpc::smpc_math_probe_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, p);
    SMPC_HIP_CHECK(hipGetLastError());
  }
  return st.finish();
}

int smpc_eval_batch(smpc_handle* h, const smpc_scene_batch* sb, const double* params, smpc_eval_batch_out* out) {
  const char* bad = nullptr;
  if (!out || !params) bad = "null params / output";
  else if (out->row_order != 0 && out->row_order != 1) bad = "row_order must be 0 or 1";
  return sweep_call(h, sb, Sweep::Eval, bad, [&](const Dims& d, smpc::KParams& k, Staging& st) -> int {
    const size_t B = sb->B;
    k.e_row_order = out->row_order;
    SMPC_TRY(st.in(k.e_x, params, B * d.P));
    SMPC_TRY(st.out(k.e_residuals, out->residuals, B * d.M));
    SMPC_TRY(st.out(k.e_jacobian, out->jacobian, B * d.M * d.P));
    SMPC_TRY(st.out(k.e_cost, out->cost, B));
    return st.out(k.e_gradient, out->gradient, B * d.P);
  });
}

}  // extern "C"
