// smpc_hip.hip — kernels + the C ABI of include/smpc.h (libsmpc_hip.so). gfx950 only, no CPU fallback.
//
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
//   and the kernels of the tick around the solve, one header each (projection, distance, format, trajectorize, window).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/smpc_fixed_shapes.h"
#include "smpc_eval_kernel.hpp"
#include "smpc_launch.hpp"
#include "smpc_lm.hpp"
#include "smpc_solve_kernel.hpp"
#include "smpc_stage_kernel.hpp"
#include "smpc_project.hpp"
#include "smpc_distance.hpp"
#include "smpc_format.hpp"
#include "smpc_trajectorize.hpp"
#include "smpc_path_window.hpp"
#include "smpc_metrics.hpp"
#include "smpc_crowd.hpp"

// ================================================================================================
// Host side of the C ABI
// ================================================================================================
namespace {

thread_local std::string g_last_error;

void set_error(const std::string& s) { g_last_error = s; }

#define SMPC_HIP_CHECK(expr)                                                                   \
  do {                                                                                         \
    hipError_t _e = (expr);                                                                    \
    if (_e != hipSuccess) {                                                                    \
      set_error(std::string(#expr) + ": " + hipGetErrorString(_e));                            \
      return SMPC_ERR_DEVICE;                                                                  \
    }                                                                                          \
  } while (0)

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

}  // namespace

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

namespace smpc {
// n rows of smpc_scene_params, all equal to `row` (neutral_rows(), below)
__global__ void smpc_fill_scene_params_kernel(smpc_scene_params* rows, int n, const smpc_scene_params row) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) rows[i] = row;
}
}  // namespace smpc

struct smpc_handle {
  smpc_params prm{};
  int device = 0;
  int num_cu = 0;
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  bool timed = false;
  int* queue = nullptr;  // device-side scene queue head
  int share = 1;         // smpc_set_solve_share: concurrent solve launches the persistent grid leaves room for
  bool fixed_shapes = true;  // smpc_set_fixed_shapes: launches of a shape of SMPC_FIXED_SHAPES run that shape's kernels
  double* stage_rec = nullptr;  // staged people block of the latest call that did not bring its own (grow-only)
  double* stage_aux = nullptr;
  size_t stage_rec_bytes = 0, stage_aux_bytes = 0;
  char* stage = nullptr;  // grow-only arena for host-pointer calls (the plugin's B = 1 use): no hipMalloc per call
  size_t stage_cap = 0;
  size_t stage_want = 0;  // high-water mark of the calls so far
  double* neutral_sp = nullptr;  // smpc_solve_trace_batch on a batch without scene_params: the handle's own values as rows
  size_t neutral_sp_bytes = 0;   // (grow-only; prm never changes, so rows once written stay valid)
  char* pin = nullptr;    // page-locked host mirror of the arena's first pin_cap bytes: the small arrays of a host-pointer call
  size_t pin_cap = 0;     // travel in ONE copy each way instead of one pageable hipMemcpy per array (Staging, below)
};

namespace {

using KernelFn = void (*)(const smpc::KParams);

// vt: the batch carries a horizon per scene (smpc_scene_batch.T_scene): the instantiation that reads T, CH, bl of each
// scene from LDS instead of taking them as launch constants. sp: the batch carries weights and bounds per scene
// (smpc_scene_batch.scene_params): kSP, which reads the horizon per scene as well (T_scene or T).
// Sweep::Trace (smpc_solve_trace_batch): the solve that also leaves a row per LM iteration, compiled for the most general
// variant only, kVT = kSP = true. A batch without T_scene runs it as it is (the kernel takes T for every scene), one
// without scene_params with the handle's own weights and bounds as every scene's row (neutral_rows()): both give the
// plain kernels' results bit for bit.
enum class Sweep { Eval, Solve, Trace };

template <int NB, int W, bool kVT, bool kSP> KernelFn pick_fn(Sweep kind) {
  return kind == Sweep::Eval ? smpc::smpc_eval_kernel<NB, W, kVT, kSP> : smpc::smpc_solve_kernel<NB, W, kVT, kSP>;
}

template <int NB> KernelFn pick_w(int W, Sweep kind, bool vt, bool sp) {
  if (kind == Sweep::Trace) return W == 32 ? smpc::smpc_solve_kernel<NB, 32, true, true, true> : smpc::smpc_solve_kernel<NB, 64, true, true, true>;
  if (W == 32) return sp ? pick_fn<NB, 32, true, true>(kind) : vt ? pick_fn<NB, 32, true, false>(kind) : pick_fn<NB, 32, false, false>(kind);
  return sp ? pick_fn<NB, 64, true, true>(kind) : vt ? pick_fn<NB, 64, true, false>(kind) : pick_fn<NB, 64, false, false>(kind);
}

KernelFn pick(int nb, int W, Sweep kind, bool vt = false, bool sp = false) {
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

// The kernels of a shape of SMPC_FIXED_SHAPES (smpc_launch.hpp): T, N, CH, bl as literals instead of launch values, the
// same results bit for bit. They stand in for the plain instantiation <NB, W, false, false> only: a launch with a horizon
// or parameters per scene, a trace, or the other slot width (the one-scene-per-wave kernel of a small batch) runs the
// run-time-shape kernel it always ran.
// *stages (if given): whether the kernel returned can stage the people block itself at the scene fetch (the solve kernel
// of a Shape with kStageAtFetch; K1 never does)
template <class Shape> KernelFn fixed_fn(Sweep kind, int W, bool* stages) {
#ifdef SMPC_ONLY_NB
  if constexpr (Shape::kNB != SMPC_ONLY_NB) return nullptr; else
#endif
  if (W != Shape::kW) return nullptr;
  if (stages) *stages = kind == Sweep::Solve && Shape::kStageAtFetch;
  return kind == Sweep::Eval ? smpc::smpc_eval_fixed_kernel<Shape> : smpc::smpc_solve_fixed_kernel<Shape>;
}

KernelFn pick_fixed(const smpc::KParams& k, int W, Sweep kind, bool vt, bool sp, bool* stages = nullptr) {
  if (stages) *stages = false;
  if (kind == Sweep::Trace || vt || sp) return nullptr;
  const int want = smpc::fixed_shape_index(k.T, k.N, k.CH, k.bl);  // the rule; below only the index -> kernel table
  int i = 0;
#define SMPC_X(t, n, ch, b) \
  if (want == i++) return fixed_fn<smpc::FixedShape<t, n, ch, b>>(kind, W, stages);
  SMPC_FIXED_SHAPES(SMPC_X)
#undef SMPC_X
  return nullptr;
}

// Whether this handle's launches may take a fixed-shape kernel at all: smpc_set_fixed_shapes, and not under the experiment
// knob SMPC_NO_HELPERS, which works through the launch value k.hp_A that a fixed shape folds in.
bool fixed_shapes_on(const smpc_handle* h) { return h->fixed_shapes && !std::getenv("SMPC_NO_HELPERS"); }

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
  if (!pick(d->nb, 64, Sweep::Solve)) { set_error("more than SMPC_MAX_BLOCKS parameter blocks (nb must be 1..10)"); return SMPC_ERR_UNSUPPORTED; }
  return SMPC_OK;
}

void fill_kparams(const smpc_handle* h, const smpc_scene_batch* sb, const Dims& d, smpc::KParams* k) {
  std::memset(k, 0, sizeof(*k));
  k->B = sb->B; k->T = sb->T; k->N = sb->N;
  k->CH = d.CH; k->bl = d.bl; k->nb = d.nb; k->P = d.P; k->nbounded = d.nbounded; k->nfeas = d.nfeas;
  k->size_x = sb->size_x; k->size_y = sb->size_y; k->costmap_shared = sb->costmap_shared;
  k->dt = sb->dt; k->resolution = sb->resolution; k->inv_resolution = 1.0 / sb->resolution;
  k->prm = h->prm;
  k->e_M = d.M;
  k->hp_A = sb->N;  // set by launch() once the slot width is chosen
  smpc::fill_math_table(&k->mt);
  smpc::fill_atan_nodes(&k->an);
}

#define SMPC_TRY(expr) do { int _rc = (expr); if (_rc != SMPC_OK) return _rc; } while (0)

// Every batch entry point takes host or device pointers (on_device) and names each of its arrays once, here: in(), out()
// or inout(), with the kernel parameter to fill, the caller's pointer and the element count. Device pointers are passed
// through. Host arrays are staged through device memory: sub-allocations of the handle's arena, which grows to the
// high-water mark at the start of the next call (every host-pointer call ends with a stream synchronise, so nothing is
// in flight then); what does not fit meanwhile comes from hipMalloc and is freed when the call returns.
// The plugin's own call (B = 1: a dozen arrays of a few hundred bytes and one costmap) used to spend more time in its 16
// pageable hipMemcpy calls than in its kernels. The head of the arena (kPinBytes) therefore has a page-locked mirror on
// the host: inputs that land there are gathered in the mirror and cross in ONE asynchronous copy (flush_up(), before the
// first kernel of the call), outputs that land there come back in one copy and are handed out from the mirror
// (finish()). What lies beyond the mirror (large batches) is copied array by array.
constexpr size_t kPinBytes = 8u << 20;
class Staging {
 public:
  Staging(smpc_handle* handle, bool on_device) : h(handle), host(!on_device) {
    if (h->stage_want > h->stage_cap) {
      if (h->stage) (void)hipFree(h->stage);
      h->stage = nullptr; h->stage_cap = 0;
      const size_t cap = h->stage_want + h->stage_want / 4;
      void* p = nullptr;
      if (hipMalloc(&p, cap) == hipSuccess) { h->stage = static_cast<char*>(p); h->stage_cap = cap; }
    }
    if (h->stage) {
      const size_t want = h->stage_cap < kPinBytes ? h->stage_cap : kPinBytes;
      if (h->pin_cap < want) {
        if (h->pin) (void)hipHostFree(h->pin);
        h->pin = nullptr; h->pin_cap = 0;
        void* p = nullptr;
        if (hipHostMalloc(&p, want, hipHostMallocDefault) == hipSuccess) { h->pin = static_cast<char*>(p); h->pin_cap = want; }
      }
    }
  }
  ~Staging() {
    for (void* p : overflow) (void)hipFree(p);
    if (need > h->stage_want) h->stage_want = need;
  }
  // n elements the kernel reads / writes / reads and updates in place
  template <typename T> int in(const T*& dev, const T* src, size_t n) { return bind(dev, src, src, nullptr, n * sizeof(T)); }
  template <typename T> int out(T*& dev, T* dst, size_t n) { return bind(dev, dst, nullptr, dst, n * sizeof(T)); }
  template <typename T> int inout(T*& dev, T* buf, size_t n) { return bind(dev, buf, buf, buf, n * sizeof(T)); }
  // the gathered inputs cross here (timed() does it before the kernels)
  int flush_up() {
    if (up_hi > up_lo) SMPC_HIP_CHECK(hipMemcpyAsync(h->stage + up_lo, h->pin + up_lo, up_hi - up_lo, hipMemcpyHostToDevice, h->stream));
    up_lo = SIZE_MAX; up_hi = 0;
    return SMPC_OK;
  }
  // The kernels of a call, between the events smpc_last_kernel_ms() reads: the inputs have crossed before ev0, so the
  // time is the kernels' alone. `kernels` launches them on h->stream and returns SMPC_OK or an error code.
  template <typename F> int timed(F&& kernels) {
    SMPC_TRY(flush_up());
    SMPC_HIP_CHECK(hipEventRecord(h->ev0, h->stream));
    SMPC_TRY(kernels());
    SMPC_HIP_CHECK(hipGetLastError());
    SMPC_HIP_CHECK(hipEventRecord(h->ev1, h->stream));
    h->timed = true;
    return SMPC_OK;
  }
  // End of the call. Host pointers: the outputs come back (those in the mirror in one copy), the stream is drained and
  // the results are handed out. Device pointers: nothing to do, the call stays asynchronous.
  int finish() {
    if (!host) return SMPC_OK;
    SMPC_TRY(flush_up());  // a call that launched nothing (empty batch)
    size_t lo = SIZE_MAX, hi = 0;
    for (const Back& b : backs) {
      if (b.off == SIZE_MAX) { SMPC_HIP_CHECK(hipMemcpyAsync(b.host, b.dev, b.bytes, hipMemcpyDeviceToHost, h->stream)); continue; }
      if (b.off < lo) lo = b.off;
      if (b.off + b.bytes > hi) hi = b.off + b.bytes;
    }
    if (hi > lo) SMPC_HIP_CHECK(hipMemcpyAsync(h->pin + lo, h->stage + lo, hi - lo, hipMemcpyDeviceToHost, h->stream));
    SMPC_HIP_CHECK(hipStreamSynchronize(h->stream));
    for (const Back& b : backs)
      if (b.off != SIZE_MAX) std::memcpy(b.host, h->pin + b.off, b.bytes);
    return SMPC_OK;
  }

 private:
  struct Back { void* host; const void* dev; size_t off, bytes; };  // off: in the mirror, or SIZE_MAX
  smpc_handle* h;
  bool host;
  size_t off = 0, need = 0;
  size_t up_lo = SIZE_MAX, up_hi = 0;  // arena bytes [up_lo, up_hi) wait in the mirror for flush_up()
  std::vector<Back> backs;             // outputs, fetched by finish()
  std::vector<void*> overflow;
  int take(size_t bytes, void** out) {
    const size_t sz = (bytes + 255) & ~(size_t)255;
    need += sz;
    if (h->stage && off + sz <= h->stage_cap) { *out = h->stage + off; off += sz; return SMPC_OK; }
    void* p = nullptr;
    SMPC_HIP_CHECK(hipMalloc(&p, sz));
    overflow.push_back(p);
    *out = p;
    return SMPC_OK;
  }
  // offset of a device pointer inside the mirrored head of the arena, or SIZE_MAX
  size_t mirrored(const void* dev, size_t bytes) const {
    if (!h->stage || !h->pin) return SIZE_MAX;
    const char* p = static_cast<const char*>(dev);
    if (p < h->stage || p + bytes > h->stage + h->pin_cap) return SIZE_MAX;
    return (size_t)(p - h->stage);
  }
  template <typename P> int bind(P& dev, P caller, const void* up, void* back, size_t bytes) {
    if (!host) { dev = caller; return SMPC_OK; }
    void* p = nullptr;
    SMPC_TRY(stage(up, back, bytes, &p));
    dev = static_cast<P>(p);
    return SMPC_OK;
  }
  // Device room for a host array of `bytes`: `up` (if any) gathered in the mirror or copied now, `back` (if any) the
  // host array finish() copies the result to. A null array or an empty one binds a null device pointer.
  int stage(const void* up, void* back, size_t bytes, void** dev) {
    *dev = nullptr;
    if ((!up && !back) || bytes == 0) return SMPC_OK;
    SMPC_TRY(take(bytes, dev));
    const size_t o = mirrored(*dev, bytes);
    if (up && o != SIZE_MAX) {
      std::memcpy(h->pin + o, up, bytes);
      if (o < up_lo) up_lo = o;
      if (o + bytes > up_hi) up_hi = o + bytes;
    } else if (up) {
      SMPC_HIP_CHECK(hipMemcpyAsync(*dev, up, bytes, hipMemcpyHostToDevice, h->stream));
    }
    if (back) backs.push_back({back, *dev, o, bytes});
    return SMPC_OK;
  }
};

int grow(double** buf, size_t* have, size_t need, hipStream_t st) {
  if (need <= *have) return SMPC_OK;
  SMPC_HIP_CHECK(hipStreamSynchronize(st));  // nothing of an earlier call may still read the old buffer
  if (*buf) SMPC_HIP_CHECK(hipFree(*buf));
  *buf = nullptr; *have = 0;
  SMPC_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(buf), need));
  *have = need;
  return SMPC_OK;
}

// The staging pass: k.people (+ pose0, has_people) -> records / aux at the given device pointers.
int launch_stage(smpc_handle* h, smpc::KParams& k, double* rec, double* aux) {
  if (k.B == 0 || k.N == 0) return SMPC_OK;
  const int W = smpc::slot_width(k.T, k.N);
  const int S = smpc::kWave / W;
  const smpc::LdsLayout L = smpc::make_layout(k.T, k.N, 2, smpc::kLayoutStage, W);
  const size_t shmem = (size_t)S * L.total * sizeof(double);
  KernelFn fn = (W == 32) ? smpc::smpc_stage_kernel<32> : smpc::smpc_stage_kernel<64>;
  if (shmem > 160 * 1024) { set_error("people block does not fit the 160 KiB LDS of one CU"); return SMPC_ERR_UNSUPPORTED; }
  if (shmem > 64 * 1024) SMPC_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem));
  k.stage_rec = rec; k.stage_aux = aux;
  hipLaunchKernelGGL(fn, dim3((k.B + S - 1) / S), dim3(smpc::kWave), shmem, h->stream, k);
  SMPC_HIP_CHECK(hipGetLastError());
  return SMPC_OK;
}

// Waves per CU a solve launch takes when it is sized for having the GPU to itself (launch(), below).
int lone_waves_per_cu() {
  int lone_per_cu = 8;
  if (const char* v = std::getenv("SMPC_LONE_WAVES_PER_CU")) { const int c = std::atoi(v); if (c >= 1) lone_per_cu = c; }  // experiment knob
  return lone_per_cu;
}

// Slot width of a solve launch. A shape that fits two scenes per wave (W = 32) still runs ONE scene per wave while the
// batch is small: up to one scene per SIMD (4 x CUs), two scenes in the lockstep of one wave only make each other wait
// (their LM phases differ from trip to trip; measured 4-17 % slower than a wave each, with bit-identical results); and
// where the W = 64 kernel's helper lanes pay (helper_owner_agents(): the 64 - T lanes beyond the horizon take over half
// of every step's agent list), up to the number of waves a lone launch takes anyway (8 per CU): every sweep of every
// scene is shorter then — the plugin's own call (B = 1, 8 people) 1.24 -> 1.06 ms, 1024 scenes 1.60 -> 1.13 ms, equal at
// 2048 (tools/gpu_width.py). Decided by the shape of the batch alone (B, T, N, the handle's share): a scene's result
// never depends on timing. With helper lanes it differs from the W = 32 kernel's in the last bits (the order of the
// sums over the agents).
int solve_slot_width(const smpc_handle* h, const smpc::KParams& k) {
  const int W = smpc::slot_width(k.T, k.N);
  if (W == 64) return 64;
  if (const char* v = std::getenv("SMPC_SOLVE_WIDTH")) { const int c = std::atoi(v); if (c == 32 || c == 64) return c; }  // experiment knob
  const int share = h->share > 1 ? h->share : 1;
  const bool helpers_pay = smpc::helper_owner_agents(k.T, k.N, 64) < k.N;
  const int per_cu = helpers_pay ? lone_waves_per_cu() : 4;
  return (k.B <= per_cu * h->num_cu / share) ? 64 : 32;
}

// The kernel a launch runs: its slot width, the function, and whether that kernel stages the people block itself.
struct Picked { int W; KernelFn fn; bool stages; };
Picked pick_launch(const smpc_handle* h, const smpc::KParams& k, Sweep kind) {
  Picked p;
  p.W = kind == Sweep::Eval ? smpc::slot_width(k.T, k.N) : solve_slot_width(h, k);
  p.stages = false;
  const bool sp = k.scene_params != nullptr;
  p.fn = fixed_shapes_on(h) ? pick_fixed(k, p.W, kind, k.T_scene != nullptr, sp, &p.stages) : nullptr;
  if (!p.fn) p.fn = pick(k.nb, p.W, kind, k.T_scene != nullptr, sp);
  return p;
}

// Makes the people block of a launch of `kind` readable by its kernel: the caller's staged block; or, where the kernel
// picked for the launch stages each scene as it fetches it (pick_launch().stages: the fixed-shape solve kernel), room for
// the records and k.stage_at_fetch — no staging kernel, no aux array, and smpc_last_kernel_ms() then covers the staging;
// or the library's own staging pass into the handle's buffers (timed separately: smpc_last_kernel_ms() reports the
// solve / sweep kernel alone).
int bind_people(smpc_handle* h, const smpc_scene_batch* sb, smpc::KParams& k, Staging* st, Sweep kind) {
  if (sb->N == 0) return SMPC_OK;
  const size_t nrec = (size_t)sb->B * sb->N * sb->T * 4, naux = (size_t)sb->B * sb->T * 2;
  if (sb->people_records) {
    SMPC_TRY(st->in(k.people_rec, sb->people_records, nrec));
    return st->in(k.people_aux, sb->people_aux, naux);
  }
  SMPC_TRY(grow(&h->stage_rec, &h->stage_rec_bytes, nrec * sizeof(double), h->stream));
  if (pick_launch(h, k, kind).stages) {
    k.stage_at_fetch = 1;  // (its own field: launch_stage() sets stage_rec for the staging kernel on this very struct)
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

// Sweep::Trace: the solve kernel that also writes k.o_trace / k.o_trace_n (k.scene_params is set by then)
int launch(smpc_handle* h, Staging& st, Sweep kind, smpc::KParams& k) {
  const bool eval = kind == Sweep::Eval;
  const Picked picked = pick_launch(h, k, kind);
  const int W = picked.W;
  const int S = smpc::kWave / W;
  const bool sp = k.scene_params != nullptr;
  KernelFn fn = picked.fn;
  if (k.stage_at_fetch && !picked.stages) { set_error("internal: a launch without staged people on a kernel that stages none"); return SMPC_ERR_UNSUPPORTED; }
  const smpc::LdsLayout L = smpc::make_layout(k.T, k.N, k.P, eval ? smpc::kLayoutEval : smpc::kLayoutSolve, W, sp);
  k.hp_A = smpc::helper_owner_agents(k.T, k.N, W);
  if (std::getenv("SMPC_NO_HELPERS")) k.hp_A = k.N;  // experiment knob (the LDS layout keeps the helper regions)
  // behind the slot blocks: the feasibility rows of every slot (solve) or the row staging blocks + parked sensitivities (K1)
  const size_t extra = eval ? (size_t)smpc::eval_extra_doubles(k.T, k.P, W) : (size_t)smpc::wave_extra_doubles(k.P, W);
  // ... and behind those the wave's copy of the arctangent's node table
  const size_t shmem = ((size_t)smpc::atan_tab_offset(S * L.total, (int)extra) + smpc::kAtanTabDoubles) * sizeof(double);
  if (shmem > 160 * 1024) { set_error("scene does not fit the 160 KiB LDS of one CU"); return SMPC_ERR_UNSUPPORTED; }
  if (shmem > 64 * 1024) SMPC_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem));
  if (k.B == 0) return SMPC_OK;
  int grid = (k.B + S - 1) / S;
  if (!eval) {
    // persistent sweep engine: no more waves than can be resident; scenes come from the queue
    int per_cu = 0;
    SMPC_HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, reinterpret_cast<const void*>(fn), smpc::kWave, shmem));
    if (h->share > 1) per_cu /= h->share;  // room for the other launches of smpc_set_solve_share
    if (per_cu < 1) per_cu = 1;
    if (const char* cap = std::getenv("SMPC_MAX_WAVES_PER_CU")) {  // experiment knob: limit resident waves per CU
      const int c = std::atoi(cap);
      if (c >= 1 && c < per_cu) per_cu = c;
    }
    if (std::getenv("SMPC_DEBUG_GRID")) std::fprintf(stderr, "[smpc] solve kernel: %zu B LDS per wave, %d waves per CU\n", shmem, per_cu);
    const int resident = per_cu * h->num_cu;
    // A launch alone on the GPU finishes soonest with two waves per SIMD (two scenes per slot at the headline batch:
    // a third wave per SIMD lengthens every trip more than it shortens the queue, and the tail of long scenes grows);
    // the third wave's registers and LDS then stay free for the launches of other streams, which is where the extra
    // occupancy pays. Only a batch with many scenes per slot takes every resident wave for itself.
    const int lone_per_cu = lone_waves_per_cu();
    const int two_per_simd = lone_per_cu * h->num_cu < resident ? lone_per_cu * h->num_cu : resident;
    if (grid > two_per_simd) grid = (grid >= 4 * resident) ? resident : two_per_simd;
    k.queue = h->queue;
    k.full_gram = std::getenv("SMPC_FULL_GRAM") ? 1 : 0;  // experiment / test knob
    k.prio_step = 0;
    if (const char* v = std::getenv("SMPC_PRIO_STEP")) { const int c = std::atoi(v); if (c >= 1) k.prio_step = c; }  // experiment knob
    SMPC_HIP_CHECK(hipMemsetAsync(h->queue, 0, sizeof(int), h->stream));
  }
#ifdef SMPC_STAMPS
  {  // diagnostic build: per-wave phase cycle sums, dumped to stderr after the launch
    static unsigned long long* d_stamps = nullptr; static int cap = 0;
    if (grid > cap) { if (d_stamps) (void)hipFree(d_stamps); SMPC_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&d_stamps), (size_t)grid * 12 * sizeof(unsigned long long))); cap = grid; }
    k.stamps = d_stamps;
  }
#endif
  SMPC_TRY(st.timed([&] { hipLaunchKernelGGL(fn, dim3(grid), dim3(smpc::kWave), shmem, h->stream, k); return SMPC_OK; }));
#ifdef SMPC_STAMPS
  {
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
  }
#endif
  return SMPC_OK;
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

}  // namespace

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
  if (hipMalloc(reinterpret_cast<void**>(&h->queue), sizeof(int)) != hipSuccess) { set_error("hipMalloc(queue) failed"); delete h; return nullptr; }
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

int smpc_solve_slot_width(const smpc_handle* h, int32_t B, int32_t T, int32_t N) {
  if (!h || B < 0 || T < 1 || N < 0) { set_error("null handle or bad B/T/N"); return SMPC_ERR_INVALID_ARG; }
  if (T + 1 > smpc::kWave || N > smpc::kWave) { set_error("T + 1 > 64 rollout poses or N > 64 agents"); return SMPC_ERR_UNSUPPORTED; }
  smpc::KParams k;
  k.B = B; k.T = T; k.N = N;
  return solve_slot_width(h, k);
}

int smpc_set_fixed_shapes(smpc_handle* h, int32_t enable) {
  if (!h) { set_error("null handle"); return SMPC_ERR_INVALID_ARG; }
  h->fixed_shapes = enable != 0;
  return SMPC_OK;
}

int smpc_solve_shape_is_fixed(const smpc_handle* h, int32_t B, int32_t T, int32_t N) {
  const int W = smpc_solve_slot_width(h, B, T, N);
  if (W < 0) return W;
  if (h->prm.control_horizon < 1 || h->prm.parameter_block_length < 1) { set_error("control_horizon and parameter_block_length must be >= 1"); return SMPC_ERR_INVALID_ARG; }
  const Dims d = make_dims(h->prm, T, true);
  smpc::KParams k;
  k.T = T; k.N = N; k.CH = d.CH; k.bl = d.bl;
  return (fixed_shapes_on(h) && pick_fixed(k, W, Sweep::Solve, false, false)) ? 1 : 0;
}

int smpc_eval_shape_is_fixed(const smpc_handle* h, int32_t T, int32_t N) {
  if (!h || T < 1 || N < 0) { set_error("null handle or bad T/N"); return SMPC_ERR_INVALID_ARG; }
  if (T + 1 > smpc::kWave || N > smpc::kWave) { set_error("T + 1 > 64 rollout poses or N > 64 agents"); return SMPC_ERR_UNSUPPORTED; }
  if (h->prm.control_horizon < 1 || h->prm.parameter_block_length < 1) { set_error("control_horizon and parameter_block_length must be >= 1"); return SMPC_ERR_INVALID_ARG; }
  const Dims d = make_dims(h->prm, T, true);
  smpc::KParams k;
  k.T = T; k.N = N; k.CH = d.CH; k.bl = d.bl;
  return (fixed_shapes_on(h) && pick_fixed(k, smpc::slot_width(T, N), Sweep::Eval, false, false)) ? 1 : 0;
}

}  // extern "C"

namespace {

// smpc_solve_batch (trace == nullptr) and smpc_solve_trace_batch
int solve_batch(smpc_handle* h, const smpc_scene_batch* sb, smpc_result_batch* out, const smpc_trace_out* trace) {
  Dims d;
  SMPC_TRY(validate(h, sb, &d));
  if (!out) { set_error("null result batch"); return SMPC_ERR_INVALID_ARG; }
  SMPC_HIP_CHECK(hipSetDevice(h->device));
  smpc::KParams k;
  fill_kparams(h, sb, d, &k);
  Staging st(h, sb->on_device);
  SMPC_TRY(bind_inputs(sb, d, &k, &st));
  SMPC_TRY(bind_people(h, sb, k, &st, trace ? Sweep::Trace : Sweep::Solve));
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
  SMPC_TRY(launch(h, st, trace ? Sweep::Trace : Sweep::Solve, k));
  return st.finish();
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
  Dims d;
  SMPC_TRY(validate(h, sb, &d));
  if (!out || !params) { set_error("null params / output"); return SMPC_ERR_INVALID_ARG; }
  if (out->row_order != 0 && out->row_order != 1) { set_error("row_order must be 0 or 1"); return SMPC_ERR_INVALID_ARG; }
  SMPC_HIP_CHECK(hipSetDevice(h->device));
  smpc::KParams k;
  fill_kparams(h, sb, d, &k);
  Staging st(h, sb->on_device);
  SMPC_TRY(bind_inputs(sb, d, &k, &st));
  SMPC_TRY(bind_people(h, sb, k, &st, Sweep::Eval));
  const size_t B = sb->B;
  k.e_row_order = out->row_order;
  SMPC_TRY(st.in(k.e_x, params, B * d.P));
  SMPC_TRY(st.out(k.e_residuals, out->residuals, B * d.M));
  SMPC_TRY(st.out(k.e_jacobian, out->jacobian, B * d.M * d.P));
  SMPC_TRY(st.out(k.e_cost, out->cost, B));
  SMPC_TRY(st.out(k.e_gradient, out->gradient, B * d.P));
  SMPC_TRY(launch(h, st, Sweep::Eval, k));
  return st.finish();
}

}  // extern "C"
