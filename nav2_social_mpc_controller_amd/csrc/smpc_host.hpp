// smpc_host.hpp — the handle behind the C ABI and the host plumbing every entry point of smpc_hip.hip uses: the error
// text, the HIP / return-code checks, and the staging of a host-pointer call's arrays through device memory.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/smpc.h"

struct smpc_handle {
  smpc_params prm{};
  int device = 0;
  int num_cu = 0;
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  bool timed = false;
  int* queue = nullptr;  // device-side scene queue head and trip counters (KParams::queue)
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
  uint32_t* gp_fail = nullptr;  // smpc_goal_field_batch: the word its kernel sets when a field did not settle (first call)
};

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
  // device room that only the call's kernels use (a workspace the caller of a host-pointer call need not bring): nothing
  // is copied either way. Device-pointer calls bring their own: `dev` is left as it is.
  int scratch(void*& dev, size_t bytes) { return host ? take(bytes, &dev) : SMPC_OK; }
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

}  // namespace
