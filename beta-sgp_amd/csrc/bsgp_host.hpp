// bsgp_host.hpp — private to the C-ABI host layer (bsgp_plan.hip, bsgp_solve.hip,
// bsgp_apps.hip): error reporting, the device scope, owning device buffers, the
// stream-ordered scratch of one call and the plan.  Host only; no kernel unit includes it.
#pragma once

#include <hip/hip_runtime.h>

#include <string>
#include <utility>

#include "bsgp_apps.hpp"
#include "bsgp_internal.hpp"
#include "bsgp_layout.hpp"

namespace bsgp {

#define HIP_TRY(expr)                                                                  \
  do {                                                                                 \
    hipError_t e_ = (expr);                                                            \
    if (e_ != hipSuccess)                                                              \
      return fail(BSGP_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));    \
  } while (0)

// Every entry point that works on a plan's device makes it current for the
// call and gives the caller's thread its own current device back on return
// (a plan destroyed from a garbage-collector thread, or a solve on another
// GPU, must not switch the device the caller's framework is using).
struct DeviceGuard {
  int prev = -1;
  hipError_t err = hipSuccess;
  explicit DeviceGuard(int dev) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    err = hipSetDevice(dev);
  }
  ~DeviceGuard() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
  DeviceGuard(const DeviceGuard&) = delete;
  DeviceGuard& operator=(const DeviceGuard&) = delete;
};
#define DEVICE_SCOPE(dev)                                                                   \
  DeviceGuard dev_guard_(dev);                                                              \
  if (dev_guard_.err != hipSuccess)                                                         \
    return fail(BSGP_ERR_HIP, std::string("hipSetDevice: ") + hipGetErrorString(dev_guard_.err))

// An owned device array that only grows.  reserve(n) keeps the array when it
// holds n elements already; otherwise it frees it and allocates exactly n (no
// geometric growth), so the contents are NOT preserved, and a failed
// allocation leaves it empty.  Freed on the device current at destruction: a
// plan's buffers under bsgp_plan_destroy's device scope, temporaries under
// their entry point's.
template <class T>
struct DevBuf {
  T* p = nullptr;
  size_t cap = 0;  // elements
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { (void)release(); }
  hipError_t reserve(size_t n) {
    if (n <= cap) return hipSuccess;
    hipError_t e = release();
    if (e == hipSuccess) e = hipMalloc(&p, n * sizeof(T));
    if (e != hipSuccess) {
      p = nullptr;
      return e;
    }
    cap = n;
    return hipSuccess;
  }
  hipError_t release() {
    const hipError_t e = p ? hipFree(p) : hipSuccess;
    p = nullptr;
    cap = 0;
    return e;
  }
  void swap(DevBuf& o) {
    std::swap(p, o.p);
    std::swap(cap, o.cap);
  }
  size_t bytes() const { return cap * sizeof(T); }
  operator T*() const { return p; }
};

// One pinned host word (256 bytes, as the plan has always allocated them).
struct HostWord {
  int* p = nullptr;
  HostWord() = default;
  HostWord(const HostWord&) = delete;
  HostWord& operator=(const HostWord&) = delete;
  ~HostWord() {
    if (p) (void)hipHostFree(p);
  }
  hipError_t alloc(unsigned flags) { return hipHostMalloc(&p, 256, flags); }
};

// The stream-ordered workspace of one entry point: allocated on the caller's
// stream and freed on it on every exit, so the call stays asynchronous and no
// path leaks.  alloc and finish return BSGP_OK or the failure they reported.
struct StreamScratch {
  void* p = nullptr;
  hipStream_t s;
  explicit StreamScratch(hipStream_t stream) : s(stream) {}
  StreamScratch(const StreamScratch&) = delete;
  StreamScratch& operator=(const StreamScratch&) = delete;
  ~StreamScratch() { (void)release(); }
  int alloc(size_t bytes) {
    const hipError_t e = hipMallocAsync(&p, bytes, s);
    if (e == hipSuccess) return BSGP_OK;
    p = nullptr;
    return fail(BSGP_ERR_HIP, "hipMallocAsync(" + std::to_string(bytes) + " bytes of workspace): " +
                                  hipGetErrorString(e));
  }
  hipError_t release() {
    const hipError_t e = p ? hipFreeAsync(p, s) : hipSuccess;
    p = nullptr;
    return e;
  }
  // after the launches: frees, and reports the launches' error e as
  // "<what> launch: ..." in preference to the free's
  int finish(hipError_t e, const char* what) {
    const hipError_t ef = release();
    if (e != hipSuccess)
      return fail(BSGP_ERR_HIP, std::string(what) + " launch: " + hipGetErrorString(e));
    HIP_TRY(ef);
    return BSGP_OK;
  }
};

}  // namespace bsgp

struct bsgp_plan_s {
  int device = 0;
  int conv_mode = 0;
  bsgp::Geo g{};
  bsgp::DevBuf<bsgp::cd> tw;  // twiddles for P then Q
  bsgp::DevBuf<bsgp::cd> tf;  // tfA then tfAT, each Qh*P (n_tf pairs after bsgp_plan_set_psfs)
  int n_tf = 1;         // 1: one PSF for every image; else image i uses pair i (B == n_tf)
  int kh = 0, kw = 0;   // PSF stamp shape of the plan
  size_t lds_fft_bytes = 0;
  size_t lds_bytes = 0;
  int wg_per_cu = 1;
  int resident_per_cu = 1;  // workgroups of every team kernel one CU holds at once
  int ncu = 256;
  // solver workspace: one slot of slot_stride doubles and one state per image
  bsgp::DevBuf<double> ws;
  size_t slot_stride = 0;
  size_t vec_stride = 0;
  size_t spec_off = 0;
  // second half spectrum per image (SolveArgs::spec2): allocated by the first
  // solve that can speculate, so plans that never do (adaptive beta, float32,
  // teams, phase kernels) keep their footprint
  bsgp::DevBuf<bsgp::cd> spec2;
  bsgp::DevBuf<bsgp::ImgState> st;
  bsgp::DevBuf<int> active;   // device counter of images still iterating
  bsgp::HostWord active_h;    // pinned host mirror for polling
  bsgp::HostWord done_h;      // host-mapped: the solve seq once every image has stopped
  int* done_d = nullptr;      // (its device address)
  int seq = 0;                // the last solve's sequence number (process-wide counter)
  static constexpr int kPollRing = 8;
  hipEvent_t ev_it[kPollRing] = {};  // after iteration it on stream 0 (lookahead polling)
  // sub-batch streams: phases of different sub-batches overlap on the device
  static constexpr int kMaxStreams = 16;
  hipStream_t sub[kMaxStreams] = {};
  hipEvent_t ev_fork = nullptr;
  hipEvent_t ev_join[kMaxStreams] = {};
  int nsub = 0;
  // teams: reduction partials and barrier counters (+ the timeout word)
  bsgp::DevBuf<double> tpart;
  bsgp::DevBuf<unsigned int> tctr;
  // projection pixel lists (proj_cache)
  bsgp::DevBuf<double> plist;
  // operator workspace
  bsgp::DevBuf<bsgp::cd> opws;
  int storage = BSGP_STORAGE_F64;
  // numpy's float32 reduction order over N elements (gn_f32 solves)
  bsgp::DevBuf<int> pwprog;
  bsgp::PwProg pw{};
  // persistent solver: dequeue counter + per-image published iterations
  bsgp::DevBuf<unsigned> pq;
  // the last solve on this plan, for bsgp_state_save: its parameters, output
  // buffers, batch and team size (valid until the next solve overwrites the slots)
  bool last_valid = false;
  bsgp_params last_prm{};
  bsgp_outputs last_out{};
  int last_B = 0, last_T = 0, last_beta0 = 0;
  // compile-time-geometry path of the persistent solver (bsgp_plan_set_static_geo):
  // the next solve's choice (-1: BSGP_STATIC_GEO, default 1), and whether the
  // last solve took the path
  int static_geo_next = -1;
  int last_static_geo = 0;

  bsgp_plan_s() = default;
  bsgp_plan_s(const bsgp_plan_s&) = delete;
  bsgp_plan_s& operator=(const bsgp_plan_s&) = delete;
  // the buffers free themselves; bsgp_plan_destroy makes the device current first
  ~bsgp_plan_s() {
    for (int i = 1; i < nsub; ++i) {
      if (sub[i]) (void)hipStreamDestroy(sub[i]);
      if (ev_join[i]) (void)hipEventDestroy(ev_join[i]);
    }
    if (ev_fork) (void)hipEventDestroy(ev_fork);
    for (hipEvent_t e : ev_it)
      if (e) (void)hipEventDestroy(e);
  }
};

// Owns a plan through its creation's early exits.
struct PlanDeleter {
  void operator()(bsgp_plan p) const { (void)bsgp_plan_destroy(p); }
};
