// bsgp_api.hip — C-ABI host layer of libbsgp.so (declared in include/bsgp.h).
//
// Owns plans (FFT geometry, twiddles, PSF transfer functions built on the
// device) and per-plan workspaces; validates arguments; launches the kernels
// of bsgp_solver.hip.  No PyTorch types cross this boundary.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cerrno>
#include <cstdlib>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "bsgp_internal.hpp"
#include "bsgp_psf.hpp"

using namespace bsgp;

namespace {

thread_local std::string g_err;

int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

// A/B override knobs (BSGP_PERWAVE_MIN_WG, BSGP_PERWAVE_TW, BSGP_COOP_ELEMS,
// BSGP_FOLD_SETUP, BSGP_SPIN_LIMIT, BSGP_LS_PREDICT; environment variables, the default is the
// literal at the call): a value that is not a whole decimal number in [lo, hi]
// is ignored and the default used, so a typo cannot turn into a
// zero (a spin limit of 0 fails every persistent solve with a timeout).
long long env_knob(const char* name, long long def, long long lo, long long hi) {
  const char* e = getenv(name);
  if (!e || !*e) return def;
  char* end = nullptr;
  errno = 0;
  const long long v = strtoll(e, &end, 10);
  if (errno != 0 || end == e || *end != '\0' || v < lo || v > hi) return def;
  return v;
}

#define HIP_TRY(expr)                                                                  \
  do {                                                                                 \
    hipError_t e_ = (expr);                                                            \
    if (e_ != hipSuccess)                                                              \
      return fail(BSGP_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));    \
  } while (0)

size_t round_up(size_t v, size_t m) { return (v + m - 1) / m * m; }

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

// numpy's float32 np.sum over n contiguous elements (numpy 1.26 and 2.x,
// checked against np.sum in tests/test_oracle.py::test_numpy_f32_sum_model):
// the reduction runs over chunks of 8192 (the ufunc buffer), folding
// res = res + pairwise(chunk) from res = 0; pairwise(n) is a leaf for n <= 128
// (8 strided accumulators, or a plain loop below 8) and otherwise
// pairwise(n2) + pairwise(n - n2) with n2 = n/2 - (n/2) % 8.  The program
// lists the leaves (start, length) in order, the inner nodes (value indices
// of the two operands; values 0..L-1 are the leaves, L+k is node k) grouped
// by height so that a level can be added in parallel, and each chunk's root.
struct PwBuild {
  std::vector<int> leaves, nodes_tmp, heights, roots;
  // returns a temporary id: >= 0 leaf, < 0 node -(k+1); *h = height
  int rec(int start, int n, int* h) {
    if (n <= 128) {
      leaves.push_back(start);
      leaves.push_back(n);
      *h = 0;
      return (int)leaves.size() / 2 - 1;
    }
    int n2 = n / 2;
    n2 -= n2 % 8;
    int ha, hb;
    const int a = rec(start, n2, &ha);
    const int b = rec(start + n2, n - n2, &hb);
    nodes_tmp.push_back(a);
    nodes_tmp.push_back(b);
    *h = (ha > hb ? ha : hb) + 1;
    heights.push_back(*h);
    return -(int)(nodes_tmp.size() / 2);
  }
};

std::vector<int> pairwise_program(long n, PwProg* pp) {
  PwBuild b;
  std::vector<int> root_tmp;
  for (long c0 = 0; c0 < n; c0 += 8192) {
    int h;
    root_tmp.push_back(b.rec((int)c0, (int)std::min<long>(8192, n - c0), &h));
  }
  const int L = (int)b.leaves.size() / 2, M = (int)b.heights.size();
  int maxh = 0;
  for (int v : b.heights) maxh = std::max(maxh, v);
  // order the nodes by height (stable), then renumber the operands
  std::vector<int> order, newid(M), lev_off(maxh + 1, 0);
  for (int h = 1; h <= maxh; ++h) {
    lev_off[h - 1] = (int)order.size();
    for (int k = 0; k < M; ++k)
      if (b.heights[k] == h) order.push_back(k);
  }
  lev_off[maxh] = (int)order.size();
  for (int i = 0; i < M; ++i) newid[order[i]] = L + i;
  auto val = [&](int t) { return t >= 0 ? t : newid[-t - 1]; };
  std::vector<int> prog(b.leaves);
  for (int i = 0; i < M; ++i) {
    prog.push_back(val(b.nodes_tmp[2 * order[i]]));
    prog.push_back(val(b.nodes_tmp[2 * order[i] + 1]));
  }
  for (int v : lev_off) prog.push_back(v);
  for (int t : root_tmp) prog.push_back(val(t));
  pp->nleaf = L;
  pp->nnode = M;
  pp->nlev = maxh;
  pp->nchunk = (int)root_tmp.size();
  return prog;
}

std::vector<cd> twiddles(int n) {
  std::vector<cd> t(n);
  const long double pi = 3.141592653589793238462643383279502884L;
  for (int k = 0; k < n; ++k) {
    const long double a = -2.0L * pi * (long double)k / (long double)n;
    t[k] = cmk((double)cosl(a), (double)sinl(a));
  }
  return t;
}

}  // namespace

struct bsgp_plan_s {
  int device = 0;
  int conv_mode = 0;
  Geo g{};
  cd* tw = nullptr;     // twiddles for P then Q
  cd* tf = nullptr;     // tfA then tfAT, each Qh*P (n_tf pairs after bsgp_plan_set_psfs)
  int n_tf = 1;         // 1: one PSF for every image; else image i uses pair i (B == n_tf)
  int kh = 0, kw = 0;   // PSF stamp shape of the plan
  size_t lds_fft_bytes = 0;
  size_t lds_bytes = 0;
  int wg_per_cu = 1;
  int resident_per_cu = 1;  // workgroups of every team kernel one CU holds at once
  int ncu = 256;
  // solver workspace
  double* ws = nullptr;
  size_t ws_slots = 0;
  size_t slot_stride = 0;
  size_t vec_stride = 0;
  size_t spec_off = 0;
  // second half spectrum per image (SolveArgs::spec2): allocated by the first
  // solve that can speculate, so plans that never do (adaptive beta, float32,
  // teams, phase kernels) keep their footprint
  cd* spec2 = nullptr;
  size_t spec2_slots = 0;
  ImgState* st = nullptr;
  size_t st_n = 0;
  int* active = nullptr;     // device counter of images still iterating
  int* active_h = nullptr;   // pinned host mirror for polling
  int* done_h = nullptr;     // host-mapped: the solve seq once every image has stopped
  int* done_d = nullptr;     // (its device address)
  int seq = 0;               // the last solve's sequence number (process-wide counter)
  static constexpr int kPollRing = 8;
  hipEvent_t ev_it[kPollRing] = {};  // after iteration it on stream 0 (lookahead polling)
  // sub-batch streams: phases of different sub-batches overlap on the device
  static constexpr int kMaxStreams = 16;
  hipStream_t sub[kMaxStreams] = {};
  hipEvent_t ev_fork = nullptr;
  hipEvent_t ev_join[kMaxStreams] = {};
  int nsub = 0;
  // teams: reduction partials and barrier counters (+ the timeout word)
  double* tpart = nullptr;
  size_t tpart_n = 0;
  unsigned int* tctr = nullptr;
  size_t tctr_bytes = 0;
  // projection pixel lists (proj_cache)
  double* plist = nullptr;
  size_t plist_n = 0;
  // operator workspace
  cd* opws = nullptr;
  size_t opws_slots = 0;
  int storage = BSGP_STORAGE_F64;
  // numpy's float32 reduction order over N elements (gn_f32 solves)
  int* pwprog = nullptr;
  PwProg pw{};
  // persistent solver: dequeue counter + per-image published iterations
  unsigned* pq = nullptr;
  size_t pq_n = 0;
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
};

// A solve entry point that can fail before solve_impl: the choice of
// bsgp_plan_set_static_geo belongs to this call whatever becomes of it, and
// until a solve runs the plan reports no static path.
struct StaticGeoCall {
  bsgp_plan p;
  explicit StaticGeoCall(bsgp_plan q) : p(q) { p->last_static_geo = 0; }
  ~StaticGeoCall() { p->static_geo_next = -1; }
};

// Capacity of one thread's projection list: the pixels it streams in one pass
// (stream2 in bsgp_solver.hip: T == 1 strides pixel pairs over the block; T > 1
// strides row chunks of cp = nfw*W pairs over the members).
static int proj_list_cap(const Geo& g, int T) {
  const long npair = ((long)g.H * g.W + 1) / 2;
  const int nb = plan_block(g);
  if (T == 1) return (int)(2 * ((npair + nb - 1) / nb));
  const long cp = (long)g.nfw * g.W;
  const long nch = (npair + cp - 1) / cp;
  return (int)(2 * ((nch + T - 1) / T) * ((cp + nb - 1) / nb));
}

static int ensure_plist(bsgp_plan p, size_t n) {
  if (n > p->plist_n) {
    if (p->plist) HIP_TRY(hipFree(p->plist));
    p->plist = nullptr;
    p->plist_n = 0;
    HIP_TRY(hipMalloc(&p->plist, n * sizeof(double)));
    p->plist_n = n;
  }
  return BSGP_OK;
}

static size_t spec2_stride(const bsgp_plan_s* p) {
  return round_up((size_t)p->g.sld * p->g.Qh, 16);  // the slot spectrum's size
}

static int ensure_spec2(bsgp_plan p, size_t slots) {
  if (slots > p->spec2_slots) {
    if (p->spec2) HIP_TRY(hipFree(p->spec2));
    p->spec2 = nullptr;
    p->spec2_slots = 0;
    HIP_TRY(hipMalloc(&p->spec2, slots * spec2_stride(p) * sizeof(cd)));
    p->spec2_slots = slots;
  }
  return BSGP_OK;
}

static int ensure_ws(bsgp_plan p, size_t slots) {
  if (slots > p->ws_slots) {
    if (p->ws) HIP_TRY(hipFree(p->ws));
    p->ws = nullptr;
    p->ws_slots = 0;
    HIP_TRY(hipMalloc(&p->ws, slots * p->slot_stride * sizeof(double)));
    p->ws_slots = slots;
  }
  if (slots > p->st_n) {
    if (p->st) HIP_TRY(hipFree(p->st));
    p->st = nullptr;
    p->st_n = 0;
    HIP_TRY(hipMalloc(&p->st, slots * sizeof(ImgState)));
    p->st_n = slots;
  }
  return BSGP_OK;
}

// Workgroups per image.  Every member of every team must be resident at once
// (the team barriers spin): B*T never exceeds the CUs times the workgroups per
// CU the runtime reports for every team kernel of the plan's build
// (p->resident_per_cu, hipOccupancyMaxActiveBlocksPerMultiprocessor).  Each
// member keeps at least one row pair and one column per FFT wave.
// Solve sequence numbers for the lookahead poll's host-mapped word: one
// process-wide counter, so no plan (nor a reused pinned block) ever sees a
// value another solve wrote.
static std::atomic<int> g_solve_seq{0};

static int choose_team(const bsgp_plan_s* p, int B, int req) {
  if (req == 1) return 1;
  const Geo& g = p->g;
  const int rows2 = (g.H + 1) / 2;
  int tgeo = rows2 / g.nfw;
  if (g.Qh / g.nfw < tgeo) tgeo = g.Qh / g.nfw;
  const int res = p->ncu * p->resident_per_cu / B;  // resident members per image
  // auto: one workgroup per CU (cooperative plans would fit two per CU, but
  // one per CU measured faster on C4: 1262 vs 1180 it/s)
  int T = std::min(p->ncu / B, tgeo);
  if (req > 1) T = std::min(req, tgeo);
  T = std::min(T, res);
  // the barrier words and the group leaders' polls cover at most kMaxTeam
  // members (bsgp_device.hpp)
  T = std::min(T, kMaxTeam);
  return T < 1 ? 1 : T;
}

static int ensure_team(bsgp_plan p, size_t B, int T) {
  const size_t np = B * kPartBufs * (size_t)(T + 8) * kMaxRed;
  if (T > 1 && np > p->tpart_n) {
    if (p->tpart) HIP_TRY(hipFree(p->tpart));
    p->tpart = nullptr;
    p->tpart_n = 0;
    HIP_TRY(hipMalloc(&p->tpart, np * sizeof(double)));
    p->tpart_n = np;
  }
  const size_t cb = round_up((B * kTeamWords + kTeamLine) * sizeof(unsigned int), 128);
  if (cb > p->tctr_bytes) {
    if (p->tctr) HIP_TRY(hipFree(p->tctr));
    p->tctr = nullptr;
    p->tctr_bytes = 0;
    HIP_TRY(hipMalloc(&p->tctr, cb));
    p->tctr_bytes = cb;
  }
  return BSGP_OK;
}

extern "C" {

int32_t bsgp_abi_version(void) { return 3; }

// Diagnostics (not in include/bsgp.h): per-phase shader cycles of a build
// with -DBSGP_PHASE_PROF; returns BSGP_ERR_UNSUPPORTED otherwise.
int bsgp_phase_prof(uint64_t* out, int32_t n, int32_t reset) {
  hipError_t e = phase_prof(reinterpret_cast<unsigned long long*>(out), n, reset);
  if (e == hipErrorNotSupported) return fail(BSGP_ERR_UNSUPPORTED, "built without BSGP_PHASE_PROF");
  if (e != hipSuccess) return fail(BSGP_ERR_HIP, hipGetErrorString(e));
  return BSGP_OK;
}

// Diagnostics (not in include/bsgp.h): the numpy float32 reduction program the
// plans use for N = n elements (tests/test_oracle.py evaluates it against
// np.sum).  counts = {nleaf, nnode, nlev, nchunk}; returns the program length,
// copying at most cap ints to out.
int64_t bsgp_pairwise_program(int64_t n, int32_t* out, int64_t cap, int32_t* counts) {
  if (n < 1) return fail(BSGP_ERR_ARG, "n must be >= 1");
  PwProg pp{};
  const std::vector<int> prog = pairwise_program((long)n, &pp);
  if (counts) {
    counts[0] = pp.nleaf;
    counts[1] = pp.nnode;
    counts[2] = pp.nlev;
    counts[3] = pp.nchunk;
  }
  for (int64_t i = 0; out && i < cap && i < (int64_t)prog.size(); ++i) out[i] = prog[i];
  return (int64_t)prog.size();
}

const char* bsgp_last_error(void) { return g_err.c_str(); }

int bsgp_device_synchronize(void) {
  HIP_TRY(hipDeviceSynchronize());
  return BSGP_OK;
}

int bsgp_plan_create(int32_t H, int32_t W, const double* psf, int32_t kh, int32_t kw,
                     int32_t conv_mode, int32_t storage, int32_t device, bsgp_plan* out) {
  return bsgp_plan_create_checked(H, W, psf, kh, kw, conv_mode, storage, device, 0, out);
}

int bsgp_plan_create_checked(int32_t H, int32_t W, const double* psf, int32_t kh, int32_t kw,
                             int32_t conv_mode, int32_t storage, int32_t device,
                             int32_t psf_checked, bsgp_plan* out) {
  if (!out) return fail(BSGP_ERR_ARG, "out is NULL");
  if (storage != BSGP_STORAGE_F64 && storage != BSGP_STORAGE_F32)
    return fail(BSGP_ERR_ARG, "bad storage");
  *out = nullptr;
  if (H < 1 || W < 1 || kh < 1 || kw < 1 || !psf) return fail(BSGP_ERR_ARG, "bad shape or psf");
  if (conv_mode != BSGP_CONV_CIRCULAR && conv_mode != BSGP_CONV_LINEAR_FILL)
    return fail(BSGP_ERR_ARG, "bad conv_mode");
  if (conv_mode == BSGP_CONV_CIRCULAR && (kh != H || kw != W))
    return fail(BSGP_ERR_ARG,
                "circular A (use_original_SGP_Afunction=True) needs psf.shape == gn.shape");
  // PSF normalisation check (sgp.py:97-102), unless the caller has made it in
  // the PSF's own dtype (a float32 PSF sums to 1 in float32, not in float64)
  if (!psf_checked) {
    double s = 0;
    for (int i = 0; i < kh * kw; ++i) s += psf[i];
    if (std::fabs(s - 1.0) > 1e4 * 2.220446049250313e-16) {
      char b[160];
      snprintf(b, sizeof b, "PSF is not normalized! sum(psf) - 1. = %.17g", s - 1.0);
      return fail(BSGP_ERR_PSF, b);
    }
  }
  DEVICE_SCOPE(device);
  bsgp_plan p = new bsgp_plan_s();
  p->device = device;
  p->conv_mode = conv_mode;
  p->kh = kh;
  p->kw = kw;
  Geo& g = p->g;
  g.H = H;
  g.W = W;
  if (conv_mode == BSGP_CONV_CIRCULAR) {
    g.P = H;
    g.Q = W;
  } else {
    // zero-fill linear convolution on a P x Q circular grid without
    // wrap-around for either kernel (A: kh x kw, AT: kw x kh)
    const int km = kh > kw ? kh : kw;
    int pmin = H + km / 2, qmin = W + km / 2;
    if (pmin < km) pmin = km;
    if (qmin < km) qmin = km;
    g.P = next_fast_len(pmin);
    g.Q = next_fast_len(qmin);
  }
  g.Qh = g.Q / 2 + 1;
  // stored half spectrum: column k at k * sld (even, so row pairs stay 32-B aligned)
  g.sld = H + ((H & 1) ? 1 : 0);
  g.fp.n = g.P;
  g.fq.n = g.Q;
  if (!plan_radices(g.P, g.fp.radix, &g.fp.ns) || !plan_radices(g.Q, g.fq.radix, &g.fq.ns)) {
    delete p;
    return fail(BSGP_ERR_UNSUPPORTED, "FFT length has too many factors");
  }
  int maxlen = g.P > g.Q ? g.P : g.Q;
  // one FFT buffer also stages a row pair's stored spectrum (2*Qh, row_inv2); odd spreads banks
  g.lpad = (maxlen + 1 > 2 * g.Qh ? maxlen + 1 : 2 * g.Qh) | 1;
  // LDS: nfw waves x 2 buffers, + reduction scratch
  size_t red_bytes = (size_t)kWaves * kMaxRed * sizeof(double) + kSharedBytes;
  int nfw = kWaves;
  size_t budget = 160 * 1024 / 4 - 256;  // four workgroups per CU
  p->wg_per_cu = 4;
  auto need = [&](int n) { return (size_t)n * 2 * g.lpad * sizeof(cd) + red_bytes; };
  g.coop = 0;
  // per-wave transforms at three workgroups per CU (12 waves/CU) before the
  // cooperative build's one 512-thread workgroup per CU (8 waves): 375^2 tiles
  // on their 400-point grid fit (52.9 KB of 54.3 KB)
  // The twiddle tables must fit beside the buffers too (BSGP_PERWAVE_TW=0: not):
  // a wave's transform that reads its twiddles from global memory waits on
  // them in every stage (375^2 tiles at 3 WG/CU: the 400-point row and column
  // transforms took 3.5x the cycles per point of C3's 270-point ones, phase
  // profile), so two workgroups per CU with LDS twiddles can beat three without.
  const size_t twb_all = (size_t)(g.P == g.Q ? g.P : g.P + g.Q) * sizeof(cd);
  {
    // plans whose per-wave transforms fit the LDS at three or two workgroups
    // per CU take them instead of the cooperative build when this allows.
    // Per-wave over cooperative (A/B): 375^2 tiles at 3 WG/CU, 1024 per launch,
    // 68.6 k -> 87.5 k image-it/s; 450^2 at 2 WG/CU 48.3 -> 59.7 k
    const int min_wg = (int)env_knob("BSGP_PERWAVE_MIN_WG", 2, 2, 4);
    const size_t tw_need = env_knob("BSGP_PERWAVE_TW", 1, 0, 1) ? twb_all : 0;
    for (int wg = 3; wg >= 2 && wg >= min_wg; --wg) {
      const size_t bw = 160 * 1024 / wg - 256;
      if (need(kWaves) > budget && need(kWaves) + tw_need <= bw) {
        budget = bw;
        p->wg_per_cu = wg;
        break;
      }
    }
  }
  if (need(kWaves) > budget) {
    // transforms too long for a wave each at four workgroups per CU: the
    // whole workgroup runs one transform at a time (cooperative passes)
    g.coop = 1;
    nfw = 1;
    budget = 160 * 1024 - 256;
    // wave partials of the cooperative build's workgroups (kCoopBlock threads)
    red_bytes = (size_t)(kCoopBlock / 64) * kMaxRed * sizeof(double) + kSharedBytes;
    if (need(1) > budget) {
      delete p;
      return fail(BSGP_ERR_UNSUPPORTED, "FFT length too large for one workgroup's LDS");
    }
    // thread groups (bsgp_device.hpp, cooperative passes): as many as the LDS
    // holds, each at least two waves and covering its transform in one load
    // batch (4 elements per thread); the 400/480-point grids take four.  A
    // transform too long for that (C4's 2048 points) takes two groups of
    // 256 threads with two load batches (BSGP_COOP_ELEMS, 8 per thread) when the LDS
    // holds both: each workgroup then runs two row pairs through the same
    // stages and barriers, and its radix-8 stages use all 512 lanes instead
    // of 256: C4 k_ls 180 -> 157 us, k_bb 72 -> 68 us, 2114 -> 2221 it/s
    // (float32 storage; f64 1868 -> 1971), the column kernel staying on one
    // group (nfc below).
    // elements per thread a group may take when one batch leaves one group
    const int elems = (int)env_knob("BSGP_COOP_ELEMS", 8, 4, 8);  // (A/B override)
    auto groups = [&](int el) {
      for (int n = kCoopGroups; n > 1; n /= 2)
        if (need(n) <= budget && kCoopBlock / n >= 128 && maxlen <= el * (kCoopBlock / n))
          return n;
      return 1;
    };
    nfw = groups(4);
    if (nfw == 1 && elems > 4) nfw = groups(elems);
    p->wg_per_cu = (int)(budget / need(nfw));
    if (p->wg_per_cu > 4) p->wg_per_cu = 4;
    budget = 160 * 1024 / p->wg_per_cu - 256;
  }
  g.nfw = nfw;
  // the column kernel of a cooperative plan keeps one load batch per thread: a
  // 2048-point column per 256-thread group doubled C4's k_col, 42 -> 75 us,
  // while the row passes gained
  int nfc = nfw;
  while (g.coop && nfc > 1 && maxlen > 4 * (kCoopBlock / nfc)) nfc /= 2;
  g.nfc = nfc;
  p->lds_fft_bytes = (size_t)nfw * 2 * g.lpad * sizeof(cd);
  p->lds_bytes = p->lds_fft_bytes + red_bytes;
  // the per-wave transforms' twiddle tables live in LDS when they fit the same
  // budget (one table when P == Q), else they read the global table (as the
  // cooperative workgroup-wide transforms always do)
  g.fp.lds_tw = g.fq.lds_tw = -1;
  g.fp.lds_tw2 = g.fq.lds_tw2 = -1;
  g.tw2 = 0;
  g.twmix = -1;
  // cooperative 2048-point transforms (fft_wide's static plan): their twiddles
  // as a two-level table (bsgp_fft.hpp Tw2, 1.5 KiB) at the start of every
  // kernel's LDS -- the full 32 KiB table does not fit beside the buffers, and
  // from global memory every Stockham stage waited on an L2 round trip
  // and, after them, the 2048-point column transforms' stage tables
  // (bsgp_fft.hpp TwMixL: 9 KiB, the global table's entries for the second and
  // third Stockham stages; loaded by every kernel with the two-level tables)
  if (g.coop) {
    size_t off = 0;
    if (g.P == 2048) {
      g.fp.lds_tw2 = 0;
      off += (64 + 2048 / 64) * sizeof(cd);
    }
    if (g.Q == 2048) {
      if (g.P == 2048) {
        g.fq.lds_tw2 = 0;
      } else {
        g.fq.lds_tw2 = (int)off;
        off += (64 + 2048 / 64) * sizeof(cd);
      }
    }
    if (g.P == 2048) {
      g.twmix = (int)off;
      off += (64 + 512) * sizeof(cd);
    }
    g.tw2 = (int)round_up(off, 16);
    p->lds_bytes += g.tw2;
  }
  if (!g.coop) {
    const size_t twb = (size_t)(g.P == g.Q ? g.P : g.P + g.Q) * sizeof(cd);
    if (p->lds_bytes + twb <= budget) {
      g.fp.lds_tw = (int)p->lds_bytes;
      g.fq.lds_tw = g.P == g.Q ? g.fp.lds_tw : (int)(p->lds_bytes + (size_t)g.P * sizeof(cd));
      p->lds_bytes += twb;
    }
  }
  {
    int ncu = 0;
    if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess &&
        ncu > 0)
      p->ncu = ncu;
  }
  if (bsgp_c512_args_size() != sizeof(SolveArgs) || bsgp_c512_block() != kCoopBlock) {
    delete p;
    return fail(BSGP_ERR_HIP, "cooperative 512-thread build does not match this library");
  }
  if (bsgp_app_args_size() != sizeof(SolveArgs)) {
    delete p;
    return fail(BSGP_ERR_HIP, "application-size persistent build does not match this library");
  }
  if (set_solver_lds_limit(p->lds_bytes) != hipSuccess) {
    delete p;
    return fail(BSGP_ERR_HIP, "hipFuncSetAttribute(MaxDynamicSharedMemorySize) failed");
  }
  if (team_resident_per_cu(g.coop != 0, storage, p->lds_bytes, &p->resident_per_cu) !=
          hipSuccess ||
      p->resident_per_cu < 1) {
    delete p;
    return fail(BSGP_ERR_HIP, "occupancy query of the team kernels failed");
  }
  // twiddles
  {
    std::vector<cd> tw = twiddles(g.P);
    std::vector<cd> twq = twiddles(g.Q);
    tw.insert(tw.end(), twq.begin(), twq.end());
    if (hipMalloc(&p->tw, tw.size() * sizeof(cd)) != hipSuccess ||
        hipMemcpy(p->tw, tw.data(), tw.size() * sizeof(cd), hipMemcpyHostToDevice) != hipSuccess) {
      bsgp_plan_destroy(p);
      return fail(BSGP_ERR_HIP, "twiddle upload failed");
    }
    g.fp.tw = p->tw;
    g.fq.tw = p->tw + g.P;
  }
  // circularly-placed kernels for A and AT on the P x Q grid
  const size_t PQ = (size_t)g.P * g.Q;
  std::vector<double> kA(PQ, 0.0), kAT(PQ, 0.0);
  if (conv_mode == BSGP_CONV_CIRCULAR) {
    // fftshift(psf): out[i][j] = psf[(i - H//2) mod H][(j - W//2) mod W]  (sgp.py:109)
    for (int i = 0; i < H; ++i)
      for (int j = 0; j < W; ++j) {
        const int si = ((i - H / 2) % H + H) % H, sj = ((j - W / 2) % W + W) % W;
        kA[(size_t)i * W + j] = psf[(size_t)si * W + sj];
      }
  } else {
    // astropy convolve_fft(normalize_kernel=True): kernel/sum, centre at k//2
    // (convolve.py:664-672, 770-787); AT uses psf.conj().T (sgp.py:157)
    double s = 0;
    for (int i = 0; i < kh * kw; ++i) s += psf[i];
    for (int u = 0; u < kh; ++u)
      for (int v = 0; v < kw; ++v) {
        const double val = psf[(size_t)u * kw + v] / s;
        const int a = ((u - kh / 2) % g.P + g.P) % g.P, b = ((v - kw / 2) % g.Q + g.Q) % g.Q;
        kA[(size_t)a * g.Q + b] += val;
        // transposed kernel T[v][u] (shape kw x kh), centre (kw//2, kh//2)
        const int at = ((v - kw / 2) % g.P + g.P) % g.P, bt = ((u - kh / 2) % g.Q + g.Q) % g.Q;
        kAT[(size_t)at * g.Q + bt] += val;
      }
  }
  double* kc = nullptr;
  cd* spec = nullptr;
  const size_t tfn = (size_t)g.Qh * g.P;
  int rc = BSGP_OK;
  if (hipMalloc(&p->tf, 2 * tfn * sizeof(cd)) != hipSuccess ||
      hipMalloc(&kc, 2 * PQ * sizeof(double)) != hipSuccess ||
      hipMalloc(&spec, (size_t)g.P * g.Qh * sizeof(cd)) != hipSuccess) {
    rc = fail(BSGP_ERR_HIP, "plan allocation failed");
  }
  if (rc == BSGP_OK) {
    g.tfA = p->tf;
    g.tfAT = p->tf + tfn;
    const double scale = 1.0 / ((double)g.P * (double)g.Q);
    if (hipMemcpy(kc, kA.data(), PQ * sizeof(double), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(kc + PQ, kAT.data(), PQ * sizeof(double), hipMemcpyHostToDevice) != hipSuccess)
      rc = fail(BSGP_ERR_HIP, "psf upload failed");
    if (rc == BSGP_OK) {
      if (launch_build_tf(g, kc, spec, p->tf, scale, 0, p->lds_bytes, 0) != hipSuccess)
        rc = fail(BSGP_ERR_HIP, "build_tf(A) launch failed");
      else if (hipDeviceSynchronize() != hipSuccess)
        rc = fail(BSGP_ERR_HIP, "build_tf(A) failed");
    }
    if (rc == BSGP_OK) {
      // circular: TF_AT = conj(TF_A) (sgp.py:110); linear: FFT of the transposed kernel
      const bool circ = conv_mode == BSGP_CONV_CIRCULAR;
      if (launch_build_tf(g, circ ? kc : kc + PQ, spec, p->tf + tfn, scale, circ ? 1 : 0,
                          p->lds_bytes, 0) != hipSuccess)
        rc = fail(BSGP_ERR_HIP, "build_tf(AT) launch failed");
      else if (hipDeviceSynchronize() != hipSuccess)
        rc = fail(BSGP_ERR_HIP, "build_tf(AT) failed");
    }
  }
  if (kc) (void)hipFree(kc);
  if (spec) (void)hipFree(spec);
  if (rc != BSGP_OK) {
    std::string m = g_err;
    bsgp_plan_destroy(p);
    return fail(rc, m);
  }
  const size_t N = (size_t)H * W;
  p->storage = storage;
  // slot: gn and bkg in float64 (vec_stride each), the seven iteration vectors
  // in the storage type, then the half spectrum (complex float64), then two
  // more vectors
  p->vec_stride = round_up(N, 32);
  const size_t vbytes = storage == BSGP_STORAGE_F32 ? sizeof(float) : sizeof(double);
  p->spec_off = 2 * p->vec_stride + 7 * p->vec_stride * vbytes / sizeof(double);
  // and, last, the second x_tf / pw pair (ImgState::par_tf; slot_bufs finds it
  // from the slot's end)
  p->slot_stride = p->spec_off + round_up((size_t)g.sld * g.Qh * 2, 32) + 2 * p->vec_stride;
  {
    const std::vector<int> prog = pairwise_program((long)N, &p->pw);
    if (hipMalloc(&p->pwprog, prog.size() * sizeof(int)) != hipSuccess ||
        hipMemcpy(p->pwprog, prog.data(), prog.size() * sizeof(int), hipMemcpyHostToDevice) !=
            hipSuccess) {
      bsgp_plan_destroy(p);
      return fail(BSGP_ERR_HIP, "pairwise program upload failed");
    }
    p->pw.prog = p->pwprog;
  }
  if (hipMalloc(&p->active, 256) != hipSuccess ||
      hipHostMalloc(&p->active_h, 256, hipHostMallocDefault) != hipSuccess ||
      hipHostMalloc(&p->done_h, 256, hipHostMallocMapped) != hipSuccess ||
      hipHostGetDevicePointer((void**)&p->done_d, p->done_h, 0) != hipSuccess) {
    bsgp_plan_destroy(p);
    return fail(BSGP_ERR_HIP, "counter allocation failed");
  }
  // a reused pinned block may still hold an old plan's seq; seqs
  // also come from one process-wide counter, so a stale word never matches
  *p->done_h = 0;
  *out = p;
  return BSGP_OK;
}

int bsgp_plan_destroy(bsgp_plan p) {
  if (!p) return BSGP_OK;
  DeviceGuard dev_guard_(p->device);
  if (p->tw) (void)hipFree(p->tw);
  if (p->tf) (void)hipFree(p->tf);
  if (p->ws) (void)hipFree(p->ws);
  if (p->spec2) (void)hipFree(p->spec2);
  for (int i = 1; i < p->nsub; ++i) {
    if (p->sub[i]) (void)hipStreamDestroy(p->sub[i]);
    if (p->ev_join[i]) (void)hipEventDestroy(p->ev_join[i]);
  }
  if (p->ev_fork) (void)hipEventDestroy(p->ev_fork);
  if (p->st) (void)hipFree(p->st);
  if (p->active) (void)hipFree(p->active);
  if (p->active_h) (void)hipHostFree(p->active_h);
  if (p->done_h) (void)hipHostFree(p->done_h);
  for (hipEvent_t e : p->ev_it)
    if (e) (void)hipEventDestroy(e);
  if (p->opws) (void)hipFree(p->opws);
  if (p->tpart) (void)hipFree(p->tpart);
  if (p->tctr) (void)hipFree(p->tctr);
  if (p->plist) (void)hipFree(p->plist);
  if (p->pwprog) (void)hipFree(p->pwprog);
  if (p->pq) (void)hipFree(p->pq);
  delete p;
  return BSGP_OK;
}

int bsgp_plan_set_psfs(bsgp_plan p, const double* psfs, int32_t n, void* stream) {
  if (!p || !psfs || n < 1) return fail(BSGP_ERR_ARG, "bad arguments");
  Geo& g = p->g;
  const bool circ = p->conv_mode == BSGP_CONV_CIRCULAR;
  // the device placement stores (no accumulation): the kernel must not wrap on the grid
  if (!circ && (p->kh > g.P || p->kw > g.Q || p->kw > g.P || p->kh > g.Q))
    return fail(BSGP_ERR_ARG, "per-image PSFs need a kernel no larger than the FFT grid");
  DEVICE_SCOPE(p->device);
  hipStream_t s = (hipStream_t)stream;
  const size_t PQ = (size_t)g.P * g.Q, tfn = (size_t)g.Qh * g.P, specn = (size_t)g.P * g.Qh;
  // chunks bound the placement/spectrum workspace (~256 MiB)
  const size_t per = 2 * PQ * sizeof(double) + specn * sizeof(cd);
  const int chunk = (int)std::max<size_t>(1, std::min<size_t>((size_t)n, (256u << 20) / per));
  cd* tf = nullptr;
  double* kc = nullptr;
  cd* spec = nullptr;
  double* sums = nullptr;
  int rc = BSGP_OK;
  if (hipMalloc(&tf, (size_t)n * 2 * tfn * sizeof(cd)) != hipSuccess ||
      hipMalloc(&kc, (size_t)chunk * 2 * PQ * sizeof(double)) != hipSuccess ||
      hipMalloc(&spec, (size_t)chunk * specn * sizeof(cd)) != hipSuccess ||
      hipMalloc(&sums, (size_t)n * sizeof(double)) != hipSuccess)
    rc = fail(BSGP_ERR_HIP, "per-image PSF allocation failed");
  const double scale = 1.0 / ((double)g.P * (double)g.Q);
  Geo gb = g;
  gb.tf_stride = 0;
  for (int c0 = 0; rc == BSGP_OK && c0 < n; c0 += chunk) {
    const int m = std::min(chunk, n - c0);
    cd* t = tf + (size_t)c0 * 2 * tfn;
    if (hipMemsetAsync(kc, 0, (size_t)m * 2 * PQ * sizeof(double), s) != hipSuccess ||
        launch_place_psfs(gb, m, psfs + (size_t)c0 * p->kh * p->kw, p->kh, p->kw, circ ? 1 : 0,
                          kc, sums + c0, s) != hipSuccess ||
        launch_build_tfs(gb, m, kc, 2 * PQ, spec, specn, t, 2 * tfn, scale, 0, p->lds_bytes,
                         s) != hipSuccess ||
        // circular: TF_AT = conj(TF_A) (sgp.py:110); linear: FFT of the transposed kernel
        launch_build_tfs(gb, m, circ ? kc : kc + PQ, 2 * PQ, spec, specn, t + tfn, 2 * tfn,
                         scale, circ ? 1 : 0, p->lds_bytes, s) != hipSuccess)
      rc = fail(BSGP_ERR_HIP, "per-image TF launch failed");
  }
  std::vector<double> hs(n);
  if (rc == BSGP_OK && (hipMemcpyAsync(hs.data(), sums, (size_t)n * sizeof(double),
                                       hipMemcpyDeviceToHost, s) != hipSuccess ||
                        hipStreamSynchronize(s) != hipSuccess))
    rc = fail(BSGP_ERR_HIP, "per-image TF build failed");
  for (int i = 0; rc == BSGP_OK && i < n; ++i)
    if (!(std::fabs(hs[i] - 1.0) <= 1e4 * 2.220446049250313e-16)) {  // sgp.py:97-102
      char b[160];
      snprintf(b, sizeof b, "PSF %d is not normalized! sum(psf) - 1. = %.17g", i, hs[i] - 1.0);
      rc = fail(BSGP_ERR_PSF, b);
    }
  if (kc) (void)hipFree(kc);
  if (spec) (void)hipFree(spec);
  if (sums) (void)hipFree(sums);
  if (rc != BSGP_OK) {
    if (tf) (void)hipFree(tf);
    return rc;
  }
  if (p->tf) (void)hipFree(p->tf);
  p->tf = tf;
  p->n_tf = n;
  g.tfA = tf;
  g.tfAT = tf + tfn;
  g.tf_stride = n > 1 ? 2 * tfn : 0;
  return BSGP_OK;
}

int bsgp_plan_set_static_geo(bsgp_plan p, int32_t mode) {
  if (!p) return fail(BSGP_ERR_ARG, "plan is NULL");
  if (mode < -1 || mode > 1) return fail(BSGP_ERR_ARG, "static_geo must be -1, 0 or 1");
  p->static_geo_next = mode;
  return BSGP_OK;
}

int bsgp_plan_static_geo(bsgp_plan p, int32_t* used) {
  if (!p || !used) return fail(BSGP_ERR_ARG, "plan or used is NULL");
  *used = p->last_static_geo;
  return BSGP_OK;
}

int bsgp_plan_info(bsgp_plan p, int32_t* P, int32_t* Q, int64_t* slot_bytes,
                   int32_t* fft_waves) {
  if (!p) return fail(BSGP_ERR_ARG, "plan is NULL");
  if (P) *P = p->g.P;
  if (Q) *Q = p->g.Q;
  if (slot_bytes) *slot_bytes = (int64_t)(p->slot_stride * sizeof(double));
  if (fft_waves) *fft_waves = p->g.nfw;
  return BSGP_OK;
}

static int check_params(const bsgp_params* q) {
  if (!q) return fail(BSGP_ERR_ARG, "params is NULL");
  if (q->variant != BSGP_VARIANT_KL && q->variant != BSGP_VARIANT_BETA)
    return fail(BSGP_ERR_ARG, "bad variant");
  if (q->MAXIT < 1) return fail(BSGP_ERR_ARG, "MAXIT must be >= 1");
  if (q->M_alpha < 1 || q->M_alpha > 32) return fail(BSGP_ERR_ARG, "M_alpha must be in [1, 32]");
  if (q->M < 1 || q->M > 32) return fail(BSGP_ERR_ARG, "M must be in [1, 32]");
  if (q->ls_spec < 1 || q->ls_spec > 8) return fail(BSGP_ERR_ARG, "ls_spec must be in [1, 8]");
  if (q->init_recon < 0 || q->init_recon > 3) return fail(BSGP_ERR_ARG, "bad init_recon");
  if (q->proj_type != 0 && q->proj_type != 1) return fail(BSGP_ERR_ARG, "bad proj_type");
  if (q->scale_data < 0 || q->scale_data > 2) return fail(BSGP_ERR_ARG, "bad scale_data");
  if (q->flux_f32 && !(q->gn_f32 && q->scale_data != 2))
    return fail(BSGP_ERR_ARG, "flux_f32 needs gn_f32 with scale_data 0 or 1");
  return BSGP_OK;
}

// Profiled solves: events around every kernel class of every iteration.
struct SolveProf {
  std::vector<hipEvent_t> ev;  // [MAXIT][6] + setup pair
  double* kernel_ms;
  int64_t* launches;
};

// A resumed solve (bsgp_solve_resume): k_state_load takes the place of the
// setup, and the iteration loop goes on where the records stopped.
struct ResumeCtx {
  StateArgs sa;     // the records (rec, rec_bytes, index, L, hist_cap); solve_impl adds the plan's part
  int T;            // the records' team size
  int it0;          // first iteration to launch: the fewest iterations done + 1
  bool uniform;     // every image that goes on has done `done_it` iterations
  int done_it;
  int beta0_given;  // the records' solve had per-image betas (picks the line-search build)
};

static int solve_impl(bsgp_plan p, int32_t B, const bsgp_params* prm, const bsgp_inputs* in,
                      const bsgp_outputs* out, void* stream, SolveProf* prof,
                      const ResumeCtx* rs = nullptr);

int bsgp_solve_device(bsgp_plan p, int32_t B, const bsgp_params* prm, const bsgp_inputs* in,
                      const bsgp_outputs* out, void* stream) {
  return solve_impl(p, B, prm, in, out, stream, nullptr);
}

int bsgp_solve_profiled(bsgp_plan p, int32_t B, const bsgp_params* prm, const bsgp_inputs* in,
                        const bsgp_outputs* out, void* stream, double* kernel_ms,
                        int64_t* launches) {
  if (!kernel_ms || !launches) return fail(BSGP_ERR_ARG, "kernel_ms / launches missing");
  if (!prm) return fail(BSGP_ERR_ARG, "params is NULL");
  if (!p) return fail(BSGP_ERR_ARG, "plan is NULL");
  StaticGeoCall sgc(p);
  DEVICE_SCOPE(p->device);
  SolveProf prof;
  prof.kernel_ms = kernel_ms;
  prof.launches = launches;
  const size_t nev = 6 * (size_t)(prm->MAXIT > 0 ? prm->MAXIT : 0) + 2;
  prof.ev.resize(nev, nullptr);
  int rc = BSGP_OK;
  for (size_t i = 0; i < nev && rc == BSGP_OK; ++i)
    if (hipEventCreate(&prof.ev[i]) != hipSuccess) rc = fail(BSGP_ERR_HIP, "event create failed");
  if (rc == BSGP_OK) {
    bsgp_params q = *prm;
    q.streams = 1;  // one stream: kernel spans do not overlap
    rc = solve_impl(p, B, &q, in, out, stream, &prof);
  }
  for (hipEvent_t e : prof.ev)
    if (e) (void)hipEventDestroy(e);
  return rc;
}

static int solve_impl(bsgp_plan p, int32_t B, const bsgp_params* prm, const bsgp_inputs* in,
                      const bsgp_outputs* out, void* stream, SolveProf* prof,
                      const ResumeCtx* rs) {
  if (!p) return fail(BSGP_ERR_ARG, "plan is NULL");
  // bsgp_plan_set_static_geo's choice is this call's alone, also when the call
  // fails below before anything runs (then no path was taken)
  const int static_geo_choice = p->static_geo_next;
  p->static_geo_next = -1;
  p->last_static_geo = 0;
  int rc = check_params(prm);
  if (rc) return rc;
  if (B < 1) return fail(BSGP_ERR_ARG, "B must be >= 1");
  if (!rs) {
    if (!in || !in->gn || !in->bkg) return fail(BSGP_ERR_ARG, "inputs gn/bkg missing");
    if ((prm->init_recon == 1 || prm->scale_data == 2) && !in->x0)
      return fail(BSGP_ERR_ARG, "init_recon=1 and scale_data=2 need x0");
  }
  if (!out || !out->x || !out->iters || !out->discr) return fail(BSGP_ERR_ARG, "outputs missing");
  if (out->err && (!in || !in->obj)) return fail(BSGP_ERR_ARG, "err needs the ground truth obj");
  if (p->n_tf > 1 && B != p->n_tf)
    return fail(BSGP_ERR_ARG, "the plan holds one PSF per image: B must equal its PSF count");
  DEVICE_SCOPE(p->device);
  rc = ensure_ws(p, (size_t)B);
  if (rc) return rc;
  const int T = rs ? rs->T : choose_team(p, B, prm->team);
  rc = ensure_team(p, (size_t)B, T);
  if (rc) return rc;
  SolveArgs a;
  a.g = p->g;
  a.prm = *prm;
  if (rs) {
    // no inputs: the records hold what the iterations read.  The kernels read
    // in.beta0 in the setup only; the launchers ask whether it was given
    // (ls_mode), so a resumed solve of per-image betas points it at the state.
    a.in = bsgp_inputs{};
    if (rs->beta0_given) a.in.beta0 = reinterpret_cast<const double*>(p->st);
  } else {
    a.in = *in;
  }
  a.out = *out;
  a.B = B;
  a.img0 = 0;
  a.nimg = B;
  a.st = p->st;
  a.active = p->active;
  a.ws = p->ws;
  a.slot_stride = p->slot_stride;
  a.vec_stride = p->vec_stride;
  a.lds_fft_bytes = p->lds_fft_bytes;
  a.T = T;
  // k_col has no team reduction, so a team image may spread its columns over
  // more workgroups than the team has (C4: 1025 columns, 256-member team)
  a.Tc = T;
  if (T > 1) {
    // (one-group cooperative columns pair column 0 with the Nyquist column)
    const int ncol = (p->g.coop && p->g.nfc == 1 && p->g.Q % 2 == 0)
                         ? p->g.Qh - 1
                         : p->g.Qh;
    const int nc = (ncol + p->g.nfc - 1) / p->g.nfc;
    const int want = 4 * p->ncu / B;
    a.Tc = std::max(T, std::min(nc, want));
  }
  // one-workgroup images run AT's column pass at the end of k_ls (bit 1);
  // teams launch k_col for it
  a.fuse_col = T == 1 ? 2 : 0;
  a.static_geo = 0;
  a.tpart = T > 1 ? p->tpart : nullptr;
  a.tctr = p->tctr;
  a.tfail = reinterpret_cast<int*>(p->tctr + (size_t)B * kTeamWords);
  a.plist = nullptr;
  a.plist_stride = 0;
  a.lcap = 0;
  a.list_lds = 0;
  a.pw = p->pw;
  a.storage = p->storage;
  a.spec_off = p->spec_off;
  a.spec2 = nullptr;
  a.spec2_stride = 0;
  a.spin_limit = (unsigned)env_knob("BSGP_SPIN_LIMIT", 1ll << 26, 0, 0xffffffffll);
  a.ls_predict = (int)env_knob("BSGP_LS_PREDICT", 1, 0, 5);
  a.ls_cap = (prm->beta > 0.0 && prm->beta < 1.0)
                 ? (int)std::ceil(std::log(1e-12) / std::log(prm->beta)) + 2
                 : 4096;
  if (prm->proj_cache && prm->proj_type == 1) {
    a.lcap = proj_list_cap(p->g, T);
    const size_t half = round_up((size_t)a.lcap * T * plan_block(p->g), 32);
    a.plist_stride = 2 * half;
    rc = ensure_plist(p, (size_t)B * a.plist_stride);
    if (rc) return rc;
    a.plist = p->plist;
    // the projection lists stay in the transform buffers' LDS as far as they
    // fit: teams, and one-workgroup images of per-wave plans (there
    // BSGP_LIST_LDS caps the entries per thread; 0: every entry in global memory)
    const size_t fit = p->lds_fft_bytes / ((size_t)plan_block(p->g) * 2 * sizeof(double));
    if (T > 1) {
      a.list_lds = (int)std::min<size_t>((size_t)a.lcap, fit);
    } else if (!p->g.coop) {
      const size_t cap = (size_t)env_knob("BSGP_LIST_LDS", 1 << 20, 0, 1 << 20);
      a.list_lds = (int)std::min<size_t>(std::min<size_t>((size_t)a.lcap, fit), cap);
    }
  }
  hipStream_t s = (hipStream_t)stream;
  const int K = (prm->adapt_beta && prm->variant == BSGP_VARIANT_BETA)
                    ? 1
                    : (prm->ls_spec <= 1 ? 1 : prm->ls_spec <= 2 ? 2 : prm->ls_spec <= 4 ? 4 : 8);
  // Sub-batches on their own streams (fork/join with the caller's stream):
  // while one sub-batch runs the compute-bound line search the other can
  // stream its memory-bound phases.
  int S = prm->streams < 1 ? 1 : prm->streams;
  if (S > bsgp_plan_s::kMaxStreams) S = bsgp_plan_s::kMaxStreams;
  if (S > B) S = B;
  // per-iteration error / iterate snapshots (errflag, save): one small kernel
  // after setup and after every iteration, off the hot kernels
  const bool track = out->err != nullptr || out->x_iter != nullptr;
  // persistent solver (one launch for every iteration, k_persist): one-workgroup
  // images, with per-wave transforms or (cooperative plans: the application's
  // 375^2 / 450^2 subdivisions) the 512-thread build's thread-group transforms
  // (bsgp_persist_c512.hip); it overlaps the phases of different images itself,
  // so it runs the whole batch as one sub-batch
  // (a resumed slot-order solve needs every image at the same iteration; records
  // that are not take the phase kernels, which are bit-identical)
  const bool ring_rule = prm->stop_criterion >= 2 && prm->stop_criterion <= 4;
  const bool persist =
      prm->persistent && T == 1 && !track && (!rs || ring_rule || rs->uniform);
  if (persist) S = 1;
  // the speculative fused pass of the persistent line search writes w's rows
  // to a second spectrum per image; without one the kernel never speculates
  if (persist && persist_speculates(a)) {
    rc = ensure_spec2(p, (size_t)B);
    if (rc) return rc;
    a.spec2 = p->spec2;
    a.spec2_stride = spec2_stride(p);
  }
  // the flagship plan's compile-time-geometry phases (k_persist): this solve's
  // choice (bsgp_plan_set_static_geo, else BSGP_STATIC_GEO, default on), taken
  // only when the kernel launched carries them and every plan value they fold
  // equals the plan's own
  {
    const int want = static_geo_choice >= 0 ? static_geo_choice
                                            : (int)env_knob("BSGP_STATIC_GEO", 1, 0, 1);
    a.static_geo = (want && persist && persist_static_geo(a, K)) ? 1 : 0;
    p->last_static_geo = a.static_geo;
  }
  // fixed-length persistent solves run every image's setup as the first task
  // of its chain inside k_persist: the setups of the last images overlap the
  // first iterations of the others, with no k_setup launch and no boundary
  // (BSGP_FOLD_SETUP=0: k_setup first, for A/B)
  const bool ring = prm->stop_criterion >= 2 && prm->stop_criterion <= 4;
  a.fold_setup = (persist && !ring && !rs && env_knob("BSGP_FOLD_SETUP", 1, 0, 1)) ? 1 : 0;
  // sub-batch 0 runs on the caller's stream itself, sub-batches 1..S-1 on the
  // plan's streams: S streams in all, so S = 4 fits the 4 hardware queues HIP
  // opens per process (GPU_MAX_HW_QUEUES)
  if (S > 1 && p->nsub < S) {
    if (!p->ev_fork) HIP_TRY(hipEventCreateWithFlags(&p->ev_fork, hipEventDisableTiming));
    for (int i = (p->nsub > 1 ? p->nsub : 1); i < S; ++i) {
      HIP_TRY(hipStreamCreateWithFlags(&p->sub[i], hipStreamNonBlocking));
      HIP_TRY(hipEventCreateWithFlags(&p->ev_join[i], hipEventDisableTiming));
    }
    p->nsub = S;
  }
  // device counter of images not yet stopped: B, counted down by every image
  // the setup or k_bb stops (count_stopped); the last one writes this solve's
  // seq to the host-mapped word
  // (resumed: 0, counted up by k_state_load for every image that goes on)
  HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)p->active, rs ? 0 : B, 1, s));
  a.seq = g_solve_seq.fetch_add(1, std::memory_order_relaxed) + 1;
  p->seq = a.seq;
  a.done_host = p->done_d;
  // team barrier counters and the timeout word restart at 0 every solve
  HIP_TRY(hipMemsetAsync(p->tctr, 0, p->tctr_bytes, s));
  // flag barriers: every partial slot starts empty
  if (T > 1 && (T <= kTeamFlags || T >= 8))
    HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)p->tpart, kPartEmptyWord,
                              B * kPartBufs * (size_t)(T + 8) * kMaxRed * 2, s));
  p->last_valid = true;
  p->last_prm = *prm;
  p->last_out = *out;
  p->last_B = B;
  p->last_T = T;
  p->last_beta0 = a.in.beta0 != nullptr;
  StateArgs ld{};
  if (rs) {
    ld = rs->sa;
    ld.ws = p->ws;
    ld.slot_stride = p->slot_stride;
    ld.vec_stride = p->vec_stride;
    ld.st = p->st;
    ld.T = T;
    ld.M1 = prm->MAXIT + 1;
    ld.out = *out;
    ld.prm = *prm;
    ld.active = p->active;
    HIP_TRY(launch_state_load(ld, B, s));
    if (!(persist && !ring))
      HIP_TRY(launch_state_post(ld, B, nullptr, nullptr, 0, p->done_d, a.seq, s));
  }
  hipStream_t ss[bsgp_plan_s::kMaxStreams];
  SolveArgs sa[bsgp_plan_s::kMaxStreams];
  if (S > 1) HIP_TRY(hipEventRecord(p->ev_fork, s));
  for (int j = 0; j < S; ++j) {
    ss[j] = j > 0 ? p->sub[j] : s;
    if (j > 0) HIP_TRY(hipStreamWaitEvent(ss[j], p->ev_fork, 0));
    sa[j] = a;
    sa[j].img0 = (int)((int64_t)B * j / S);
    sa[j].nimg = (int)((int64_t)B * (j + 1) / S) - sa[j].img0;
    if (prof) HIP_TRY(hipEventRecord(prof->ev[0], ss[j]));
    if (!a.fold_setup && !rs) HIP_TRY(launch_setup(sa[j], p->lds_bytes, ss[j]));
    if (prof) HIP_TRY(hipEventRecord(prof->ev[1], ss[j]));
    if (track) HIP_TRY(launch_track(sa[j], 0, ss[j]));
  }
  if (persist) {
    const size_t need = (size_t)2 * B + 4;  // head, tail, pad, ready ring[B] (64-bit entries)
    if (need > p->pq_n) {
      if (p->pq) HIP_TRY(hipFree(p->pq));
      p->pq = nullptr;
      p->pq_n = 0;
      HIP_TRY(hipMalloc(&p->pq, need * sizeof(unsigned)));
      p->pq_n = need;
    }
    HIP_TRY(hipMemsetAsync(p->pq, 0, need * sizeof(unsigned), s));
    if (rs && !ring)  // slot order: the queue starts at the records' iteration
      HIP_TRY(launch_state_post(ld, B, p->pq, p->pq + 1, rs->done_it, p->done_d, a.seq, s));
    int per_cu = 0;
    HIP_TRY(persist_resident_per_cu(sa[0], K, p->lds_bytes, &per_cu));
    if (per_cu < 1) return fail(BSGP_ERR_HIP, "persistent solver does not fit a CU");
    // every workgroup resident at once (a dequeued task's predecessor is always
    // running or done); no more workgroups than images
    const int grid = (int)std::min<long>(B, (long)p->ncu * per_cu);
    if (prof) HIP_TRY(hipEventRecord(prof->ev[2], s));
    HIP_TRY(launch_persist(sa[0], K, p->lds_bytes, s, p->pq, p->pq + 1, grid));
    if (prof) {
      HIP_TRY(hipEventRecord(prof->ev[3], s));
      HIP_TRY(hipStreamSynchronize(s));
      for (int k = 0; k < 6; ++k) {
        prof->kernel_ms[k] = 0.0;
        prof->launches[k] = 0;
      }
      float ms = 0.f;
      HIP_TRY(hipEventElapsedTime(&ms, prof->ev[0], prof->ev[1]));
      // (a folded setup runs inside k_persist: no k_setup launch)
      prof->kernel_ms[0] = a.fold_setup ? 0.0 : ms;
      prof->launches[0] = a.fold_setup ? 0 : 1;
      HIP_TRY(hipEventElapsedTime(&ms, prof->ev[2], prof->ev[3]));
      prof->kernel_ms[5] = ms;
      prof->launches[5] = 1;
    }
    return BSGP_OK;
  }
  // Fixed-length runs (stop_criterion 0/1) are launched back to back with no
  // host synchronisation.  Data-dependent stop rules are polled with
  // lookahead: the host keeps at most kLook iterations queued ahead of the
  // device (it waits for the event after iteration it - kLook, never for the
  // stream to drain) and stops enqueueing once the host-mapped word carries
  // this solve's seq, i.e. every image has stopped; the iterations queued
  // past the last stop find every image stopped and return at once.  (Draining
  // the stream after every iteration, as round 4 did, is one host round trip
  // per iteration on the latency-bound single-image solves: measured and
  // removed.)
  const bool data_stop = prm->stop_criterion >= 2 && prm->stop_criterion <= 4;
  constexpr int kLook = 2;
  if (data_stop)
    for (int i = 0; i < bsgp_plan_s::kPollRing; ++i)
      if (!p->ev_it[i]) HIP_TRY(hipEventCreateWithFlags(&p->ev_it[i], hipEventDisableTiming));
  int it_run = 0;
  const int it0 = rs ? rs->it0 : 1;
  for (int it = it0; it <= prm->MAXIT; ++it) {
    it_run = it;
    for (int j = 0; j < S; ++j) {
      HIP_TRY(launch_iteration(sa[j], K, p->lds_bytes, ss[j],
                               prof ? &prof->ev[2 + 6 * (size_t)(it - 1)] : nullptr));
      if (track) HIP_TRY(launch_track(sa[j], it, ss[j]));
    }
    if (data_stop && it < prm->MAXIT) {
      HIP_TRY(hipEventRecord(p->ev_it[it % bsgp_plan_s::kPollRing], ss[0]));
      if (it - it0 >= kLook) {
        HIP_TRY(hipEventSynchronize(p->ev_it[(it - kLook) % bsgp_plan_s::kPollRing]));
        if (__atomic_load_n(p->done_h, __ATOMIC_ACQUIRE) == a.seq) break;
      }
    }
  }
  if (S > 1) {
    for (int j = 1; j < S; ++j) {
      HIP_TRY(hipEventRecord(p->ev_join[j], ss[j]));
      HIP_TRY(hipStreamWaitEvent(s, p->ev_join[j], 0));
    }
  }
  if (prof) {
    // kernel classes: 0 setup, 1 dir, 2 col (A and AT launches), 3 ls, 4 bb
    HIP_TRY(hipStreamSynchronize(s));
    for (int k = 0; k < 6; ++k) {
      prof->kernel_ms[k] = 0.0;
      prof->launches[k] = 0;
    }
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, prof->ev[0], prof->ev[1]));
    prof->kernel_ms[0] = ms;
    prof->launches[0] = 1;
    const int cls[5] = {1, 2, 3, 2, 4};
    const bool launched[5] = {true, true, true, !(sa[0].fuse_col & 2), true};
    for (int it = 0; it < it_run; ++it) {
      hipEvent_t* e = &prof->ev[2 + 6 * (size_t)it];
      for (int k = 0; k < 5; ++k) {
        HIP_TRY(hipEventElapsedTime(&ms, e[k], e[k + 1]));
        prof->kernel_ms[cls[k]] += ms;
        if (launched[k]) prof->launches[cls[k]] += 1;
      }
    }
  }
  return BSGP_OK;
}

int bsgp_solve_host(bsgp_plan p, int32_t B, const bsgp_params* prm, const bsgp_inputs* in,
                    const bsgp_outputs* out) {
  if (!p) return fail(BSGP_ERR_ARG, "plan is NULL");
  int rc = check_params(prm);
  if (rc) return rc;
  if (B < 1 || !in || !in->gn || !in->bkg || !out || !out->x || !out->iters || !out->discr)
    return fail(BSGP_ERR_ARG, "bad arguments");
  DEVICE_SCOPE(p->device);
  const size_t N = (size_t)p->g.H * p->g.W, M1 = (size_t)prm->MAXIT + 1;
  std::vector<void*> bufs;
  auto dalloc = [&](size_t bytes) -> void* {
    void* d = nullptr;
    if (hipMalloc(&d, bytes ? bytes : 8) != hipSuccess) return nullptr;
    bufs.push_back(d);
    return d;
  };
  auto cleanup = [&]() {
    for (void* b : bufs) (void)hipFree(b);
  };
  bsgp_inputs di{};
  bsgp_outputs dout{};
  const size_t nb = prm->bkg_is_map ? B * N : (size_t)B;
  di.gn = (const double*)dalloc(B * N * 8);
  di.bkg = (const double*)dalloc(nb * 8);
  if (in->flux) di.flux = (const double*)dalloc(B * 8);
  if (in->x0) di.x0 = (const double*)dalloc(B * N * 8);
  if (in->beta0) di.beta0 = (const double*)dalloc(B * 8);
  if (in->obj) di.obj = (const double*)dalloc(B * N * 8);
  dout.x = (double*)dalloc(B * N * 8);
  dout.iters = (int32_t*)dalloc(B * 4);
  dout.discr = (double*)dalloc(B * M1 * 8);
  if (out->times) dout.times = (double*)dalloc(B * M1 * 8);
  if (out->crit) dout.crit = (double*)dalloc(B * M1 * 8);
  if (out->flags) dout.flags = (int32_t*)dalloc(B * M1 * 4);
  if (out->beta_final) dout.beta_final = (double*)dalloc(B * 8);
  if (out->counters) dout.counters = (int64_t*)dalloc(B * 8 * 8);
  if (out->err) dout.err = (double*)dalloc(B * M1 * 8);
  if (out->x_iter) dout.x_iter = (double*)dalloc(B * (M1 - 1) * N * 8);
  for (void* b : bufs)
    if (!b) {
      cleanup();
      return fail(BSGP_ERR_HIP, "device allocation failed");
    }
  auto h2d = [&](const void* d, const void* h, size_t bytes) {
    return hipMemcpy(const_cast<void*>(d), h, bytes, hipMemcpyHostToDevice) == hipSuccess;
  };
  bool ok = h2d(di.gn, in->gn, B * N * 8) && h2d(di.bkg, in->bkg, nb * 8) &&
            (!in->flux || h2d(di.flux, in->flux, B * 8)) &&
            (!in->x0 || h2d(di.x0, in->x0, B * N * 8)) &&
            (!in->beta0 || h2d(di.beta0, in->beta0, B * 8)) &&
            (!in->obj || h2d(di.obj, in->obj, B * N * 8));
  if (!ok) {
    cleanup();
    return fail(BSGP_ERR_HIP, "host to device copy failed");
  }
  rc = bsgp_solve_device(p, B, prm, &di, &dout, nullptr);
  if (rc) {
    std::string m = g_err;
    cleanup();
    return fail(rc, m);
  }
  auto d2h = [&](void* h, const void* d, size_t bytes) {
    return !h || hipMemcpy(h, d, bytes, hipMemcpyDeviceToHost) == hipSuccess;
  };
  ok = hipDeviceSynchronize() == hipSuccess && d2h(out->x, dout.x, B * N * 8) &&
       d2h(out->iters, dout.iters, B * 4) && d2h(out->discr, dout.discr, B * M1 * 8) &&
       (!out->times || d2h(out->times, dout.times, B * M1 * 8)) &&
       (!out->crit || d2h(out->crit, dout.crit, B * M1 * 8)) &&
       (!out->flags || d2h(out->flags, dout.flags, B * M1 * 4)) &&
       (!out->beta_final || d2h(out->beta_final, dout.beta_final, B * 8)) &&
       (!out->counters || d2h(out->counters, dout.counters, B * 64)) &&
       (!out->err || d2h(out->err, dout.err, B * M1 * 8)) &&
       (!out->x_iter || d2h(out->x_iter, dout.x_iter, B * (M1 - 1) * N * 8));
  cleanup();
  if (!ok) return fail(BSGP_ERR_HIP, "solve or device to host copy failed");
  return BSGP_OK;
}

// ---- solver state: save / resume (kernels in bsgp_state.hip) ---------------

int bsgp_state_layout(int32_t H, int32_t W, int32_t storage, int32_t bkg_is_map,
                      int32_t hist_cap, int64_t* offs) {
  if (!offs) return fail(BSGP_ERR_ARG, "offs is NULL");
  if (H < 1 || W < 1 || hist_cap < 1) return fail(BSGP_ERR_ARG, "bad shape or hist_cap");
  if (storage != BSGP_STORAGE_F64 && storage != BSGP_STORAGE_F32)
    return fail(BSGP_ERR_ARG, "bad storage");
  const StateLayout L = state_layout((size_t)H * W, storage, bkg_is_map != 0, hist_cap);
  const size_t v[11] = {L.bytes, L.discr, L.crit, L.times, L.flags, L.x,
                        L.g,     L.xtf,   L.pw,   L.gn,    L.bkg};
  for (int i = 0; i < 11; ++i) offs[i] = (int64_t)v[i];
  return BSGP_OK;
}

int bsgp_state_bytes(bsgp_plan p, int32_t bkg_is_map, int32_t MAXIT_done_max,
                     int64_t* bytes_per_image) {
  if (!p) return fail(BSGP_ERR_ARG, "plan is NULL");
  if (!bytes_per_image || MAXIT_done_max < 0) return fail(BSGP_ERR_ARG, "bad arguments");
  *bytes_per_image = (int64_t)state_layout((size_t)p->g.H * p->g.W, p->storage, bkg_is_map != 0,
                                           MAXIT_done_max + 1)
                         .bytes;
  return BSGP_OK;
}

int bsgp_state_save(bsgp_plan p, int32_t B, void* state_dev, int64_t bytes_per_image,
                    void* stream) {
  if (!p) return fail(BSGP_ERR_ARG, "plan is NULL");
  if (!state_dev) return fail(BSGP_ERR_ARG, "state_dev is NULL");
  if (!p->last_valid) return fail(BSGP_ERR_ARG, "no solve has run on this plan");
  if (B != p->last_B || B > 65535)
    return fail(BSGP_ERR_ARG, "B must be the last solve's batch size (at most 65535)");
  const bsgp_params& q = p->last_prm;
  if (q.stop_criterion == 2 && !p->last_out.crit)
    return fail(BSGP_ERR_ARG, "saving a stop_criterion 2 solve needs its out->crit");
  StateArgs a{};
  a.N = p->g.H * p->g.W;
  a.H = p->g.H;
  a.W = p->g.W;
  a.storage = p->storage;
  a.conv_mode = p->conv_mode;
  a.bmap = q.bkg_is_map != 0;
  a.hist_cap = q.MAXIT + 1;
  a.L = state_layout((size_t)a.N, a.storage, a.bmap != 0, a.hist_cap);
  if ((int64_t)a.L.bytes != bytes_per_image)
    return fail(BSGP_ERR_ARG, "bytes_per_image is not bsgp_state_bytes(plan, bkg_is_map, MAXIT)");
  a.rec = static_cast<unsigned char*>(state_dev);
  a.rec_bytes = a.L.bytes;
  a.ws = p->ws;
  a.slot_stride = p->slot_stride;
  a.vec_stride = p->vec_stride;
  a.st = p->st;
  a.T = p->last_T;
  a.beta0_given = p->last_beta0;
  a.M1 = q.MAXIT + 1;
  a.out = p->last_out;
  a.prm = q;
  DEVICE_SCOPE(p->device);
  HIP_TRY(launch_state_save(a, B, (hipStream_t)stream));
  return BSGP_OK;
}

int bsgp_solve_resume(bsgp_plan p, int32_t B, const bsgp_params* prm, const void* state_dev,
                      int32_t n_state, int64_t bytes_per_image, const int32_t* index,
                      const bsgp_outputs* out, void* stream) {
  if (!p) return fail(BSGP_ERR_ARG, "plan is NULL");
  StaticGeoCall sgc(p);
  int rc = check_params(prm);
  if (rc) return rc;
  if (!state_dev || n_state < 1) return fail(BSGP_ERR_ARG, "state_dev missing");
  if (B < 1 || B > 65535 || (!index && B > n_state))
    return fail(BSGP_ERR_ARG, "B must be in [1, 65535] and, without an index, at most n_state");
  if (!out || !out->x || !out->iters || !out->discr) return fail(BSGP_ERR_ARG, "outputs missing");
  if (out->err || out->x_iter)
    return fail(BSGP_ERR_UNSUPPORTED, "err / x_iter are not available on a resumed solve");
  if (p->n_tf > 1 && B != p->n_tf)
    return fail(BSGP_ERR_ARG, "the plan holds one PSF per image: B must equal its PSF count");
  if (bytes_per_image < BSGP_STATE_HEADER_BYTES || bytes_per_image % 16)
    return fail(BSGP_ERR_ARG, "bad bytes_per_image");
  DEVICE_SCOPE(p->device);
  hipStream_t s = (hipStream_t)stream;
  // the headers (and the index) on the host, for validation
  std::vector<bsgp_state_header> hs((size_t)n_state);
  std::vector<int32_t> idx((size_t)B);
  HIP_TRY(hipMemcpy2DAsync(hs.data(), sizeof(bsgp_state_header), state_dev,
                           (size_t)bytes_per_image, sizeof(bsgp_state_header), (size_t)n_state,
                           hipMemcpyDeviceToHost, s));
  if (index)
    HIP_TRY(hipMemcpyAsync(idx.data(), index, (size_t)B * sizeof(int32_t), hipMemcpyDeviceToHost,
                           s));
  HIP_TRY(hipStreamSynchronize(s));
  if (!index)
    for (int i = 0; i < B; ++i) idx[i] = i;
  const size_t N = (size_t)p->g.H * p->g.W;
  ResumeCtx rs{};
  int min_done = -1, max_done = -1;
  char msg[200];
  for (int i = 0; i < B; ++i) {
    if (idx[i] < 0 || idx[i] >= n_state) {
      snprintf(msg, sizeof msg, "index[%d] = %d is outside the %d records", i, idx[i], n_state);
      return fail(BSGP_ERR_ARG, msg);
    }
    const bsgp_state_header& h = hs[(size_t)idx[i]];
    const bsgp_params& q = h.prm;
    const char* bad = nullptr;
    auto same = [](const void* a, const void* b, size_t n) { return memcmp(a, b, n) == 0; };
#define BSGP_SAME(f) \
  if (!bad && !same(&q.f, &prm->f, sizeof q.f)) bad = #f
    if (h.magic != BSGP_STATE_MAGIC) bad = "magic";
    if (!bad && h.version != BSGP_STATE_VERSION) bad = "version";
    if (!bad && (h.H != p->g.H || h.W != p->g.W)) bad = "shape (H, W)";
    if (!bad && h.storage != p->storage) bad = "storage";
    if (!bad && h.conv_mode != p->conv_mode) bad = "conv_mode";
    BSGP_SAME(variant);
    BSGP_SAME(init_recon);
    BSGP_SAME(proj_type);
    BSGP_SAME(stop_criterion);
    BSGP_SAME(M_alpha);
    BSGP_SAME(M);
    BSGP_SAME(max_projs);
    BSGP_SAME(gamma);
    BSGP_SAME(beta);
    BSGP_SAME(alpha);
    BSGP_SAME(alpha_min);
    BSGP_SAME(alpha_max);
    BSGP_SAME(tau);
    BSGP_SAME(ccd_sat_level);
    BSGP_SAME(betaParam);
    BSGP_SAME(lr);
    BSGP_SAME(lr_exp_param);
    BSGP_SAME(tol_convergence);
    BSGP_SAME(prescaled_scaling);
    BSGP_SAME(prescaled_tol4);
    BSGP_SAME(has_sat);
    BSGP_SAME(scale_data);
    BSGP_SAME(verbose);
    BSGP_SAME(adapt_beta);
    BSGP_SAME(schedule_lr);
    BSGP_SAME(bkg_is_map);
    BSGP_SAME(ls_series);
    BSGP_SAME(gn_compact);
    BSGP_SAME(gn_f32);
    BSGP_SAME(beta0_general);
    BSGP_SAME(flux_f32);
#undef BSGP_SAME
    if (!bad && (h.hist_cap < 1 || h.iters_done < 0 || h.iters_done >= h.hist_cap ||
                 h.record_bytes != bytes_per_image ||
                 (int64_t)state_layout(N, p->storage, q.bkg_is_map != 0, h.hist_cap).bytes !=
                     bytes_per_image))
      bad = "record_bytes / hist_cap";
    if (!bad && i > 0 && (h.hist_cap != rs.sa.hist_cap || h.T != rs.T ||
                          h.beta0_given != rs.beta0_given))
      bad = "hist_cap / T / beta0_given (records of different solves)";
    if (!bad && h.T < 1) bad = "T";
    if (bad) {
      snprintf(msg, sizeof msg, "state record %d does not match the plan / parameters: %s",
               idx[i], bad);
      return fail(BSGP_ERR_ARG, msg);
    }
    if (prm->MAXIT <= h.iters_done) {
      snprintf(msg, sizeof msg, "MAXIT = %d must exceed the %d iterations record %d has done",
               prm->MAXIT, h.iters_done, idx[i]);
      return fail(BSGP_ERR_ARG, msg);
    }
    if (i == 0) {
      rs.sa.hist_cap = h.hist_cap;
      rs.T = h.T;
      rs.beta0_given = h.beta0_given;
    }
    if (!h.stopped) {
      min_done = min_done < 0 ? h.iters_done : std::min(min_done, h.iters_done);
      max_done = std::max(max_done, h.iters_done);
    }
  }
  // the team size decides the order of every sum: it must be the records'
  const int Tres = choose_team(p, B, prm->team == 0 ? rs.T : prm->team);
  if (Tres != rs.T) {
    snprintf(msg, sizeof msg,
             "team: the records were solved with %d workgroups per image, this resume would "
             "run %d",
             rs.T, Tres);
    return fail(BSGP_ERR_ARG, msg);
  }
  if (min_done < 0) min_done = max_done = prm->MAXIT;  // every record is stopped: nothing runs
  rs.it0 = min_done + 1;
  rs.uniform = min_done == max_done;
  rs.done_it = min_done;
  StateArgs& a = rs.sa;
  a.rec = static_cast<unsigned char*>(const_cast<void*>(state_dev));
  a.rec_bytes = (size_t)bytes_per_image;
  a.index = index;
  a.N = (int)N;
  a.H = p->g.H;
  a.W = p->g.W;
  a.storage = p->storage;
  a.conv_mode = p->conv_mode;
  a.bmap = prm->bkg_is_map != 0;
  a.L = state_layout(N, p->storage, a.bmap != 0, a.hist_cap);
  a.beta0_given = rs.beta0_given;
  return solve_impl(p, B, prm, nullptr, out, stream, nullptr, &rs);
}

int bsgp_apply_operator(bsgp_plan p, int32_t B, int32_t transpose, const double* x, double* out,
                        void* stream) {
  if (!p || !x || !out || B < 1) return fail(BSGP_ERR_ARG, "bad arguments");
  if (p->n_tf > 1 && B != p->n_tf)
    return fail(BSGP_ERR_ARG, "the plan holds one PSF per image: B must equal its PSF count");
  DEVICE_SCOPE(p->device);
  const int slots = p->ncu * p->wg_per_cu;
  // few images: spread each over many workgroups (rows, columns, rows), one
  // spectrum per image; many images: one persistent workgroup per image
  const bool split = (size_t)B * 4 <= (size_t)slots;
  const int grid = split ? B : (B < slots ? B : slots);
  const size_t stride = round_up((size_t)p->g.sld * p->g.Qh, 16);
  if ((size_t)grid > p->opws_slots) {
    if (p->opws) HIP_TRY(hipFree(p->opws));
    p->opws = nullptr;
    p->opws_slots = 0;
    HIP_TRY(hipMalloc(&p->opws, (size_t)grid * stride * sizeof(cd)));
    p->opws_slots = grid;
  }
  if (split)
    HIP_TRY(launch_apply_op_split(p->g, B, transpose, x, out, p->opws, stride, slots / B,
                                  p->lds_bytes, (hipStream_t)stream));
  else
    HIP_TRY(launch_apply_op(p->g, B, transpose, x, out, p->opws, stride, grid, p->lds_bytes,
                            (hipStream_t)stream));
  return BSGP_OK;
}

int bsgp_project_df(int64_t n, double b, const double* c, const double* dia, double scaling,
                    int32_t has_sat, double ccd_sat_level, double lambda0, double dlambda0,
                    double tol_lam, int32_t biter, int32_t siter, int32_t max_projs, double* x,
                    double* info, void* stream) {
  if (n < 1 || n > 0x7fffffff || !c || !dia || !x || !info)
    return fail(BSGP_ERR_ARG, "bad arguments");
  ProjClip clip{has_sat != 0, ccd_sat_level / scaling - 2.220446049250313e-16};
  HIP_TRY(launch_project_df((int)n, b, c, dia, clip, lambda0, dlambda0, tol_lam, biter, siter,
                            max_projs, x, info, (hipStream_t)stream));
  return BSGP_OK;
}

int bsgp_extract_tiles(const double* img, int32_t H, int32_t W, const int32_t* boxes, int32_t n,
                       int32_t th, int32_t tw, double* out, void* stream) {
  if (!img || !boxes || !out || H < 1 || W < 1 || n < 1 || th < 1 || tw < 1 || th > H || tw > W)
    return fail(BSGP_ERR_ARG, "bad arguments");
  if ((int64_t)n * th > 0x7fffffff) return fail(BSGP_ERR_ARG, "too many tile rows");
  HIP_TRY(launch_extract_tiles(img, W, boxes, n, th, tw, out, (hipStream_t)stream));
  return BSGP_OK;
}

int bsgp_coadd_tiles(const double* tiles, int32_t n, int32_t th, int32_t tw, const int32_t* boxes,
                     int32_t H, int32_t W, double* mean, double* footprint, void* stream) {
  if (!tiles || !boxes || !mean || H < 1 || W < 1 || n < 1 || n > 8192 || th < 1 || tw < 1)
    return fail(BSGP_ERR_ARG, "bad arguments");
  HIP_TRY(launch_coadd_tiles(tiles, n, th, tw, boxes, H, W, mean, footprint, (hipStream_t)stream));
  return BSGP_OK;
}

int bsgp_fits_to_f64(const void* raw, int64_t n, int32_t bitpix, double bscale, double bzero,
                     double* out, void* stream) {
  if (!raw || !out || n < 0) return fail(BSGP_ERR_ARG, "bad arguments");
  if (bitpix != 8 && bitpix != 16 && bitpix != 32 && bitpix != 64 && bitpix != -32 &&
      bitpix != -64)
    return fail(BSGP_ERR_ARG, "BITPIX must be 8, 16, 32, 64, -32 or -64");
  if (n == 0) return BSGP_OK;
  HIP_TRY(launch_fits_to_f64(raw, n, bitpix, bscale, bzero, out, (hipStream_t)stream));
  return BSGP_OK;
}

int bsgp_psf_stamps(const bsgp_psf_model* m, const double* xy, int32_t n, int32_t spatial,
                    int32_t normalize, double* out, void* stream) {
  if (!m || !out || n < 0 || (spatial && !xy) || !m->coeffs)
    return fail(BSGP_ERR_ARG, "bad arguments");
  if (m->hw < 0 || m->hw > 255 || m->ngauss < 1 || m->ldeg < 0 || m->sdeg < 0)
    return fail(BSGP_ERR_ARG, "bad PSF model degrees or half width");
  PsfModel M{};
  M.ncomp = m->ngauss * (m->ldeg + 1) * (m->ldeg + 2) / 2;
  const int nterm = (m->sdeg + 1) * (m->sdeg + 2) / 2;
  const int need = spatial ? M.ncomp * nterm : M.ncomp;
  if (M.ncomp > kPsfMaxLocal || need > kPsfMaxCoef)
    return fail(BSGP_ERR_ARG, "PSF model has too many coefficients");
  if (m->ncoef < need) return fail(BSGP_ERR_ARG, "too few PSF coefficients for the degrees");
  if (n == 0) return BSGP_OK;
  M.cosv = m->cos;
  M.sinv = m->sin;
  M.ax = m->ax;
  M.ay = m->ay;
  M.sig2 = m->sigma_inc * m->sigma_inc;
  M.x_orig = m->x_orig;
  M.y_orig = m->y_orig;
  M.ngauss = m->ngauss;
  M.ldeg = m->ldeg;
  M.sdeg = m->sdeg;
  M.hw = m->hw;
  M.ncoef = need;
  for (int i = 0; i < need; ++i) M.coef[i] = m->coeffs[i];
  HIP_TRY(launch_psf_stamps(M, xy, n, spatial ? 1 : 0, normalize ? 1 : 0, out,
                            (hipStream_t)stream));
  return BSGP_OK;
}

int bsgp_background2d(const void* data, int32_t dtype, int32_t B, int32_t H, int32_t W, int32_t bh,
                      int32_t bw, int32_t fh, int32_t fw, double sigma, int32_t maxiters,
                      double exclude_percentile, int32_t clip, const uint8_t* mask, double* bkg_out,
                      double* rms_out, double* mesh_out, double* rms_mesh_out, double* medians_out,
                      int32_t* status_out, void* stream) {
  if (!data) return fail(BSGP_ERR_ARG, "data is NULL");
  if (dtype != BSGP_DTYPE_F32 && dtype != BSGP_DTYPE_F64)
    return fail(BSGP_ERR_ARG, "dtype must be BSGP_DTYPE_F32 or BSGP_DTYPE_F64");
  if (B < 1 || H < 1 || W < 1) return fail(BSGP_ERR_ARG, "B, H and W must be >= 1");
  if (bh < 1 || bw < 1) return fail(BSGP_ERR_ARG, "box size (bh, bw) must be >= 1");
  if (fh < 1 || fw < 1 || fh % 2 == 0 || fw % 2 == 0)
    return fail(BSGP_ERR_ARG, "filter size (fh, fw) must be odd and >= 1");
  if (!(sigma >= 0.0)) return fail(BSGP_ERR_ARG, "sigma must be >= 0");
  if (maxiters < 0) return fail(BSGP_ERR_ARG, "maxiters must be >= 0");
  if (!(exclude_percentile >= 0.0 && exclude_percentile <= 100.0))
    return fail(BSGP_ERR_ARG, "exclude_percentile must be in [0, 100]");
  char msg[192];
  if ((int64_t)bh * bw > kBkgMaxBox) {
    snprintf(msg, sizeof msg, "box of %lld pixels: a box holds at most %d (bh * bw <= %d)",
             (long long)bh * bw, kBkgMaxBox, kBkgMaxBox);
    return fail(BSGP_ERR_UNSUPPORTED, msg);
  }
  if (fh > kBkgMaxFilter || fw > kBkgMaxFilter) {
    snprintf(msg, sizeof msg, "filter window larger than %d x %d", kBkgMaxFilter, kBkgMaxFilter);
    return fail(BSGP_ERR_UNSUPPORTED, msg);
  }
  const int64_t ny = (H + (int64_t)bh - 1) / bh, nx = (W + (int64_t)bw - 1) / bw;
  if (ny * nx > kBkgMaxCells) {
    snprintf(msg, sizeof msg, "mesh of %lld cells: an image's mesh holds at most %d",
             (long long)(ny * nx), kBkgMaxCells);
    return fail(BSGP_ERR_UNSUPPORTED, msg);
  }
  if (B > 65535 || H > 65535)
    return fail(BSGP_ERR_UNSUPPORTED, "B and H must be at most 65535");
  const size_t ncell = (size_t)(ny * nx);
  BkgArgs a{};
  a.data = data;
  a.mask = mask;
  a.B = B, a.H = H, a.W = W, a.bh = bh, a.bw = bw, a.fh = fh, a.fw = fw;
  a.ny = (int)ny, a.nx = (int)nx, a.maxiters = maxiters, a.clip = clip ? 1 : 0;
  a.sigma = sigma;
  a.excl_count = exclude_percentile / 100.0 * (double)(bh * bw);
  a.ws_stride = 6 * ncell + 8;
  a.bkg = bkg_out, a.rms = rms_out, a.mesh = mesh_out, a.rms_mesh = rms_mesh_out;
  a.medians = medians_out, a.status = status_out;
  hipStream_t s = (hipStream_t)stream;
  // stream-ordered workspace: the call stays asynchronous
  const size_t wsb = (size_t)B * a.ws_stride * sizeof(double);
  const size_t wib = (size_t)B * (1 + 3 * ncell) * sizeof(int);
  void* w = nullptr;
  HIP_TRY(hipMallocAsync(&w, wsb + wib, s));
  a.ws = static_cast<double*>(w);
  a.wsi = reinterpret_cast<int*>(static_cast<char*>(w) + wsb);
  hipError_t e = launch_bkg_boxstats(a, dtype == BSGP_DTYPE_F32, s);
  if (e == hipSuccess) e = launch_bkg_mesh(a, s);
  if (e == hipSuccess && (bkg_out || rms_out)) e = launch_bkg_zoom(a, s);
  const hipError_t ef = hipFreeAsync(w, s);
  if (e != hipSuccess) return fail(BSGP_ERR_HIP, std::string("background launch: ") + hipGetErrorString(e));
  HIP_TRY(ef);
  return BSGP_OK;
}

namespace {
// shape checks shared by the segmentation entry points
int seg_shape(int32_t B, int32_t H, int32_t W) {
  if (B < 1 || H < 1 || W < 1) return fail(BSGP_ERR_ARG, "B, H and W must be >= 1");
  if ((int64_t)H * W > 0x7fffffffLL)
    return fail(BSGP_ERR_UNSUPPORTED, "an image holds fewer than 2^31 pixels (H * W < 2^31)");
  if (B > 65535) return fail(BSGP_ERR_UNSUPPORTED, "B must be at most 65535");
  return BSGP_OK;
}
}  // namespace

int bsgp_convolve2d(const void* data, int32_t dtype, int32_t B, int32_t H, int32_t W,
                    const double* kernel, int32_t kh, int32_t kw, double* out, void* stream) {
  if (!data) return fail(BSGP_ERR_ARG, "data is NULL");
  if (!kernel) return fail(BSGP_ERR_ARG, "kernel is NULL");
  if (!out) return fail(BSGP_ERR_ARG, "out is NULL");
  if (dtype != BSGP_DTYPE_F32 && dtype != BSGP_DTYPE_F64)
    return fail(BSGP_ERR_ARG, "dtype must be BSGP_DTYPE_F32 or BSGP_DTYPE_F64");
  if (kh < 1 || kw < 1) return fail(BSGP_ERR_ARG, "kernel size (kh, kw) must be >= 1");
  if (int rc = seg_shape(B, H, W)) return rc;
  if (kh % 2 == 0 || kw % 2 == 0 || kh > kSegMaxKernel || kw > kSegMaxKernel) {
    char msg[128];
    snprintf(msg, sizeof msg, "kernel of %d x %d: kernels are odd and at most %d x %d", kh, kw,
             kSegMaxKernel, kSegMaxKernel);
    return fail(BSGP_ERR_UNSUPPORTED, msg);
  }
  if (H > 65535) return fail(BSGP_ERR_UNSUPPORTED, "H must be at most 65535");
  SegConvArgs a{};
  a.data = data, a.kernel = kernel, a.out = out;
  a.B = B, a.H = H, a.W = W, a.kh = kh, a.kw = kw;
  HIP_TRY(launch_seg_convolve(a, dtype == BSGP_DTYPE_F32, (hipStream_t)stream));
  return BSGP_OK;
}

int bsgp_detect_sources(const void* data, int32_t dtype, int32_t B, int32_t H, int32_t W,
                        const double* threshold_map, double threshold, int32_t npixels,
                        int32_t connectivity, const uint8_t* mask, int32_t* labels_out,
                        int32_t* nlabels_out, void* stream) {
  if (!data) return fail(BSGP_ERR_ARG, "data is NULL");
  if (!labels_out || !nlabels_out) return fail(BSGP_ERR_ARG, "labels_out / nlabels_out is NULL");
  if (dtype != BSGP_DTYPE_F32 && dtype != BSGP_DTYPE_F64)
    return fail(BSGP_ERR_ARG, "dtype must be BSGP_DTYPE_F32 or BSGP_DTYPE_F64");
  if (npixels < 1) return fail(BSGP_ERR_ARG, "npixels must be >= 1");
  if (connectivity != 4 && connectivity != 8)
    return fail(BSGP_ERR_ARG, "connectivity must be 4 or 8");
  if (int rc = seg_shape(B, H, W)) return rc;
  const size_t hw = (size_t)H * W;
  SegArgs a{};
  a.data = data, a.thr_map = threshold_map, a.mask = mask, a.thr = threshold;
  a.B = B, a.H = H, a.W = W, a.npixels = npixels, a.conn = connectivity;
  a.nblk = (int)((hw + kSegChunk - 1) / kSegChunk);
  a.labels_out = labels_out, a.nlabels_out = nlabels_out;
  hipStream_t s = (hipStream_t)stream;
  // stream-ordered workspace: the call stays asynchronous
  const size_t per = 2 * hw + (size_t)a.nblk;
  void* w = nullptr;
  HIP_TRY(hipMallocAsync(&w, (size_t)B * per * sizeof(int), s));
  a.lab = static_cast<int*>(w);
  a.area = a.lab + (size_t)B * hw;
  a.blk = a.area + (size_t)B * hw;
  const hipError_t e = launch_seg_detect(a, dtype == BSGP_DTYPE_F32, s);
  const hipError_t ef = hipFreeAsync(w, s);
  if (e != hipSuccess) return fail(BSGP_ERR_HIP, std::string("detection launch: ") + hipGetErrorString(e));
  HIP_TRY(ef);
  return BSGP_OK;
}

int bsgp_segment_catalog(const double* data, const double* conv, const int32_t* labels, int32_t B,
                         int32_t H, int32_t W, int32_t cap, const int32_t* nlabels,
                         int32_t* int_cols_out, double* f64_cols_out, int32_t* status_out,
                         void* stream) {
  if (!data) return fail(BSGP_ERR_ARG, "data is NULL");
  if (!labels) return fail(BSGP_ERR_ARG, "labels is NULL");
  if (!int_cols_out || !f64_cols_out || !status_out)
    return fail(BSGP_ERR_ARG, "int_cols_out / f64_cols_out / status_out is NULL");
  if (cap < 1) return fail(BSGP_ERR_ARG, "cap must be >= 1");
  if (int rc = seg_shape(B, H, W)) return rc;
  SegCatArgs a{};
  a.data = data, a.conv = conv, a.labels = labels, a.nlabels = nlabels;
  a.B = B, a.H = H, a.W = W, a.cap = cap;
  a.icols = int_cols_out, a.fcols = f64_cols_out, a.status = status_out;
  HIP_TRY(launch_seg_catalog(a, (hipStream_t)stream));
  return BSGP_OK;
}

int bsgp_segment_local_background(const void* data, int32_t dtype, const int32_t* labels, int32_t B,
                                  int32_t H, int32_t W, int32_t cap, const int32_t* nlabels,
                                  const int32_t* int_cols, double* f64_cols,
                                  double localbkg_width, double sigma, int32_t maxiters,
                                  int32_t min_pixels, int32_t apply, double* lb_out,
                                  int32_t* npix_out, int32_t* status_out, void* stream) {
  if (!(localbkg_width > 0.0) || !std::isfinite(localbkg_width))
    return fail(BSGP_ERR_ARG, "localbkg_width must be finite and > 0");
  if (!(sigma > 0.0)) return fail(BSGP_ERR_ARG, "sigma must be > 0");
  if (maxiters < 0) return fail(BSGP_ERR_ARG, "maxiters must be >= 0");
  if (min_pixels < 1) return fail(BSGP_ERR_ARG, "min_pixels must be >= 1");
  if (dtype != BSGP_DTYPE_F32 && dtype != BSGP_DTYPE_F64)
    return fail(BSGP_ERR_ARG, "dtype must be BSGP_DTYPE_F32 or BSGP_DTYPE_F64");
  if (cap < 1) return fail(BSGP_ERR_ARG, "cap must be >= 1");
  if (B == 0) return BSGP_OK;  // no image: nothing to do, no pointer is followed
  if (!data) return fail(BSGP_ERR_ARG, "data is NULL");
  if (!labels || !int_cols) return fail(BSGP_ERR_ARG, "labels / int_cols is NULL");
  if (apply && !f64_cols) return fail(BSGP_ERR_ARG, "f64_cols is NULL (apply != 0)");
  if (!lb_out || !npix_out || !status_out)
    return fail(BSGP_ERR_ARG, "lb_out / npix_out / status_out is NULL");
  if (int rc = seg_shape(B, H, W)) return rc;
  LocalBkgArgs a{};
  a.data = data, a.labels = labels, a.nlabels = nlabels, a.icols = int_cols, a.fcols = f64_cols;
  a.B = B, a.H = H, a.W = W, a.cap = cap, a.maxiters = maxiters, a.min_pixels = min_pixels;
  a.apply = apply ? 1 : 0, a.width = localbkg_width, a.sigma = sigma;
  a.lb = lb_out, a.npix = npix_out, a.status = status_out;
  hipStream_t s = (hipStream_t)stream;
  const size_t rows = (size_t)B * cap;
  HIP_TRY(hipMemsetAsync(lb_out, 0, rows * sizeof(double), s));
  HIP_TRY(hipMemsetAsync(npix_out, 0, 2 * rows * sizeof(int), s));
  HIP_TRY(hipMemsetAsync(status_out, 0, (size_t)B * sizeof(int), s));
  HIP_TRY(launch_localbkg(a, dtype == BSGP_DTYPE_F32, s));
  return BSGP_OK;
}

// both deblending entry points; lds_max_box < 0: bsgp_deblend_sources (no global-memory path)
static int deblend_sources(const double* data, const int32_t* labels, int32_t B, int32_t H, int32_t W,
                           int32_t cap, const int32_t* nlabels, const int32_t* int_cols,
                           const uint8_t* select, int32_t npixels, int32_t nlevels, double contrast,
                           int32_t mode, int32_t connectivity, int32_t lds_max_box,
                           int32_t* labels_out, int32_t* nlabels_out, int32_t* status_out,
                           void* stream) {
  if (!data) return fail(BSGP_ERR_ARG, "data is NULL");
  if (!labels || !nlabels || !int_cols) return fail(BSGP_ERR_ARG, "labels / nlabels / int_cols is NULL");
  if (!labels_out || !nlabels_out || !status_out)
    return fail(BSGP_ERR_ARG, "labels_out / nlabels_out / status_out is NULL");
  if (labels_out == labels) return fail(BSGP_ERR_ARG, "labels_out must not be labels");
  if (cap < 1) return fail(BSGP_ERR_ARG, "cap must be >= 1");
  if (npixels < 1) return fail(BSGP_ERR_ARG, "npixels must be >= 1");
  if (nlevels < 1) return fail(BSGP_ERR_ARG, "nlevels must be >= 1");
  if (!(contrast >= 0.0 && contrast <= 1.0)) return fail(BSGP_ERR_ARG, "contrast must lie in [0, 1]");
  if (mode != BSGP_DEBLEND_LINEAR && mode != BSGP_DEBLEND_EXPONENTIAL)
    return fail(BSGP_ERR_ARG, "mode must be BSGP_DEBLEND_LINEAR or BSGP_DEBLEND_EXPONENTIAL");
  if (connectivity != 4 && connectivity != 8)
    return fail(BSGP_ERR_ARG, "connectivity must be 4 or 8");
  if (int rc = seg_shape(B, H, W)) return rc;
  DeblendArgs a{};
  a.data = data, a.labels = labels, a.nlabels = nlabels, a.icols = int_cols, a.sel = select;
  a.B = B, a.H = H, a.W = W, a.cap = cap, a.npixels = npixels, a.nlevels = nlevels;
  a.conn = connectivity, a.mode = mode, a.contrast = contrast;
  a.labels_out = labels_out, a.nlabels_out = nlabels_out, a.status = status_out;
  a.large = lds_max_box >= 0;
  a.lds_max_box = a.large ? lds_max_box : kDeblendMaxBox;
  hipStream_t s = (hipStream_t)stream;
  // stream-ordered workspace: the call stays asynchronous.  The global-memory
  // path adds 32 bytes per pixel (one double and six ints), sized by B, H, W
  // alone and never initialised.
  const size_t rows = (size_t)B * cap, px = a.large ? (size_t)B * H * W : 0;
  void* w = nullptr;
  HIP_TRY(hipMallocAsync(&w, px * (sizeof(double) + 6 * sizeof(int)) + 2 * rows * sizeof(int), s));
  a.hkey = static_cast<double*>(w);
  a.lev = reinterpret_cast<int*>(a.hkey + px);
  a.reg = a.lev + px, a.cnt = a.reg + px, a.kept = a.cnt + px, a.mk = a.kept + px;
  a.hidx = a.mk + px;
  a.nchild = a.hidx + px;
  a.base = a.nchild + rows;
  hipError_t e = hipMemsetAsync(a.nchild, 0, rows * sizeof(int), s);
  if (e == hipSuccess) e = hipMemsetAsync(status_out, 0, (size_t)B * sizeof(int), s);
  if (e == hipSuccess) e = launch_deblend(a, s);
  const hipError_t ef = hipFreeAsync(w, s);
  if (e != hipSuccess) return fail(BSGP_ERR_HIP, std::string("deblend launch: ") + hipGetErrorString(e));
  HIP_TRY(ef);
  return BSGP_OK;
}

int bsgp_deblend_sources(const double* data, const int32_t* labels, int32_t B, int32_t H, int32_t W,
                         int32_t cap, const int32_t* nlabels, const int32_t* int_cols,
                         const uint8_t* select, int32_t npixels, int32_t nlevels, double contrast,
                         int32_t mode, int32_t connectivity, int32_t* labels_out,
                         int32_t* nlabels_out, int32_t* status_out, void* stream) {
  return deblend_sources(data, labels, B, H, W, cap, nlabels, int_cols, select, npixels, nlevels,
                         contrast, mode, connectivity, -1, labels_out, nlabels_out, status_out,
                         stream);
}

int bsgp_deblend_sources_large(const double* data, const int32_t* labels, int32_t B, int32_t H,
                               int32_t W, int32_t cap, const int32_t* nlabels,
                               const int32_t* int_cols, const uint8_t* select, int32_t npixels,
                               int32_t nlevels, double contrast, int32_t mode,
                               int32_t connectivity, int32_t lds_max_box, int32_t* labels_out,
                               int32_t* nlabels_out, int32_t* status_out, void* stream) {
  if (lds_max_box < 0 || lds_max_box > BSGP_DEBLEND_MAX_BOX)
    return fail(BSGP_ERR_ARG, "lds_max_box must lie in 0 .. BSGP_DEBLEND_MAX_BOX");
  return deblend_sources(data, labels, B, H, W, cap, nlabels, int_cols, select, npixels, nlevels,
                         contrast, mode, connectivity, lds_max_box, labels_out, nlabels_out,
                         status_out, stream);
}

int bsgp_radial_profile(const void* data, int32_t dtype, int32_t B, int32_t H, int32_t W,
                        const double* centers, int32_t rcap, double* prof, int32_t* len,
                        void* stream) {
  if (!data) return fail(BSGP_ERR_ARG, "data is NULL");
  if (!centers) return fail(BSGP_ERR_ARG, "centers is NULL");
  if (!prof || !len) return fail(BSGP_ERR_ARG, "prof / len is NULL");
  if (dtype != BSGP_DTYPE_F32 && dtype != BSGP_DTYPE_F64)
    return fail(BSGP_ERR_ARG, "dtype must be BSGP_DTYPE_F32 or BSGP_DTYPE_F64");
  if (B < 1 || H < 1 || W < 1) return fail(BSGP_ERR_ARG, "B, H and W must be >= 1");
  if (rcap < 1) return fail(BSGP_ERR_ARG, "rcap must be >= 1");
  char msg[160];
  if ((int64_t)H * W > kStampMaxPixels) {
    snprintf(msg, sizeof msg, "stamp of %lld pixels: a stamp holds at most %d (H * W <= %d)",
             (long long)H * W, kStampMaxPixels, kStampMaxPixels);
    return fail(BSGP_ERR_UNSUPPORTED, msg);
  }
  if (rcap > kStampMaxBins) {
    snprintf(msg, sizeof msg, "%d radial bins: a profile holds at most %d", rcap, kStampMaxBins);
    return fail(BSGP_ERR_UNSUPPORTED, msg);
  }
  StampProfArgs a{};
  a.data = data, a.centers = centers, a.B = B, a.H = H, a.W = W, a.rcap = rcap;
  a.prof = prof, a.len = len;
  HIP_TRY(launch_stamp_radprof(a, dtype == BSGP_DTYPE_F32, (hipStream_t)stream));
  return BSGP_OK;
}

int bsgp_fit_gauss1d(const double* prof, const int32_t* len, int32_t B, int32_t rcap,
                     const double* fwhm, double* fitted, double* params, double* perr,
                     int32_t* info, void* stream) {
  if (!prof || !len || !fwhm) return fail(BSGP_ERR_ARG, "prof / len / fwhm is NULL");
  if (!fitted || !params || !perr || !info)
    return fail(BSGP_ERR_ARG, "fitted / params / perr / info is NULL");
  if (B < 1 || rcap < 1) return fail(BSGP_ERR_ARG, "B and rcap must be >= 1");
  if (rcap > kStampMaxBins) {
    char msg[128];
    snprintf(msg, sizeof msg, "profiles of %d values: a profile holds at most %d", rcap,
             kStampMaxBins);
    return fail(BSGP_ERR_UNSUPPORTED, msg);
  }
  StampFitArgs a{};
  a.prof = prof, a.len = len, a.fwhm = fwhm, a.B = B, a.rcap = rcap;
  a.fitted = fitted, a.params = params, a.perr = perr, a.info = info;
  HIP_TRY(launch_stamp_fit(a, (hipStream_t)stream));
  return BSGP_OK;
}

int bsgp_wasserstein1(const double* u, const int32_t* ulen, const double* v, const int32_t* vlen,
                      int32_t B, int32_t rcap, double* out, void* stream) {
  if (!u || !v) return fail(BSGP_ERR_ARG, "u / v is NULL");
  if (!out) return fail(BSGP_ERR_ARG, "out is NULL");
  if (B < 1 || rcap < 1) return fail(BSGP_ERR_ARG, "B and rcap must be >= 1");
  if (rcap > kStampMaxBins) {
    char msg[128];
    snprintf(msg, sizeof msg, "samples of %d values: a sample holds at most %d", rcap,
             kStampMaxBins);
    return fail(BSGP_ERR_UNSUPPORTED, msg);
  }
  StampW1Args a{};
  a.u = u, a.v = v, a.ulen = ulen, a.vlen = vlen, a.B = B, a.rcap = rcap, a.out = out;
  a.P = 2;
  while (a.P < 2 * rcap) a.P *= 2;
  HIP_TRY(launch_stamp_w1(a, (hipStream_t)stream));
  return BSGP_OK;
}

int bsgp_beta_div(int64_t n, const double* y, const double* x, double beta, double* out,
                  void* stream) {
  if (n < 1 || n > 0x7fffffff || !y || !x || !out) return fail(BSGP_ERR_ARG, "bad arguments");
  HIP_TRY(launch_beta_div((int)n, y, x, beta, out, (hipStream_t)stream));
  return BSGP_OK;
}

int bsgp_beta_div_deriv(int64_t n, const double* y, const double* x, double beta, double* out,
                        void* stream) {
  if (n < 1 || !y || !x || !out) return fail(BSGP_ERR_ARG, "bad arguments");
  HIP_TRY(launch_beta_div_deriv(n, y, x, beta, out, (hipStream_t)stream));
  return BSGP_OK;
}

int bsgp_beta_div_grad_parts(int64_t n, const double* den, const double* gn, double beta,
                             double* pow1, double* w, void* stream) {
  if (n < 1 || !den || !gn || !pow1 || !w) return fail(BSGP_ERR_ARG, "bad arguments");
  HIP_TRY(launch_grad_parts(n, den, gn, beta, pow1, w, (hipStream_t)stream));
  return BSGP_OK;
}

}  // extern "C"
