// bsgp_plan.hip — plans of the C-ABI host layer (declared in include/bsgp.h):
// a plan's layout (bsgp_layout.hpp plan_layout), its twiddles and the PSF
// transfer functions built on the device, and the operator A / AT on a plan.
// The solves on a plan are in bsgp_solve.hip.  No PyTorch types cross this
// boundary.
#include <cmath>
#include <cstdio>
#include <memory>
#include <vector>

#include "bsgp_host.hpp"

using namespace bsgp;

static_assert(layout::kWaves == kWaves && layout::kMaxRed == kMaxRed &&
                  layout::kSharedBytes == kSharedBytes && layout::kCoopBlock == kCoopBlock &&
                  layout::kCoopGroups == kCoopGroups,
              "bsgp_layout.hpp restates the kernels' constants");

namespace {

std::vector<cd> twiddles(int n) {
  std::vector<cd> t(n);
  const long double pi = 3.141592653589793238462643383279502884L;
  for (int k = 0; k < n; ++k) {
    const long double a = -2.0L * pi * (long double)k / (long double)n;
    t[k] = cmk((double)cosl(a), (double)sinl(a));
  }
  return t;
}

// The plan's geometry and sizes from its layout (the pointers come later).
void apply_layout(bsgp_plan p, const PlanLayout& l) {
  Geo& g = p->g;
  g.H = l.H, g.W = l.W, g.P = l.P, g.Q = l.Q, g.Qh = l.Qh;
  g.nfw = l.nfw, g.nfc = l.nfc, g.coop = l.coop, g.lpad = l.lpad, g.sld = l.sld;
  g.tw2 = l.tw2, g.twmix = l.twmix;
  g.fp = l.fp;
  g.fq = l.fq;
  p->lds_fft_bytes = l.lds_fft_bytes;
  p->lds_bytes = l.lds_bytes;
  p->wg_per_cu = l.wg_per_cu;
  p->vec_stride = l.vec_stride;
  p->spec_off = l.spec_off;
  p->slot_stride = l.slot_stride;
}

// Circularly-placed kernels for A and AT on the P x Q grid (AT's stays zero in
// circular mode: its transfer function is conj(TF_A)).
void place_kernels(const Geo& g, const double* psf, int kh, int kw, int conv_mode,
                   std::vector<double>& kA, std::vector<double>& kAT) {
  const int H = g.H, W = g.W;
  if (conv_mode == BSGP_CONV_CIRCULAR) {
    // fftshift(psf): out[i][j] = psf[(i - H//2) mod H][(j - W//2) mod W]  (sgp.py:109)
    for (int i = 0; i < H; ++i)
      for (int j = 0; j < W; ++j) {
        const int si = ((i - H / 2) % H + H) % H, sj = ((j - W / 2) % W + W) % W;
        kA[(size_t)i * W + j] = psf[(size_t)si * W + sj];
      }
    return;
  }
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

// The plan's transfer functions of A and AT from the host PSF.
int build_tf(bsgp_plan p, const double* psf) {
  Geo& g = p->g;
  const size_t PQ = (size_t)g.P * g.Q, tfn = (size_t)g.Qh * g.P;
  std::vector<double> kA(PQ, 0.0), kAT(PQ, 0.0);
  place_kernels(g, psf, p->kh, p->kw, p->conv_mode, kA, kAT);
  DevBuf<double> kc;
  DevBuf<cd> spec;
  if (p->tf.reserve(2 * tfn) != hipSuccess || kc.reserve(2 * PQ) != hipSuccess ||
      spec.reserve((size_t)g.P * g.Qh) != hipSuccess)
    return fail(BSGP_ERR_HIP, "plan allocation failed");
  g.tfA = p->tf;
  g.tfAT = p->tf + tfn;
  const double scale = 1.0 / ((double)g.P * (double)g.Q);
  if (hipMemcpy(kc, kA.data(), PQ * sizeof(double), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(kc + PQ, kAT.data(), PQ * sizeof(double), hipMemcpyHostToDevice) != hipSuccess)
    return fail(BSGP_ERR_HIP, "psf upload failed");
  if (launch_build_tf(g, kc, spec, p->tf, scale, 0, p->lds_bytes, 0) != hipSuccess)
    return fail(BSGP_ERR_HIP, "build_tf(A) launch failed");
  if (hipDeviceSynchronize() != hipSuccess) return fail(BSGP_ERR_HIP, "build_tf(A) failed");
  // circular: TF_AT = conj(TF_A) (sgp.py:110); linear: FFT of the transposed kernel
  const bool circ = p->conv_mode == BSGP_CONV_CIRCULAR;
  if (launch_build_tf(g, circ ? kc : kc + PQ, spec, p->tf + tfn, scale, circ ? 1 : 0,
                      p->lds_bytes, 0) != hipSuccess)
    return fail(BSGP_ERR_HIP, "build_tf(AT) launch failed");
  if (hipDeviceSynchronize() != hipSuccess) return fail(BSGP_ERR_HIP, "build_tf(AT) failed");
  return BSGP_OK;
}

}  // namespace

extern "C" {

int32_t bsgp_abi_version(void) { return 3; }

const char* bsgp_last_error(void) { return g_err.c_str(); }

// Diagnostics (not in include/bsgp.h): the numpy float32 reduction program the
// plans use for N = n elements (tests/test_oracle.py evaluates it against
// np.sum).  counts = {nleaf, nnode, nlev, nchunk}; returns the program length,
// copying at most cap ints to out.
int64_t bsgp_pairwise_program(int64_t n, int32_t* out, int64_t cap, int32_t* counts) {
  if (n < 1) return fail(BSGP_ERR_ARG, "n must be >= 1");
  int c[4];
  const std::vector<int> prog = pairwise_program((long)n, c);
  for (int i = 0; counts && i < 4; ++i) counts[i] = c[i];
  for (int64_t i = 0; out && i < cap && i < (int64_t)prog.size(); ++i) out[i] = prog[i];
  return (int64_t)prog.size();
}

// Diagnostics (not in include/bsgp.h): the layout bsgp_plan_create would give
// a plan of these arguments (plan_layout with the environment's plan-time
// knobs); needs no GPU.  Copies at most n of these values to out:
//   0 H        1 W          2 P           3 Q           4 Qh        5 sld
//   6 lpad     7 nfw        8 nfc         9 coop       10 tw2      11 twmix
//  12 fp.lds_tw   13 fq.lds_tw   14 fp.lds_tw2   15 fq.lds_tw2
//  16 lds_fft_bytes   17 lds_bytes   18 wg_per_cu
//  19 vec_stride   20 spec_off   21 slot_stride (doubles)
//  22 fp.ns   23 fq.ns   24.. fp's kMaxStages radices, then fq's (0 past ns)
int bsgp_plan_layout(int32_t H, int32_t W, int32_t kh, int32_t kw, int32_t conv_mode,
                     int32_t storage, int64_t* out, int32_t n) {
  if (!out || n < 0) return fail(BSGP_ERR_ARG, "out is NULL or n < 0");
  if (int rc = check_plan_shape(H, W, kh, kw, conv_mode, storage)) return rc;
  PlanLayout l;
  if (int rc = plan_layout(H, W, kh, kw, conv_mode, storage, PlanKnobs::from_env(), &l)) return rc;
  int64_t v[24 + 2 * kMaxStages] = {
      l.H,          l.W,          l.P,           l.Q,           l.Qh,
      l.sld,        l.lpad,       l.nfw,         l.nfc,         l.coop,
      l.tw2,        l.twmix,      l.fp.lds_tw,   l.fq.lds_tw,   l.fp.lds_tw2,
      l.fq.lds_tw2, (int64_t)l.lds_fft_bytes,    (int64_t)l.lds_bytes,        l.wg_per_cu,
      (int64_t)l.vec_stride,      (int64_t)l.spec_off,          (int64_t)l.slot_stride,
      l.fp.ns,      l.fq.ns};
  for (int i = 0; i < l.fp.ns; ++i) v[24 + i] = l.fp.radix[i];
  for (int i = 0; i < l.fq.ns; ++i) v[24 + kMaxStages + i] = l.fq.radix[i];
  for (int i = 0; i < n && i < 24 + 2 * kMaxStages; ++i) out[i] = v[i];
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
  if (!psf) return fail(BSGP_ERR_ARG, "bad shape or psf");
  if (int rc = check_plan_shape(H, W, kh, kw, conv_mode, storage)) return rc;
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
  PlanLayout lay;
  if (int rc = plan_layout(H, W, kh, kw, conv_mode, storage, PlanKnobs::from_env(), &lay))
    return rc;
  DEVICE_SCOPE(device);
  // every early exit below destroys what the plan holds so far
  std::unique_ptr<bsgp_plan_s, PlanDeleter> p(new bsgp_plan_s());
  p->device = device;
  p->conv_mode = conv_mode;
  p->kh = kh;
  p->kw = kw;
  p->storage = storage;
  apply_layout(p.get(), lay);
  Geo& g = p->g;
  int ncu = 0;
  if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess &&
      ncu > 0)
    p->ncu = ncu;
  if (bsgp_c512_args_size() != sizeof(SolveArgs) || bsgp_c512_block() != kCoopBlock)
    return fail(BSGP_ERR_HIP, "cooperative 512-thread build does not match this library");
  if (bsgp_app_args_size() != sizeof(SolveArgs))
    return fail(BSGP_ERR_HIP, "application-size persistent build does not match this library");
  if (set_solver_lds_limit(p->lds_bytes) != hipSuccess)
    return fail(BSGP_ERR_HIP, "hipFuncSetAttribute(MaxDynamicSharedMemorySize) failed");
  if (team_resident_per_cu(g.coop != 0, storage, p->lds_bytes, &p->resident_per_cu) !=
          hipSuccess ||
      p->resident_per_cu < 1)
    return fail(BSGP_ERR_HIP, "occupancy query of the team kernels failed");
  {
    std::vector<cd> tw = twiddles(g.P);
    const std::vector<cd> twq = twiddles(g.Q);
    tw.insert(tw.end(), twq.begin(), twq.end());
    if (p->tw.reserve(tw.size()) != hipSuccess ||
        hipMemcpy(p->tw, tw.data(), tw.size() * sizeof(cd), hipMemcpyHostToDevice) != hipSuccess)
      return fail(BSGP_ERR_HIP, "twiddle upload failed");
    g.fp.tw = p->tw;
    g.fq.tw = p->tw + g.P;
  }
  if (int rc = build_tf(p.get(), psf)) return rc;
  {
    int c[4];
    const std::vector<int> prog = pairwise_program((long)H * W, c);
    if (p->pwprog.reserve(prog.size()) != hipSuccess ||
        hipMemcpy(p->pwprog, prog.data(), prog.size() * sizeof(int), hipMemcpyHostToDevice) !=
            hipSuccess)
      return fail(BSGP_ERR_HIP, "pairwise program upload failed");
    p->pw = PwProg{p->pwprog, c[0], c[1], c[2], c[3]};
  }
  if (p->active.reserve(256 / sizeof(int)) != hipSuccess ||
      p->active_h.alloc(hipHostMallocDefault) != hipSuccess ||
      p->done_h.alloc(hipHostMallocMapped) != hipSuccess ||
      hipHostGetDevicePointer((void**)&p->done_d, p->done_h.p, 0) != hipSuccess)
    return fail(BSGP_ERR_HIP, "counter allocation failed");
  // a reused pinned block may still hold an old plan's seq; seqs
  // also come from one process-wide counter, so a stale word never matches
  *p->done_h.p = 0;
  *out = p.release();
  return BSGP_OK;
}

int bsgp_plan_destroy(bsgp_plan p) {
  if (!p) return BSGP_OK;
  DeviceGuard dev_guard_(p->device);
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
  DevBuf<cd> tf, spec;
  DevBuf<double> kc, sums;
  int rc = BSGP_OK;
  if (tf.reserve((size_t)n * 2 * tfn) != hipSuccess ||
      kc.reserve((size_t)chunk * 2 * PQ) != hipSuccess ||
      spec.reserve((size_t)chunk * specn) != hipSuccess || sums.reserve((size_t)n) != hipSuccess)
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
  if (rc != BSGP_OK) return rc;
  p->tf.swap(tf);  // the plan's old transfer functions go with `tf`
  p->n_tf = n;
  g.tfA = p->tf;
  g.tfAT = p->tf + tfn;
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
  HIP_TRY(p->opws.reserve((size_t)grid * stride));
  if (split)
    HIP_TRY(launch_apply_op_split(p->g, B, transpose, x, out, p->opws, stride, slots / B,
                                  p->lds_bytes, (hipStream_t)stream));
  else
    HIP_TRY(launch_apply_op(p->g, B, transpose, x, out, p->opws, stride, grid, p->lds_bytes,
                            (hipStream_t)stream));
  return BSGP_OK;
}

}  // extern "C"
