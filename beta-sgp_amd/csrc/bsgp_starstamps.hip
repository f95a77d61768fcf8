// bsgp_starstamps.hip — the two ends of the star-stamp application around the
// solver and the metrics (restoration/application_sgp_star_stamps.py:56-148;
// include/bsgp.h and DESIGN §3.11):
//
//  k_extract_stamps<T>  Cutout2D(img, (x, y), size) in mode 'trim' (:58) for n
//                       float positions.  One workgroup per stamp; the box is
//                       astropy 4.3.1's overlap_slices rule, evaluated by every
//                       thread from the two coordinates (uniform loads); the
//                       sh * sw elements are walked in raster order, so the
//                       stores are contiguous over the whole stamp and the
//                       loads contiguous along each image row.  Pixels of the
//                       box outside the image are written as 0.
//  k_stamp_select       the choice among the K candidates of a star and its
//                       result row (:92-98, 125-139).  One wave per star: lane
//                       k scores candidate k, a shuffle reduction ordered by
//                       (score, k) finds what sgp.argmin_strict finds, lane 0
//                       writes the row.
//
// The shape columns follow segmentation.shape_columns operation for
// operation, without contraction, so fwhm and ellipticity equal the host's bit
// for bit.
#include <hip/hip_runtime.h>

#include "bsgp_apps.hpp"
#include "bsgp_prims.hpp"

#pragma clang fp contract(off)

namespace bsgp {

namespace {


// imin = (int)ceil(pos - size / 2.0), kept inside +-kStampBoxLimit so that
// imin + size is an int; a box clamped there has no overlap with any image
__device__ __forceinline__ int ss_box_min(double pos, int size) {
  double e = ceil(pos - (double)size / 2.0);
  const double lim = (double)kStampBoxLimit;
  e = e < -lim ? -lim : (e > lim ? lim : e);
  return (int)e;
}

// np.maximum(v, 0.0): NaN stays NaN
__device__ __forceinline__ double ss_clip0(double v) { return (v >= 0.0 || v != v) ? v : 0.0; }

// fwhm and ellipticity of segmentation.shape_columns from covar_sigx2 / sigxy /
// sigy2, as numpy evaluates them for arrays (the catalogue's call): one
// correctly rounded operation each
__device__ __forceinline__ void ss_shape(double sx, double sxy, double sy, double* fwhm, double* ell) {
  const double half = __ddiv_rn(__dadd_rn(sx, sy), 2.0);
  const double d = __ddiv_rn(__dsub_rn(sx, sy), 2.0);
  const double root = __dsqrt_rn(__dadd_rn(__dmul_rn(d, d), __dmul_rn(sxy, sxy)));
  const double a2 = ss_clip0(__dadd_rn(half, root)), b2 = ss_clip0(__dsub_rn(half, root));
  const double a = __dsqrt_rn(a2), b = __dsqrt_rn(b2);
  *ell = __dsub_rn(1.0, __ddiv_rn(b, a));
  // np.log(2.0)
  *fwhm = __dmul_rn(2.0, __dsqrt_rn(__dmul_rn(0.6931471805599453, __dadd_rn(a2, b2))));
}

}  // namespace

template <typename T>
__global__ void __launch_bounds__(256) k_extract_stamps(StampCutArgs a) {
  const int s = blockIdx.x, tid = threadIdx.x;
  const double x = a.xy[2 * (size_t)s], y = a.xy[2 * (size_t)s + 1];
  int x0 = 0, y0 = 0, st = 0;
  if (!(__builtin_isfinite(x) && __builtin_isfinite(y))) {
    st = BSGP_STAMP_BAD_POSITION;
  } else {
    x0 = ss_box_min(x, a.sw), y0 = ss_box_min(y, a.sh);
    if (x0 >= a.W || x0 + a.sw <= 0 || y0 >= a.H || y0 + a.sh <= 0)
      st = BSGP_STAMP_NO_OVERLAP;
    else if (x0 < 0 || y0 < 0 || x0 + a.sw > a.W || y0 + a.sh > a.H)
      st = BSGP_STAMP_PARTIAL;
  }
  if (tid == 0) {
    int* bx = a.box + 4 * (size_t)s;
    const bool none = st == BSGP_STAMP_BAD_POSITION;
    bx[0] = x0, bx[1] = y0, bx[2] = none ? 0 : x0 + a.sw, bx[3] = none ? 0 : y0 + a.sh;
    a.status[s] = st;
  }
  const T* img = static_cast<const T*>(a.img);
  const int N = a.sh * a.sw;  // <= kStampCutMaxPixels (checked on the host)
  T* out = static_cast<T*>(a.out) + (size_t)s * N;
  const bool copy = st == 0 || st == BSGP_STAMP_PARTIAL;
  for (int p = tid; p < N; p += 256) {
    const int r = p / a.sw, c = p - r * a.sw;
    const int iy = y0 + r, ix = x0 + c;
    T v = (T)0;
    if (copy && iy >= 0 && iy < a.H && ix >= 0 && ix < a.W) v = img[(size_t)iy * a.W + ix];
    out[p] = v;
  }
}

__global__ void __launch_bounds__(64) k_stamp_select(StampSelectArgs a) {
  const int s = blockIdx.x, lane = threadIdx.x;
  const double* oc = a.obs_cols + (size_t)s * a.obs_stride;
  const double flux_o = oc[0];
  // the running minimum from +inf of this lane's candidates, ascending: a
  // later equal score does not replace an earlier one, NaN replaces nothing
  double low = dev_inf();
  int best = 0x7fffffff;
  for (int k = lane; k < a.K; k += 64) {
    const size_t i = (size_t)s * a.K + k;
    double sc = dev_inf();
    if (a.res_nlabels[i] > 0) sc = __dsub_rn(1.0, __ddiv_rn(a.res_cols[i * a.res_stride], flux_o));
    a.scores[i] = sc;
    if (sc < low) low = sc, best = k;
  }
  for (int o = 32; o > 0; o >>= 1) {
    const double l2 = __shfl_xor(low, o, 64);
    const int b2 = __shfl_xor(best, o, 64);
    if (l2 < low || (l2 == low && b2 < best)) low = l2, best = b2;
  }
  if (lane != 0) return;
  int st = 0;
  if (a.K == 1) {  // the KL branch: no search, the one restoration is the result
    best = 0;
    if (a.res_nlabels[s] <= 0) st = BSGP_STAMP_RESTORED_NO_SOURCE;
  } else if (best == 0x7fffffff) {
    best = -1;
    st = BSGP_STAMP_NO_CANDIDATE;
  }
  double fwhm_o, ell_o;
  ss_shape(oc[5], oc[6], oc[7], &fwhm_o, &ell_o);
  double* row = a.rows + (size_t)s * kStampRowCols;
  row[0] = flux_o;
  row[5] = oc[3], row[6] = oc[4], row[7] = fwhm_o;
  if (st) {
    const double q = dev_nan();
    row[1] = q, row[2] = q, row[3] = q, row[4] = q, row[8] = q, row[9] = q, row[10] = q;
    a.num_iters[s] = -1;
  } else {
    const size_t i = (size_t)s * a.K + best;
    const double* rc = a.res_cols + i * a.res_stride;
    double fwhm_r, ell_r;
    ss_shape(rc[5], rc[6], rc[7], &fwhm_r, &ell_r);
    row[1] = rc[0];
    row[2] = __dsub_rn(1.0, __ddiv_rn(rc[0], flux_o));
    row[3] = __ddiv_rn(fwhm_r, fwhm_o);
    row[4] = __ddiv_rn(ell_r, ell_o);
    row[8] = rc[3], row[9] = rc[4], row[10] = fwhm_r;
    a.num_iters[s] = a.iters[i];
  }
  a.best[s] = best;
  a.status[s] = st;
}

hipError_t launch_extract_stamps(const StampCutArgs& a, int f32, hipStream_t s) {
  if (f32)
    hipLaunchKernelGGL(k_extract_stamps<float>, dim3(a.n), dim3(256), 0, s, a);
  else
    hipLaunchKernelGGL(k_extract_stamps<double>, dim3(a.n), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_stamp_select(const StampSelectArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k_stamp_select, dim3(a.n), dim3(64), 0, s, a);
  return hipGetLastError();
}

}  // namespace bsgp
