// bsgp_validate.hip — the validation of detected sources: what the reference's
// utils.validation_source (restoration/utils.py:313-329) decides for one source
// from three 100 x 100 cutouts, for every source of a batch of catalogues in
// one launch (include/bsgp.h and DESIGN §3.13, V1 to V6).
//
//  k_validate<T>  one 256-thread workgroup per (source, image).  The box is
//                 astropy 4.3.1's overlap_slices rule (as k_extract_stamps);
//                 its sh * sw cells are read straight from the image, the
//                 background map and the rms map, a cell outside the frame
//                 being 0.0.  No cutout is written anywhere.
//                   V2  every thread keeps the three largest image values it
//                       meets in registers; the waves merge theirs by
//                       shuffles, thread 0 merges the four waves'.
//                   V3  the background window goes to dynamic LDS, padded
//                       with +inf to a power of two, is sorted there
//                       (bkg_sort, bsgp_sigclip.hpp) and read at the two
//                       middle ranks.
//                   V4  numpy's sum of the rms window (pairwise inside its
//                       buffers of 8192 values): thread 0 writes the leaf
//                       table of n = sh * sw (a function of n alone,
//                       bsgp_validate.hpp), every leaf of <= 128 values is
//                       summed by one lane with numpy's 8 accumulators,
//                       thread 0 folds the leaf sums in numpy's order.
//                 A NaN in the image or the background window is seen while
//                 the window is read and makes that statistic NaN; the rms
//                 sum carries its own.
#include <hip/hip_runtime.h>

#include "bsgp_apps.hpp"
#include "bsgp_prims.hpp"
#include "bsgp_sigclip.hpp"
#include "bsgp_validate.hpp"

#pragma clang fp contract(off)

namespace bsgp {

static_assert(kValidateMax == 16384, "bsgp_validate.hpp counts the leaves of n <= 16384");
static_assert(kValidateMax * sizeof(double) + 8192 <= 160 * 1024, "the window and the tables fit the LDS");

namespace {

// imin = (int)ceil(pos - size / 2.0), kept inside +-kStampBoxLimit so that
// imin + size is an int; a box clamped there has no overlap with any image
__device__ __forceinline__ int vs_box_min(double pos, int size) {
  double e = ceil(pos - (double)size / 2.0);
  const double lim = (double)kStampBoxLimit;
  e = e < -lim ? -lim : (e > lim ? lim : e);
  return (int)e;
}

// the window's cell (r, c) of a frame: 0 outside the frame (V1)
template <typename U>
__device__ __forceinline__ U vs_cell(const U* f, int H, int W, int y0, int x0, int r, int c) {
  const int iy = y0 + r, ix = x0 + c;
  return (iy >= 0 && iy < H && ix >= 0 && ix < W) ? f[(size_t)iy * W + ix] : (U)0;
}

// the next cell in raster order
__device__ __forceinline__ double vs_next(const double* f, int H, int W, int y0, int x0, int sw,
                                          int& r, int& c) {
  const double v = vs_cell(f, H, W, y0, x0, r, c);
  if (++c == sw) c = 0, ++r;
  return v;
}

// v into the ascending triple (t0, t1, t2) of the largest values so far
template <typename T>
__device__ __forceinline__ void vs_top3(T v, T& t0, T& t1, T& t2) {
  // selects, not branches: stores through a chosen reference put the triple in scratch
  const bool g0 = v > t0, g1 = v > t1, g2 = v > t2;
  t0 = g1 ? t1 : (g0 ? v : t0);
  t1 = g2 ? t2 : (g1 ? v : t1);
  t2 = g2 ? v : t2;
}

template <typename T>
__device__ __forceinline__ T vs_neg_inf() {
  return (T)(-dev_inf());
}

}  // namespace

template <typename T>
__global__ void __launch_bounds__(256) k_validate(ValidateArgs a) {
  extern __shared__ double s[];  // a.P values: the background window
  __shared__ PairwiseStack stk;
  __shared__ int loff[kValidateMaxLeaves], llen[kValidateMaxLeaves];
  __shared__ double lsum[kValidateMaxLeaves];
  __shared__ T wtop[4 * 3];
  __shared__ int nleaf, nanbits;
  const int tid = threadIdx.x, lane = tid & 63, row = blockIdx.x, b = blockIdx.y;
  int nr = a.n ? a.n[b] : a.cap;
  nr = nr < a.cap ? nr : a.cap;
  if (row >= nr) return;
  const size_t rr = (size_t)b * a.cap + row;
  const double x = a.xy[rr * a.xy_stride], y = a.xy[rr * a.xy_stride + 1];

  // V1, V6: the box and its status (uniform over the workgroup)
  int x0 = 0, y0 = 0, st = 0;
  if (!(__builtin_isfinite(x) && __builtin_isfinite(y))) {
    st = BSGP_STAMP_BAD_POSITION;
  } else {
    x0 = vs_box_min(x, a.sw), y0 = vs_box_min(y, a.sh);
    if (x0 >= a.W || x0 + a.sw <= 0 || y0 >= a.H || y0 + a.sh <= 0)
      st = BSGP_STAMP_NO_OVERLAP;
    else if (x0 < 0 || y0 < 0 || x0 + a.sw > a.W || y0 + a.sh > a.H)
      st = BSGP_STAMP_PARTIAL;
  }
  if (st & (BSGP_STAMP_BAD_POSITION | BSGP_STAMP_NO_OVERLAP)) {
    if (tid == 0) {
      const double q = dev_nan();
      a.stats[rr * 3] = q, a.stats[rr * 3 + 1] = q, a.stats[rr * 3 + 2] = q;
      a.valid[rr] = 0;
      a.status[rr] = st;
    }
    return;
  }
  const int n = a.sh * a.sw;  // <= kValidateMax (checked on the host)
  const size_t img_off = (size_t)b * a.H * a.W, map_off = a.maps_per_image ? img_off : 0;
  const T* img = static_cast<const T*>(a.img) + img_off;
  const double* bkg = a.bkg + map_off;
  const double* rms = a.rms + map_off;

  if (tid == 0) {
    nanbits = 0;
    nleaf = (int)np_sum_walk(n, &stk, loff, llen, kValidateMaxLeaves, nullptr);
  }

  // V2: the three largest image values; V3: the background window into LDS
  T t0 = vs_neg_inf<T>(), t1 = t0, t2 = t0;
  bool inan = false, bnan = false;
  for (int p = tid; p < n; p += 256) {
    const int r = p / a.sw, c = p - r * a.sw;
    const T v = vs_cell(img, a.H, a.W, y0, x0, r, c);
    inan |= v != v;
    vs_top3(v, t0, t1, t2);
    const double g = vs_cell(bkg, a.H, a.W, y0, x0, r, c);
    bnan |= g != g;
    s[p] = g;
  }
  for (int p = n + tid; p < a.P; p += 256) s[p] = dev_inf();
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const T u0 = __shfl_xor(t0, o, 64), u1 = __shfl_xor(t1, o, 64), u2 = __shfl_xor(t2, o, 64);
    vs_top3(u0, t0, t1, t2);
    vs_top3(u1, t0, t1, t2);
    vs_top3(u2, t0, t1, t2);
  }
  if (lane == 0) {
    T* w = wtop + 3 * (tid >> 6);
    w[0] = t0, w[1] = t1, w[2] = t2;
  }
  __syncthreads();  // nanbits, the leaf table, wtop and s are written
  const int bits = (__any(inan) ? 1 : 0) | (__any(bnan) ? 2 : 0);
  if (lane == 0 && bits) atomicOr(&nanbits, bits);

  // V4: one leaf per lane, numpy's leaf (np_pairwise_block) over the window's cells
  const int nl = nleaf < kValidateMaxLeaves ? nleaf : kValidateMaxLeaves;
  if (tid < nl) {
    const int off = loff[tid], len = llen[tid];
    int r = off / a.sw, c = off - r * a.sw;
    double acc;
    if (len < 8) {
      acc = 0.0;
      for (int i = 0; i < len; ++i) acc += vs_next(rms, a.H, a.W, y0, x0, a.sw, r, c);
    } else {
      double q[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) q[j] = vs_next(rms, a.H, a.W, y0, x0, a.sw, r, c);
      int i = 8;
      for (; i < len - (len % 8); i += 8) {
#pragma unroll
        for (int j = 0; j < 8; ++j) q[j] += vs_next(rms, a.H, a.W, y0, x0, a.sw, r, c);
      }
      acc = ((q[0] + q[1]) + (q[2] + q[3])) + ((q[4] + q[5]) + (q[6] + q[7]));
      for (; i < len; ++i) acc += vs_next(rms, a.H, a.W, y0, x0, a.sw, r, c);
    }
    lsum[tid] = acc;
  }

  bkg_sort(s, a.P);  // its barriers also publish lsum and nanbits (P >= 2; P == 1 below)
  if (a.P < 2) __syncthreads();
  if (tid != 0) return;

  // V2: np.sort(c.flatten())[-3:].mean() in the image's type
  for (int w = 1; w < 4; ++w) {
    vs_top3(wtop[3 * w], t0, t1, t2);
    vs_top3(wtop[3 * w + 1], t0, t1, t2);
    vs_top3(wtop[3 * w + 2], t0, t1, t2);
  }
  T pix;
  if (n >= 3)
    pix = ((t0 + t1) + t2) / (T)3;
  else if (n == 2)
    pix = (t1 + t2) / (T)2;
  else
    pix = t2;
  double source_pixs = (nanbits & 1) ? dev_nan() : (double)pix;
  // V3: np.median
  const double lo = s[(n - 1) / 2], hi = s[n / 2];
  double med = (n & 1) ? lo : (lo + hi) / 2.0;
  if (nanbits & 2) med = dev_nan();
  // V4: np.mean
  const double mean = np_sum_walk(n, &stk, nullptr, nullptr, 0, lsum) / (double)n;
  // V5
  const int valid = source_pixs > med + a.nsigma * mean ? 1 : 0;
  a.stats[rr * 3] = source_pixs, a.stats[rr * 3 + 1] = med, a.stats[rr * 3 + 2] = mean;
  a.valid[rr] = valid;
  a.status[rr] = st;
}

hipError_t launch_validate(ValidateArgs a, int f32, hipStream_t s) {
  const int n = a.sh * a.sw;
  a.P = 1;
  while (a.P < n) a.P <<= 1;
  const dim3 grid(a.cap, a.B), block(256);
  auto* kern = f32 ? k_validate<float> : k_validate<double>;
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                                     hipFuncAttributeMaxDynamicSharedMemorySize,
                                     kValidateMax * (int)sizeof(double));
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(kern, grid, block, (size_t)a.P * sizeof(double), s, a);
  return hipGetLastError();
}

}  // namespace bsgp
