// bsgp_background.hip — the sky background of a field or a batch of images on
// the device: the estimator restoration/utils.py:235-239 builds with photutils
// (Background2D(data, box_size, filter_size=(3, 3), MedianBackground())),
// restated from its parts:
//
//  k_bkg_boxstats  one workgroup per (box, image): the box's valid pixels are
//                  sorted once in LDS; sigma clipping (astropy SigmaClip,
//                  median / population std, inclusive bounds) then only moves
//                  the two ends [lo, hi) of the sorted range.  Writes the
//                  clipped median and std, the excluded flag, the survivor and
//                  iteration counts of every mesh cell.
//  k_bkg_mesh      one workgroup per image, both meshes in turn, in LDS: fill
//                  of excluded cells (inverse distance, 10 nearest kept
//                  cells), fh x fw median filter ignoring cells outside the
//                  mesh, min / max / median of the filtered mesh, and the
//                  cubic B-spline prefilter along both axes (half-sample
//                  symmetric boundary, scipy.ndimage's recursion).
//  k_bkg_zoom      one thread per pair of adjacent pixels of an output row:
//                  cubic B-spline evaluation at (p + 0.5) / box - 0.5 of both
//                  coefficient meshes, clamped to the filtered mesh's range.
//
// All arithmetic is float64 in a fixed order (no atomics): a batch gives each
// image the bits it gets alone, and a float32 image the bits of its widening.
#include <hip/hip_runtime.h>

#include <cmath>

#include "bsgp_apps.hpp"
#include "bsgp_prims.hpp"
#include "bsgp_reduce.hpp"
#include "bsgp_sigclip.hpp"

namespace bsgp {

namespace {

// min and max of one value per thread over the workgroup, in every thread
__device__ __forceinline__ void block_minmax(double& mn, double& mx, double* red) {
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  mn = wave_min(mn);
  mx = wave_max(mx);
  if (lane == 0) {
    red[w] = mn;
    red[kWaves + w] = mx;
  }
  __syncthreads();
  mn = red[0];
  mx = red[kWaves];
  for (int k = 1; k < kWaves; ++k) {
    mn = red[k] < mn ? red[k] : mn;
    mx = red[kWaves + k] > mx ? red[kWaves + k] : mx;
  }
  __syncthreads();
}

}  // namespace

// ------------------------------------------------------------ box statistics
template <typename T>
__global__ void __launch_bounds__(256) k_bkg_boxstats(BkgArgs a) {
  extern __shared__ double s[];  // the box, padded to a power of two (the launch sizes it)
  __shared__ double red[(kWaves + 1) * kMaxRed];
  const int tid = threadIdx.x, cell = blockIdx.x, b = blockIdx.y;
  const int ncell = a.ny * a.nx;
  const int j = cell / a.nx, i = cell - j * a.nx;
  const int npix = a.bh * a.bw;
  int P = 1;
  while (P < npix) P <<= 1;
  const size_t img_off = (size_t)b * a.H * a.W;
  const T* img = static_cast<const T*>(a.data) + img_off;
  const unsigned char* msk = a.mask ? a.mask + img_off : nullptr;

  // valid pixels, then +inf sentinels up to the power of two
  double cnt[1] = {0.0};
  for (int k = tid; k < P; k += 256) {
    double v = dev_inf();
    if (k < npix) {
      const int r = k / a.bw, c = k - r * a.bw;
      const int y = j * a.bh + r, x = i * a.bw + c;
      if (y < a.H && x < a.W) {
        const size_t o = (size_t)y * a.W + x;
        const double u = (double)img[o];
        if (__builtin_isfinite(u) && !(msk && msk[o])) {
          v = u;
          cnt[0] += 1.0;
        }
      }
    }
    s[k] = v;
  }
  block_sum<1>(cnt, red);
  const int nvalid = (int)cnt[0];

  double* raw = a.ws + (size_t)b * a.ws_stride;
  int* wi = a.wsi + (size_t)b * (1 + 3 * (size_t)ncell) + 1;
  if ((double)(npix - nvalid) > a.excl_count || nvalid == 0) {
    if (tid == 0) {
      raw[cell] = dev_nan();
      raw[ncell + cell] = dev_nan();
      wi[cell] = 1;
      wi[ncell + cell] = 0;
      wi[2 * ncell + cell] = 0;
    }
    return;
  }

  bkg_sort(s, P);

  // sigma clipping on the sorted range [lo, hi) (bsgp_sigclip.hpp)
  const SigClip c = sigma_clip_sorted(s, nvalid, a.sigma, a.maxiters, red);
  if (tid == 0) {
    raw[cell] = c.med;
    raw[ncell + cell] = c.sd;
    wi[cell] = 0;
    wi[ncell + cell] = c.hi - c.lo;
    wi[2 * ncell + cell] = c.it;
  }
}

// --------------------------------------------------------------------- mesh
// scipy.ndimage's cubic spline prefilter of one line (mode='reflect'): gain 6,
// pole z = sqrt(3) - 2.  Its causal start accumulates into c[0] in place, so
// the last term of the sum (i = n - 1) reads the partial sum instead of the
// original c[0]; reproduced here, since the maps are pinned to scipy's zoom.
__device__ __forceinline__ void bkg_prefilter_line(double* c, int n, int stride) {
  const double z = -0x1.126145e9ecd58p-2;  // sqrt(3) - 2 in float64
  for (int i = 0; i < n; ++i) c[i * stride] *= 6.0;
  double zn = 1.0;
  for (int i = 0; i < n; ++i) zn *= z;
  const double c0 = c[0];
  double acc = c0 + zn * c[(n - 1) * stride];
  double zi = z;
  for (int i = 1; i < n; ++i) {
    const double other = (i == n - 1) ? acc : c[(n - 1 - i) * stride];
    acc += zi * (c[i * stride] + zn * other);
    zi *= z;
  }
  acc *= z / (1.0 - zn * zn);
  acc += c0;
  c[0] = acc;
  for (int i = 1; i < n; ++i) c[i * stride] += z * c[(i - 1) * stride];
  c[(n - 1) * stride] *= z / (z - 1.0);
  for (int i = n - 2; i >= 0; --i) c[i * stride] = z * (c[(i + 1) * stride] - c[i * stride]);
}

__global__ void __launch_bounds__(256) k_bkg_mesh(BkgArgs a) {
  __shared__ double A[kBkgMaxCells], F[kBkgMaxCells];
  __shared__ unsigned char ex[kBkgMaxCells];
  __shared__ double red[(kWaves + 1) * kMaxRed];
  const int tid = threadIdx.x, b = blockIdx.x;
  const int ny = a.ny, nx = a.nx, ncell = ny * nx;
  double* ws = a.ws + (size_t)b * a.ws_stride;
  int* wi = a.wsi + (size_t)b * (1 + 3 * (size_t)ncell);
  double* scal = ws + 6 * (size_t)ncell;

  double kc[1] = {0.0};
  for (int c = tid; c < ncell; c += 256) {
    const int e = wi[1 + c];
    ex[c] = (unsigned char)e;
    kc[0] += e ? 0.0 : 1.0;
  }
  block_sum<1>(kc, red);
  const int kept = (int)kc[0];
  if (tid == 0) wi[0] = kept;
  if (a.status) {
    int* st = a.status + (size_t)b * (1 + 3 * (size_t)ncell);
    for (int c = tid; c < 3 * ncell; c += 256) st[1 + c] = wi[1 + c];
    if (tid == 0) st[0] = kept;
  }
  if (kept == 0) {  // every box excluded: the caller reads status[0] == 0
    for (int c = tid; c < 4 * ncell; c += 256) ws[2 * (size_t)ncell + c] = dev_nan();
    if (tid < 8) scal[tid] = dev_nan();
    for (int m = 0; m < 2; ++m) {
      double* mo = m == 0 ? a.mesh : a.rms_mesh;
      if (mo)
        for (int c = tid; c < ncell; c += 256) mo[(size_t)b * ncell + c] = dev_nan();
    }
    if (a.medians && tid < 2) a.medians[2 * (size_t)b + tid] = dev_nan();
    return;
  }

  for (int m = 0; m < 2; ++m) {
    const double* raw = ws + (size_t)m * ncell;
    for (int c = tid; c < ncell; c += 256) A[c] = raw[c];
    __syncthreads();

    // fill: inverse-distance mean of the 10 nearest kept cells, nearest first,
    // ties in row-major order (selected one by one: no per-thread list)
    for (int c = tid; c < ncell; c += 256) {
      if (!ex[c]) continue;
      const int cy = c / nx, cx = c - cy * nx;
      int last_d2 = -1, last_q = -1;
      double sw = 0.0, swv = 0.0;
      const int npick = kept < 10 ? kept : 10;
      for (int p = 0; p < npick; ++p) {
        int best_d2 = 0x7fffffff, best_q = -1;
        for (int q = 0; q < ncell; ++q) {
          if (ex[q]) continue;
          const int qy = q / nx, dy = qy - cy, dx = q - qy * nx - cx;
          const int d2 = dy * dy + dx * dx;
          const bool after = d2 > last_d2 || (d2 == last_d2 && q > last_q);
          if (after && d2 < best_d2) {
            best_d2 = d2;
            best_q = q;
          }
        }
        const double w = 1.0 / sqrt((double)best_d2);
        sw += w;
        swv += w * A[best_q];
        last_d2 = best_d2;
        last_q = best_q;
      }
      F[c] = swv / sw;
    }
    __syncthreads();
    for (int c = tid; c < ncell; c += 256)
      if (ex[c]) A[c] = F[c];
    __syncthreads();

    // median filter, cells outside the mesh ignored (rank by counting)
    const int ry = a.fh / 2, rx = a.fw / 2;
    double mn = dev_inf(), mx = -dev_inf();
    for (int c = tid; c < ncell; c += 256) {
      const int cy = c / nx, cx = c - cy * nx;
      const int y0 = cy - ry < 0 ? 0 : cy - ry, y1 = cy + ry > ny - 1 ? ny - 1 : cy + ry;
      const int x0 = cx - rx < 0 ? 0 : cx - rx, x1 = cx + rx > nx - 1 ? nx - 1 : cx + rx;
      const int n = (y1 - y0 + 1) * (x1 - x0 + 1);
      const int k_lo = (n - 1) / 2, k_hi = n / 2;
      double v_lo = 0.0, v_hi = 0.0;
      for (int uy = y0; uy <= y1; ++uy)
        for (int ux = x0; ux <= x1; ++ux) {
          const double u = A[uy * nx + ux];
          int less = 0, leq = 0;
          for (int wy = y0; wy <= y1; ++wy)
            for (int wx = x0; wx <= x1; ++wx) {
              const double w = A[wy * nx + wx];
              less += w < u;
              leq += w <= u;
            }
          if (less <= k_lo && k_lo < leq) v_lo = u;
          if (less <= k_hi && k_hi < leq) v_hi = u;
        }
      const double f = (n & 1) ? v_lo : (v_lo + v_hi) / 2.0;
      F[c] = f;
      mn = f < mn ? f : mn;
      mx = f > mx ? f : mx;
    }
    __syncthreads();
    block_minmax(mn, mx, red);

    // the filtered mesh, its range and its median (of a sorted copy in A,
    // which is free until the prefilter)
    double* filt = ws + (size_t)(2 + m) * ncell;
    double* mo = m == 0 ? a.mesh : a.rms_mesh;
    int P = 1;
    while (P < ncell) P <<= 1;
    for (int c = tid; c < P; c += 256) {
      const double u = c < ncell ? F[c] : dev_inf();
      A[c] = u;
      if (c < ncell) {
        filt[c] = u;
        if (mo) mo[(size_t)b * ncell + c] = u;
      }
    }
    __syncthreads();
    bkg_sort(A, P);
    if (tid == 0) {
      const double md = (ncell & 1) ? A[ncell / 2] : (A[ncell / 2 - 1] + A[ncell / 2]) / 2.0;
      scal[2 * m] = mn;
      scal[2 * m + 1] = mx;
      scal[4 + m] = md;
      if (a.medians) a.medians[2 * (size_t)b + m] = md;
    }
    __syncthreads();

    // spline coefficients: prefilter along y (one lane per mesh column), then
    // along x (one lane per mesh row); an axis of length 1 stays as it is
    for (int c = tid; c < ncell; c += 256) A[c] = F[c];
    __syncthreads();
    if (ny > 1)
      for (int c = tid; c < nx; c += 256) bkg_prefilter_line(A + c, ny, nx);
    __syncthreads();
    if (nx > 1)
      for (int r = tid; r < ny; r += 256) bkg_prefilter_line(A + r * nx, nx, 1);
    __syncthreads();
    double* coef = ws + (size_t)(4 + m) * ncell;
    for (int c = tid; c < ncell; c += 256) coef[c] = A[c];
    __syncthreads();
  }
}

// --------------------------------------------------------------------- zoom
// index of the half-sample symmetric extension (-1 -> 0, n -> n - 1)
__device__ __forceinline__ int bkg_reflect(int i, int n) {
  if (i < 0) i = -i - 1;
  if (i >= n) i = 2 * n - 1 - i;
  return i < 0 ? 0 : (i >= n ? n - 1 : i);
}

// cubic B-spline taps of output pixel p along an axis of n cells of `box`
// pixels: mesh coordinate (p + 0.5) / box - 0.5, first tap floor(.) - 1
__device__ __forceinline__ int bkg_taps(int p, int box, int n, double (&w)[4]) {
  if (n == 1) {  // constant axis: exactly the one coefficient
    w[0] = 1.0;
    w[1] = w[2] = w[3] = 0.0;
    return 0;
  }
  const double cc = ((double)p + 0.5) / (double)box - 0.5;
  const double fl = floor(cc);
  const double t = cc - fl, z = 1.0 - t;
  w[1] = (t * t * (t - 2.0) * 3.0 + 4.0) / 6.0;
  w[2] = (z * z * (z - 2.0) * 3.0 + 4.0) / 6.0;
  w[0] = z * z * z / 6.0;
  w[3] = 1.0 - w[0] - w[1] - w[2];
  return (int)fl - 1;
}

// PX pixels per thread (2: 16-byte stores; 1 where W is odd or an output is
// not 16-byte aligned).  A workgroup covers 256 * PX pixels of one row and
// first folds the four coefficient rows with the row weights into one line in
// LDS (at most 256 * PX / bw + 4 entries, already reflected at the borders).
template <int PX>
__global__ void __launch_bounds__(256) k_bkg_zoom(BkgArgs a) {
  __shared__ double line[2][kBkgZoomLine];
  const int tid = threadIdx.x, y = blockIdx.y, b = blockIdx.z;
  const int ny = a.ny, nx = a.nx, ncell = ny * nx;
  const double* ws = a.ws + (size_t)b * a.ws_stride;
  const double* coef0 = ws + 4 * (size_t)ncell;
  const double* coef1 = ws + 5 * (size_t)ncell;
  const double* scal = ws + 6 * (size_t)ncell;

  double wy[4];
  const int iy = bkg_taps(y, a.bh, ny, wy);
  const int r0 = bkg_reflect(iy, ny) * nx, r1 = bkg_reflect(iy + 1, ny) * nx;
  const int r2 = bkg_reflect(iy + 2, ny) * nx, r3 = bkg_reflect(iy + 3, ny) * nx;

  const int xa = blockIdx.x * 256 * PX;
  int xl = xa + 256 * PX - 1;
  if (xl > a.W - 1) xl = a.W - 1;
  double wtmp[4];
  const int ixa = bkg_taps(xa, a.bw, nx, wtmp);
  int cnt = bkg_taps(xl, a.bw, nx, wtmp) + 4 - ixa;
  if (cnt > kBkgZoomLine) cnt = kBkgZoomLine;
  for (int k = tid; k < cnt; k += 256) {
    const int ix = bkg_reflect(ixa + k, nx);
    line[0][k] = wy[0] * coef0[r0 + ix] + wy[1] * coef0[r1 + ix] + wy[2] * coef0[r2 + ix] +
                 wy[3] * coef0[r3 + ix];
    line[1][k] = wy[0] * coef1[r0 + ix] + wy[1] * coef1[r1 + ix] + wy[2] * coef1[r2 + ix] +
                 wy[3] * coef1[r3 + ix];
  }
  __syncthreads();

  const int x = xa + tid * PX;
  if (x >= a.W) return;
  double vb[PX], vr[PX];
#pragma unroll
  for (int p = 0; p < PX; ++p) {
    double wx[4];
    int k = bkg_taps(x + p < a.W ? x + p : a.W - 1, a.bw, nx, wx) - ixa;
    k = k < 0 ? 0 : (k > kBkgZoomLine - 4 ? kBkgZoomLine - 4 : k);
    double v0 = wx[0] * line[0][k] + wx[1] * line[0][k + 1] + wx[2] * line[0][k + 2] +
                wx[3] * line[0][k + 3];
    double v1 = wx[0] * line[1][k] + wx[1] * line[1][k + 1] + wx[2] * line[1][k + 2] +
                wx[3] * line[1][k + 3];
    if (a.clip) {
      v0 = v0 < scal[0] ? scal[0] : (v0 > scal[1] ? scal[1] : v0);
      v1 = v1 < scal[2] ? scal[2] : (v1 > scal[3] ? scal[3] : v1);
    }
    vb[p] = v0;
    vr[p] = v1;
  }
  const size_t o = ((size_t)b * a.H + y) * a.W + x;
  if constexpr (PX == 2) {  // W is even here, so x + 1 < W
    if (a.bkg) *reinterpret_cast<double2*>(a.bkg + o) = make_double2(vb[0], vb[1]);
    if (a.rms) *reinterpret_cast<double2*>(a.rms + o) = make_double2(vr[0], vr[1]);
  } else {
    if (a.bkg) a.bkg[o] = vb[0];
    if (a.rms) a.rms[o] = vr[0];
  }
}

// ------------------------------------------------------------------ launches
hipError_t launch_bkg_boxstats(const BkgArgs& a, int f32, hipStream_t s) {
  const dim3 grid(a.ny * a.nx, a.B), block(256);
  size_t P = 1;
  while (P < (size_t)a.bh * a.bw) P <<= 1;
  // dynamic LDS: a small box leaves room for more workgroups per CU
  if (f32)
    hipLaunchKernelGGL(k_bkg_boxstats<float>, grid, block, P * sizeof(double), s, a);
  else
    hipLaunchKernelGGL(k_bkg_boxstats<double>, grid, block, P * sizeof(double), s, a);
  return hipGetLastError();
}

hipError_t launch_bkg_mesh(const BkgArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k_bkg_mesh, dim3(a.B), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_bkg_zoom(const BkgArgs& a, hipStream_t s) {
  const bool al = ((reinterpret_cast<uintptr_t>(a.bkg) | reinterpret_cast<uintptr_t>(a.rms)) & 15) == 0;
  if (a.W % 2 == 0 && al) {
    const dim3 grid((a.W + 511) / 512, a.H, a.B);
    hipLaunchKernelGGL(k_bkg_zoom<2>, grid, dim3(256), 0, s, a);
  } else {
    const dim3 grid((a.W + 255) / 256, a.H, a.B);
    hipLaunchKernelGGL(k_bkg_zoom<1>, grid, dim3(256), 0, s, a);
  }
  return hipGetLastError();
}

}  // namespace bsgp
