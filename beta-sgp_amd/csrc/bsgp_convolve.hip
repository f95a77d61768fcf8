// bsgp_convolve.hip — astropy.convolution.convolve on the device for kernels
// the size of a PSF (odd, up to kConvMaxKernel per axis): boundary='fill' with
// any fill value, nan_treatment 'interpolate' and 'fill', a mask,
// preserve_nan and normalize_kernel (include/bsgp.h bsgp_convolve2d_ex,
// DESIGN §3.12).  What restoration/utils.py's degrade and scale_psf call.
//
//  k_conv_scan  one flag per image: it holds a NaN or a masked pixel
//               (an integer OR into the image's status word).
//  k_conv       one workgroup per output tile of 4R rows x 64 columns.  The
//               tile and its halo are staged once in LDS as float64 (widened,
//               masked pixels as NaN, NaNs as the fill value under 'fill',
//               pixels outside the image as the fill value).  A wave owns R
//               rows of the tile, a lane one column: a thread carries R
//               output pixels, each its own chain of rounded products and
//               sums.  One LDS value P[s][x + j] serves the R pixels as tap
//               (s - r, j) of pixel r, so every pixel still sees its taps in
//               row-major order of its window (i outer, j inner) and
//               multiplies tap (i, j) by K[kh-1-i][kw-1-j].  The kernel's
//               entries are uniform over the workgroup and read from global
//               memory by address, not staged.
//
// No floating-point atomics and no sum shared between pixels: a batch gives
// each image the bits it gets alone, and every run gives the same bits.
#include <hip/hip_runtime.h>

#include "bsgp_apps.hpp"
#include "bsgp_layout.hpp"
#include "bsgp_prims.hpp"

namespace bsgp {

namespace {

constexpr int kConvTileW = 64;  // columns of a tile: one per lane
constexpr int kConvWaves = 4;   // waves of a workgroup, R rows each
// dynamic LDS of one workgroup: two workgroups share a CU (less what the
// allocation granularity and the runtime may take)
constexpr size_t kConvLdsMax = layout::kLdsPerCu / 2 - 1024;

constexpr size_t conv_lds_bytes(int R, int kh, int kw) {
  return (size_t)(kConvWaves * R + kh - 1) * (size_t)(kConvTileW + kw - 1) * sizeof(double);
}
static_assert(conv_lds_bytes(1, kConvMaxKernel, kConvMaxKernel) <= kConvLdsMax,
              "the largest kernel's smallest tile must fit the LDS budget");


// one tap of one pixel: top += v * k (and bot += k), skipped for a NaN value
// on the interpolating path
template <bool NANP>
__device__ __forceinline__ void conv_tap(double& top, double& bot, double v, double k) {
  const double t = __dadd_rn(top, __dmul_rn(v, k));
  if (NANP) {
    const bool ok = v == v;
    const double u = __dadd_rn(bot, k);
    top = ok ? t : top;
    bot = ok ? u : bot;
  } else {
    top = t;
  }
}

// all taps of the thread's R pixels.  P: the thread's LDS column at the first
// row of its wave; LDS row s holds tap row i = s - r of pixel r.
template <int R, bool NANP>
__device__ __forceinline__ void conv_taps(const double* P, int LW, const double* __restrict__ K,
                                          int kh, int kw, double (&top)[R], double (&bot)[R]) {
  for (int s = 0; s < kh + R - 1; ++s) {
    const double* row = P + s * LW;
    // K[kh-1-i][kw-1-j] at i = s - r: kr[r * kw - j]
    const double* kr = K + (kh - 1 - s) * kw + (kw - 1);
    if (s >= R - 1 && s < kh) {  // the row is a tap row of all R pixels
#pragma unroll 4
      for (int j = 0; j < kw; ++j) {
        const double v = row[j];
#pragma unroll
        for (int r = 0; r < R; ++r) conv_tap<NANP>(top[r], bot[r], v, kr[r * kw - j]);
      }
    } else {
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const int i = s - r;
        if (i < 0 || i >= kh) continue;
        for (int j = 0; j < kw; ++j) conv_tap<NANP>(top[r], bot[r], row[j], kr[r * kw - j]);
      }
    }
  }
}

}  // namespace

template <typename T>
__global__ void __launch_bounds__(256) k_conv_scan(const T* data, const unsigned char* mask, int hw,
                                                   int* status) {
  const int b = blockIdx.y;
  const T* img = data + (size_t)b * hw;
  const unsigned char* m = mask ? mask + (size_t)b * hw : nullptr;
  bool f = false;
  for (size_t p = (size_t)blockIdx.x * 256 + threadIdx.x; p < (size_t)hw;
       p += (size_t)gridDim.x * 256) {
    const T v = img[p];
    f |= (v != v) || (m && m[p]);
  }
  if (__any(f) && (threadIdx.x & 63) == 0) atomicOr(status + b, BSGP_CONV_HAD_NAN);
}

template <typename T, int R>
__global__ void __launch_bounds__(256) k_conv(ConvArgs a) {
  extern __shared__ double P[];  // [4R + kh - 1][64 + kw - 1]
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, b = blockIdx.y;
  const int ty0 = (int)(blockIdx.x / (unsigned)a.ntx) * (kConvWaves * R);
  const int tx0 = (int)(blockIdx.x % (unsigned)a.ntx) * kConvTileW;
  const int py = a.kh / 2, px = a.kw / 2;
  const int LH = kConvWaves * R + a.kh - 1, LW = kConvTileW + a.kw - 1;
  const size_t base = (size_t)b * a.H * a.W;
  const T* img = static_cast<const T*>(a.data) + base;
  const unsigned char* mask = a.mask ? a.mask + base : nullptr;
  const bool fill_nan = (a.flags & BSGP_CONV_F_FILL) != 0;
  const double fill = a.fill_value;

  for (int ly = w; ly < LH; ly += kConvWaves) {
    const int gy = ty0 - py + ly;
    const bool rowok = gy >= 0 && gy < a.H;
    for (int lx = lane; lx < LW; lx += 64) {
      const int gx = tx0 - px + lx;
      double v = fill;
      if (rowok && gx >= 0 && gx < a.W) {
        const size_t p = (size_t)gy * a.W + gx;
        v = (double)img[p];
        if (mask && mask[p]) v = dev_nan();
        if (fill_nan && v != v) v = fill;
      }
      P[ly * LW + lx] = v;
    }
  }
  __syncthreads();

  const bool nanp = !fill_nan && (a.status[b] & BSGP_CONV_HAD_NAN);
  const double* __restrict__ K = a.kernel + (size_t)b * a.kernel_stride;
  const double* mine = P + (w * R) * LW + lane;
  double top[R], bot[R];
#pragma unroll
  for (int r = 0; r < R; ++r) top[r] = 0.0, bot[r] = 0.0;
  if (nanp)
    conv_taps<R, true>(mine, LW, K, a.kh, a.kw, top, bot);
  else
    conv_taps<R, false>(mine, LW, K, a.kh, a.kw, top, bot);

  const double ksum = a.kernel_sum[a.kernel_stride ? b : 0];
  const bool norm = (a.flags & BSGP_CONV_F_NORMALIZE) != 0;
  const bool preserve = (a.flags & BSGP_CONV_F_PRESERVE_NAN) != 0;
  const int x = tx0 + lane;
  bool left = false;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int y = ty0 + w * R + r;
    if (x >= a.W || y >= a.H) continue;
    const size_t p = (size_t)y * a.W + x;
    double o;
    if (nanp) {
      o = bot[r] == 0.0 ? mine[(r + py) * LW + px] : top[r] / bot[r];
      if (!norm) o = __dmul_rn(o, ksum);
    } else {
      o = norm ? top[r] / ksum : top[r];
    }
    const T v = img[p];
    const bool was_nan = (v != v) || (mask && mask[p]);
    if (preserve && was_nan) o = dev_nan();
    left |= (o != o) && !(preserve && was_nan);
    a.out[base + p] = o;
  }
  if (__any(left) && lane == 0) atomicOr(a.status + b, BSGP_CONV_NAN_LEFT);
}

namespace {

template <typename T, int R>
hipError_t conv_launch(ConvArgs a, hipStream_t s) {
  const size_t lds = conv_lds_bytes(R, a.kh, a.kw);
  auto* kern = k_conv<T, R>;
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)kConvLdsMax);
  if (e != hipSuccess) return e;
  const int nty = (a.H + kConvWaves * R - 1) / (kConvWaves * R);
  a.ntx = (a.W + kConvTileW - 1) / kConvTileW;
  const dim3 grid((unsigned)((int64_t)a.ntx * nty), a.B), block(256);
  hipLaunchKernelGGL(kern, grid, block, lds, s, a);
  return hipGetLastError();
}

template <typename T>
hipError_t conv_launch_r(const ConvArgs& a, int R, hipStream_t s) {
  switch (R) {
    case 8: return conv_launch<T, 8>(a, s);
    case 4: return conv_launch<T, 4>(a, s);
    case 2: return conv_launch<T, 2>(a, s);
    default: return conv_launch<T, 1>(a, s);
  }
}

}  // namespace

// rows per thread: the most the LDS budget admits, and no more than the image
// needs (a low image gets lower tiles and so more of them)
int conv_rows_per_thread(int H, int kh, int kw) {
  int R = 8;
  while (R > 1 && (conv_lds_bytes(R, kh, kw) > kConvLdsMax || kConvWaves * (R / 2) >= H)) R /= 2;
  return R;
}

int64_t conv_tiles(int H, int W, int kh, int kw) {
  const int th = kConvWaves * conv_rows_per_thread(H, kh, kw);
  return (int64_t)((H + th - 1) / th) * ((W + kConvTileW - 1) / kConvTileW);
}

hipError_t launch_convolve(const ConvArgs& a, int f32, hipStream_t s) {
  hipError_t e = hipMemsetAsync(a.status, 0, (size_t)a.B * sizeof(int), s);
  if (e != hipSuccess) return e;
  const int hw = a.H * a.W;
  const int64_t want = ((int64_t)hw + 256 * 8 - 1) / (256 * 8);  // 8 pixels per thread
  const int nb = want > 1024 ? 1024 : (int)want;
  const dim3 sgrid(nb, a.B), block(256);
  if (f32)
    hipLaunchKernelGGL(k_conv_scan<float>, sgrid, block, 0, s, static_cast<const float*>(a.data),
                       a.mask, hw, a.status);
  else
    hipLaunchKernelGGL(k_conv_scan<double>, sgrid, block, 0, s, static_cast<const double*>(a.data),
                       a.mask, hw, a.status);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  const int R = conv_rows_per_thread(a.H, a.kh, a.kw);
  return f32 ? conv_launch_r<float>(a, R, s) : conv_launch_r<double>(a, R, s);
}

}  // namespace bsgp
