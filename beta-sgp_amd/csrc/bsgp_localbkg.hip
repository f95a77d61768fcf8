// bsgp_localbkg.hip — the local background of the source catalogue: what
// photutils' SourceCatalog(..., localbkg_width=L) (restoration/utils.py:244-246)
// measures around every source and subtracts from segment_flux, min_value and
// max_value (include/bsgp.h and DESIGN §3.8, L1 to L6).
//
//  k_localbkg  one workgroup per (label, image).  The group walks the outer
//              rectangle clipped to the image, tests L2 and compacts the
//              passing values into LDS (one LDS integer atomic per wave and
//              step; the order is free, the values are sorted next), pads to
//              a power of two with +inf, sorts, clips (bsgp_sigclip.hpp, the
//              code of the sky background's boxes) and takes SExtractor's
//              mode.  Every sum runs over the sorted range: a batch gives
//              each image the bits it gets alone.
//
// The launch runs the kernel twice, with 16 KiB and with 64 KiB of dynamic LDS:
// a label belongs to the launch whose capacity first holds the pixel count of
// its clipped annulus (its rectangles alone, before labels and non-finite
// pixels are looked at), so that the many small sources do not each hold the
// 64 KiB the largest annulus needs.
#include <hip/hip_runtime.h>

#include <cmath>

#include "bsgp_apps.hpp"
#include "bsgp_prims.hpp"
#include "bsgp_reduce.hpp"
#include "bsgp_sigclip.hpp"

namespace bsgp {

namespace {
constexpr int kLocalBkgSmall = 2048;  // values of the small launch
}

// lds_cap: the values this launch's LDS holds; a label whose annulus holds at
// most lds_min pixels belongs to the other launch (lds_min = -1: none does)
template <typename T>
__global__ void __launch_bounds__(256) k_localbkg(LocalBkgArgs a, int lds_min, int lds_cap) {
  extern __shared__ double s[];  // lds_cap values
  __shared__ double red[(kWaves + 1) * kMaxRed];
  __shared__ int count;
  const int tid = threadIdx.x, lane = tid & 63, row = blockIdx.x, b = blockIdx.y;
  int nl = a.nlabels ? a.nlabels[b] : a.cap;
  nl = nl < a.cap ? nl : a.cap;
  if (row >= nl) return;
  const size_t r = (size_t)b * a.cap + row;
  const int* ic = a.icols + r * 5;
  const int area = ic[0];
  if (area <= 0) return;
  const int x0 = ic[1], x1 = ic[2], y0 = ic[3], y1 = ic[4];

  // L1
  const double cx = ((double)x0 + (double)x1) / 2.0, cy = ((double)y0 + (double)y1) / 2.0;
  const double ix = 0.75 * ((double)x1 - (double)x0 + 1.0), iy = 0.75 * ((double)y1 - (double)y0 + 1.0);
  const double ox = ix + a.width, oy = iy + a.width;
  // the outer rectangle clipped to the image, a pixel wider than the strict
  // test admits: the test below decides
  const int xa = (int)fmax(0.0, floor(cx - ox)), xb = (int)fmin((double)(a.W - 1), ceil(cx + ox));
  const int ya = (int)fmax(0.0, floor(cy - oy)), yb = (int)fmin((double)(a.H - 1), ceil(cy + oy));
  if (xb < xa || yb < ya) {  // a box outside the image: no values
    if (tid == 0) atomicOr(a.status + b, BSGP_LOCALBKG_FEW);
    return;
  }
  const int rw = xb - xa + 1, rh = yb - ya + 1;
  // pixels strictly inside the inner rectangle (exact: multiples of 0.25)
  const int ia = (int)fmax((double)xa, floor(cx - ix) + 1.0), ib = (int)fmin((double)xb, ceil(cx + ix) - 1.0);
  const int ja = (int)fmax((double)ya, floor(cy - iy) + 1.0), jb = (int)fmin((double)yb, ceil(cy + iy) - 1.0);
  const int inner = (ib >= ia && jb >= ja) ? (ib - ia + 1) * (jb - ja + 1) : 0;
  const int bound = rw * rh - inner;  // rw * rh <= H * W < 2^31
  if (bound <= lds_min || (bound > lds_cap && lds_cap < kLocalBkgMax)) return;

  // L2: gather
  if (tid == 0) count = 0;
  __syncthreads();
  const size_t img_off = (size_t)b * a.H * a.W;
  const T* img = static_cast<const T*>(a.data) + img_off;
  const int* lab = a.labels + img_off;
  const int nrect = rw * rh;
  for (int k0 = 0; k0 < nrect; k0 += 256) {
    const int k = k0 + tid;
    bool pass = false;
    double u = 0.0;
    if (k < nrect) {
      const int yy = k / rw, y = ya + yy, x = xa + (k - yy * rw);
      const double dx = fabs((double)x - cx), dy = fabs((double)y - cy);
      if (dx < ox && dy < oy && !(dx < ix && dy < iy)) {
        const size_t o = (size_t)y * a.W + x;
        if (lab[o] == 0) {
          u = (double)img[o];
          pass = __builtin_isfinite(u);
        }
      }
    }
    const unsigned long long m = __ballot(pass);
    int base = 0;
    if (lane == 0 && m) base = atomicAdd(&count, __popcll(m));
    base = __shfl(base, 0, 64);
    if (pass) {
      const int idx = base + __popcll(m & ((1ULL << lane) - 1ULL));
      if (idx < lds_cap) s[idx] = u;
    }
  }
  __syncthreads();
  const int n = count;
  int* np = a.npix + r * 2;
  if (n > lds_cap) {  // over the cap (the large launch only): lb = 0, no correction
    if (tid == 0) {
      np[0] = n;
      atomicOr(a.status + b, BSGP_LOCALBKG_OVER_CAP);
    }
    return;
  }
  if (n < a.min_pixels) {  // L3
    if (tid == 0) {
      np[0] = n;
      atomicOr(a.status + b, BSGP_LOCALBKG_FEW);
    }
    return;
  }
  int P = 1;
  while (P < n) P <<= 1;
  for (int k = n + tid; k < P; k += 256) s[k] = dev_inf();
  __syncthreads();
  bkg_sort(s, P);

  // L4, L5
  const SigClip c = sigma_clip_sorted(s, n, a.sigma, a.maxiters, red);
  if (tid != 0) return;
  double lb;
  if (c.sd == 0.0)
    lb = c.mean;
  else if (fabs(c.mean - c.med) / c.sd < 0.3)
    lb = 2.5 * c.med - 1.5 * c.mean;
  else
    lb = c.med;
  a.lb[r] = lb;
  np[0] = n;
  np[1] = c.hi - c.lo;
  if (a.apply) {  // L6
    double* fc = a.fcols + r * 8;
    fc[0] = fc[0] - (double)area * lb;
    fc[1] = fc[1] - lb;
    fc[2] = fc[2] - lb;
  }
}

hipError_t launch_localbkg(const LocalBkgArgs& a, int f32, hipStream_t s) {
  const dim3 grid(a.cap, a.B), block(256);
  auto* kern = f32 ? k_localbkg<float> : k_localbkg<double>;
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                                     hipFuncAttributeMaxDynamicSharedMemorySize,
                                     kLocalBkgMax * (int)sizeof(double));
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(kern, grid, block, kLocalBkgSmall * sizeof(double), s, a, -1, kLocalBkgSmall);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(kern, grid, block, kLocalBkgMax * sizeof(double), s, a, kLocalBkgSmall,
                     kLocalBkgMax);
  return hipGetLastError();
}

}  // namespace bsgp
