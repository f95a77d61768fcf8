// bsgp_stamps.hip — the metrics the star-stamp application computes for the
// observed and the restored stamp (restoration/application_sgp_star_stamps.py:
// 117-142), on the device:
//
//  k_radprof      utils.radial_profile (restoration/utils.py:81-92).  One wave
//                 per image, one lane per bin (up to four bins per lane): the
//                 wave stages 256 pixels and their bin numbers in LDS, then
//                 every lane walks them in raster order and adds the pixels of
//                 its own bins.  A bin's sum is therefore numpy.bincount's,
//                 bit for bit: the same additions in the same order.
//  k_fit_gauss1d  utils.fit_radprof (utils.py:180-202): MINPACK's lmder
//                 (bsgp_lmder.hpp) on one wave per profile, vectors in LDS.
//  k_w1           utils.wasserstein_distance_norm (utils.py:276-291), that is
//                 scipy.stats.wasserstein_distance of two unweighted samples:
//                 one wave sorts the merged values in LDS (bitonic), then adds
//                 |F_u - F_v| dt over them in ascending order.
//
// No floating-point atomics, no reduction whose order depends on the batch:
// an image gets the bits it gets alone.
#include <hip/hip_runtime.h>

#include "bsgp_apps.hpp"
#include "bsgp_prims.hpp"
#include "bsgp_reduce.hpp"

#define LM_FN __device__ __forceinline__
#define LM_LANE ((int)threadIdx.x)
#define LM_NL 64
#define LM_SYNC() bsgp::wave_sync()
#define LM_SUM(v) bsgp::wave_sum(v)
#define LM_MAX(v) bsgp::wave_ext<true>(v)
#include "bsgp_lmder.hpp"

namespace bsgp {

namespace {

constexpr int kTile = 256;  // pixels staged per round of k_radprof

// NCH: bins per lane (bin = lane + 64 c); rcap <= 64 NCH
template <int NCH, typename T>
__global__ void __launch_bounds__(64) k_radprof(StampProfArgs a) {
  __shared__ double tv[kTile];
  __shared__ int tk[kTile];
  const int b = blockIdx.x, lane = threadIdx.x;
  const int HW = a.H * a.W;
  const T* img = static_cast<const T*>(a.data) + (size_t)b * HW;
  const double c0 = a.centers[2 * b], c1 = a.centers[2 * b + 1];
  double acc[NCH];
  int cnt[NCH];
#pragma unroll
  for (int c = 0; c < NCH; ++c) acc[c] = 0.0, cnt[c] = 0;
  int kmax = -1;
  for (int base = 0; base < HW; base += kTile) {
    wave_sync();
#pragma unroll
    for (int t = 0; t < kTile / 64; ++t) {
      const int p = base + t * 64 + lane;
      if (p < HW) {
        const int i = p / a.W, j = p - i * a.W;
        // center[0] is measured along the rows, as the reference's
        // np.indices order has it (utils.py:85-86)
        const double di = (double)i - c0, dj = (double)j - c1;
        const int k = (int)sqrt(di * di + dj * dj);
        kmax = k > kmax ? k : kmax;
        tv[t * 64 + lane] = (double)img[p];
        tk[t * 64 + lane] = k;
      }
    }
    wave_sync();
    const int n = HW - base < kTile ? HW - base : kTile;
    for (int q = 0; q < n; ++q) {
      const int k = tk[q];
      const double v = tv[q];
#pragma unroll
      for (int c = 0; c < NCH; ++c)
        if (k == lane + 64 * c) acc[c] += v, ++cnt[c];
    }
  }
  kmax = wave_max(kmax);
  const int len = kmax + 1;
  if (lane == 0) a.len[b] = len;
  double* out = a.prof + (size_t)b * a.rcap;
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int k = lane + 64 * c;
    if (k < a.rcap) out[k] = k < len ? acc[c] / (double)cnt[c] : dev_nan();
  }
}

__global__ void __launch_bounds__(64) k_fit_gauss1d(StampFitArgs a) {
  extern __shared__ __attribute__((aligned(16))) char bsgp_dyn_lds[];
  const int b = blockIdx.x, lane = threadIdx.x;
  const int ld = a.rcap;
  bsgp_lm::Work w;
  w.y = reinterpret_cast<double*>(bsgp_dyn_lds);
  w.fvec = w.y + ld;
  w.wa4 = w.fvec + ld;
  w.fjac = w.wa4 + ld;
  w.ld = ld;
  double* sm = w.fjac + 3 * ld;
  w.x = sm, w.diag = sm + 3, w.qtf = sm + 6, w.wa1 = sm + 9, w.wa2 = sm + 12, w.wa3 = sm + 15;
  w.sdiag = sm + 18, w.xs = sm + 21, w.wq = sm + 24;
  w.ipvt = reinterpret_cast<int*>(sm + bsgp_lm::kSmallDoubles);
  const int m = a.len[b];
  const double* y = a.prof + (size_t)b * a.rcap;
  for (int i = lane; i < ld; i += 64) w.y[i] = (i < m) ? y[i] : 0.0;
  wave_sync();
  bsgp_lm::fit_gauss1d(w, m, a.rcap, a.fwhm[b], a.fitted + (size_t)b * a.rcap, a.params + 3 * (size_t)b,
                       a.perr + 3 * (size_t)b, a.info + 2 * (size_t)b);
}

__global__ void __launch_bounds__(64) k_w1(StampW1Args a) {
  extern __shared__ __attribute__((aligned(16))) char bsgp_dyn_lds[];
  double* val = reinterpret_cast<double*>(bsgp_dyn_lds);
  int* tag = reinterpret_cast<int*>(val + a.P);
  const int b = blockIdx.x, lane = threadIdx.x;
  const int n = a.ulen ? a.ulen[b] : a.rcap, m = a.vlen ? a.vlen[b] : a.rcap;
  if (n < 1 || m < 1 || n > a.rcap || m > a.rcap) {
    if (lane == 0) a.out[b] = dev_nan();
    return;
  }
  const double* u = a.u + (size_t)b * a.rcap;
  const double* v = a.v + (size_t)b * a.rcap;
  const double inf = dev_inf();
  int bad = 0;
  for (int i = lane; i < a.P; i += 64) {
    double x = inf;
    int t = 2;
    if (i < n) x = u[i], t = 0;
    else if (i < n + m) x = v[i - n], t = 1;
    if (t < 2 && !(fabs(x) < inf)) bad = 1;
    val[i] = x;
    tag[i] = t;
  }
  bad = wave_max(bad);
  if (bad) {
    if (lane == 0) a.out[b] = dev_nan();
    return;
  }
  wave_sync();
  for (int k = 2; k <= a.P; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = lane; i < a.P; i += 64) {
        const int p = i ^ j;
        if (p > i) {
          const double x = val[i], y = val[p];
          if ((x > y) == ((i & k) == 0)) {
            const int tx = tag[i], ty = tag[p];
            val[i] = y, val[p] = x;
            tag[i] = ty, tag[p] = tx;
          }
        }
      }
      wave_sync();
    }
  }
  // every lane alike: the terms in ascending order.  The counts at position q
  // are those of the values up to q; between equal values dt is 0, so the term
  // is 0 as it is with the counts of all values <= t.
  int cu = 0, cv = 0;
  double sum = 0.0;
  const double dn = (double)n, dm = (double)m;
  for (int q = 0; q + 1 < n + m; ++q) {
    const int t = tag[q];
    cu += t == 0;
    cv += t == 1;
    const double dt = val[q + 1] - val[q];
    sum += fabs((double)cu / dn - (double)cv / dm) * dt;
  }
  if (lane == 0) a.out[b] = sum;
}

template <typename T>
hipError_t launch_radprof_t(const StampProfArgs& a, hipStream_t s) {
  const dim3 grid(a.B), block(64);
  if (a.rcap <= 64) hipLaunchKernelGGL((k_radprof<1, T>), grid, block, 0, s, a);
  else if (a.rcap <= 128) hipLaunchKernelGGL((k_radprof<2, T>), grid, block, 0, s, a);
  else hipLaunchKernelGGL((k_radprof<4, T>), grid, block, 0, s, a);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_stamp_radprof(const StampProfArgs& a, int f32, hipStream_t s) {
  return f32 ? launch_radprof_t<float>(a, s) : launch_radprof_t<double>(a, s);
}

hipError_t launch_stamp_fit(const StampFitArgs& a, hipStream_t s) {
  const size_t lds = (6 * (size_t)a.rcap + bsgp_lm::kSmallDoubles) * sizeof(double) + 4 * sizeof(int);
  hipLaunchKernelGGL(k_fit_gauss1d, dim3(a.B), dim3(64), lds, s, a);
  return hipGetLastError();
}

hipError_t launch_stamp_w1(const StampW1Args& a, hipStream_t s) {
  const size_t lds = (size_t)a.P * (sizeof(double) + sizeof(int));
  hipLaunchKernelGGL(k_w1, dim3(a.B), dim3(64), lds, s, a);
  return hipGetLastError();
}

}  // namespace bsgp
