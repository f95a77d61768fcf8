// bsgp_sigclip.hpp — the sort and the sigma clipping that the box statistics of
// the sky background (bsgp_background.hip) and the local
// background of the source catalogue (bsgp_localbkg.hip) share:
// astropy's SigmaClip(cenfunc='median', stdfunc='std') on values sorted once in
// LDS, where clipping only moves the two ends [lo, hi) of the sorted range.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

#include "bsgp_prims.hpp"
#include "bsgp_reduce.hpp"

namespace bsgp {

// ascending bitonic sort of s[0, P) in LDS, P a power of two, 256 threads
__device__ __forceinline__ void bkg_sort(double* s, int P) {
  for (int k = 2; k <= P; k <<= 1) {
    for (int jj = k >> 1; jj > 0; jj >>= 1) {
      for (int t = threadIdx.x; t < (P >> 1); t += 256) {
        const int lo_i = 2 * t - (t & (jj - 1)), hi_i = lo_i + jj;
        const bool up = (lo_i & k) == 0;
        const double x = s[lo_i], y = s[hi_i];
        if ((x > y) == up) {
          s[lo_i] = y;
          s[hi_i] = x;
        }
      }
      __syncthreads();
    }
  }
}

// What sigma clipping leaves of the sorted values s[0, nvalid), nvalid >= 1:
// the range [lo, hi), the iterations run (the last may remove nothing), and the
// median, mean and population standard deviation of the survivors.  Bounds are
// inclusive (median -+ sigma * std).  Every thread of the 256 gets the same
// result; red: (kWaves + 1) * kMaxRed doubles of LDS.
struct SigClip {
  int lo, hi, it;
  double med, mean, sd;
};

__device__ __forceinline__ SigClip sigma_clip_sorted(const double* s, int nvalid, double sigma,
                                                     int maxiters, double* red) {
  const int tid = threadIdx.x;
  int lo = 0, hi = nvalid, it = 0;
  bool more = maxiters > 0;
  double med, mean, sd;
  for (;;) {
    const int n = hi - lo;
    med = (n & 1) ? s[lo + n / 2] : (s[lo + n / 2 - 1] + s[lo + n / 2]) / 2.0;
    double v[1] = {0.0};
    for (int k = lo + tid; k < hi; k += 256) v[0] += s[k];
    block_sum<1>(v, red);
    mean = v[0] / (double)n;
    v[0] = 0.0;
    for (int k = lo + tid; k < hi; k += 256) {
      const double d = s[k] - mean;
      v[0] += d * d;
    }
    block_sum<1>(v, red);
    sd = sqrt(v[0] / (double)n);
    if (!more) break;
    const double lb = med - sd * sigma, ub = med + sd * sigma;
    int l = lo, r = hi;
    while (l < r) {  // first value >= lb
      const int m = (l + r) >> 1;
      if (s[m] < lb) l = m + 1; else r = m;
    }
    const int nlo = l;
    r = hi;
    while (l < r) {  // first value > ub
      const int m = (l + r) >> 1;
      if (s[m] <= ub) l = m + 1; else r = m;
    }
    const int nhi = l;
    ++it;
    if (nhi <= nlo) {  // a sigma so small that nothing is left: NaN, as numpy of no values
      lo = hi = nlo;
      med = mean = sd = dev_nan();
      break;
    }
    const bool changed = nlo != lo || nhi != hi;
    lo = nlo;
    hi = nhi;
    if (!changed) break;
    more = it < maxiters;
  }
  return SigClip{lo, hi, it, med, mean, sd};
}

}  // namespace bsgp
