// bsgp_match.hip — the cross-match of two source catalogues by position: the
// greedy symmetric best match within max_sep that the reference's published
// tables results/*_MATCHED.csv hold (include/bsgp.h and DESIGN §3.10, M1 to
// M6).
//
//  k_match<LDS>  one workgroup per image pair, every round inside the kernel,
//                workgroup barriers only.  The rows of both catalogues share
//                one index space: catalogue 1 at 0, catalogue 2 at the next
//                multiple of 64, so that a wave scans one catalogue.  Per row:
//                (x, y), best (the partner the row picked, or -1) and match.
//                A row that takes no part (M1), or is taken, has x = NaN: its
//                d2 is NaN and fails the one comparison of the scan, which
//                therefore reads nothing but the 16 bytes of (x, y) per pair,
//                every lane of a wave at the same address (a broadcast).
//                Round 1 scans every row; a later round rescans only the rows
//                whose partner was taken by another row: an untaken partner is
//                still the best of fewer candidates.
//                LDS = true keeps the rows in dynamic LDS (24 bytes per row),
//                LDS = false in the caller's workspace in global memory.
//
// x - y and y - x are negatives of each other in IEEE arithmetic and square to
// the same bits, so both catalogues' scans evaluate M2's d2 with the row's own
// coordinates on the left.
#include <hip/hip_runtime.h>

#include "bsgp_apps.hpp"
#include "bsgp_prims.hpp"

#pragma clang fp contract(off)

namespace bsgp {

namespace {


__device__ __forceinline__ double match_d2(const double2 p, const double2 q) {
  const double dx = p.x - q.x, dy = p.y - q.y;
  return __dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy));
}

// M1: stages the rows of one catalogue and returns the status bits this lane met
__device__ __forceinline__ int match_stage(const MatchCat& c, int b, int n, int lo, int hi, int tid, int nt,
                                  double2* xy, int* best, int* match) {
  int st = 0;
  for (int r = lo + tid; r < hi; r += nt) {
    const int i = r - lo;
    double2 p{dev_nan(), dev_nan()};
    if (i < n) {
      const size_t e = (size_t)b * c.cap + i;
      if (!c.valid || c.valid[e * c.vstride] > 0) {
        const double x = c.x[e * c.stride], y = c.y[e * c.stride];
        if (__builtin_isfinite(x) && __builtin_isfinite(y))
          p.x = x, p.y = y;
        else
          st = BSGP_MATCH_NONFINITE;
      }
    }
    xy[r] = p;
    best[r] = -1;
    match[r] = -1;
  }
  return st;
}

}  // namespace

template <bool LDS>
__global__ void __launch_bounds__(1024) k_match(MatchArgs a) {
  extern __shared__ double2 s_rows[];
  __shared__ int s_status, s_pairs;
  const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
  int n1 = a.c1.n ? a.c1.n[b] : a.c1.cap, n2 = a.c2.n ? a.c2.n[b] : a.c2.cap;
  int st = (n1 > a.c1.cap || n2 > a.c2.cap) ? BSGP_MATCH_OVER_CAP : 0;
  n1 = n1 < 0 ? 0 : (n1 < a.c1.cap ? n1 : a.c1.cap);
  n2 = n2 < 0 ? 0 : (n2 < a.c2.cap ? n2 : a.c2.cap);
  const int R1 = (n1 + 63) & ~63, rows = R1 + n2;  // <= match_rows(cap1, cap2)
  const int cap_rows = match_rows(a.c1.cap, a.c2.cap);
  double2* xy;
  int* best;
  if constexpr (LDS) {
    xy = s_rows;
    best = reinterpret_cast<int*>(s_rows + cap_rows);
  } else {
    xy = reinterpret_cast<double2*>(a.ws_xy) + (size_t)b * cap_rows;
    best = a.ws_state + (size_t)b * 2 * cap_rows;
  }
  int* match = best + cap_rows;

  if (tid == 0) s_status = 0, s_pairs = 0;
  st |= match_stage(a.c1, b, n1, 0, R1, tid, nt, xy, best, match);
  st |= match_stage(a.c2, b, n2, R1, rows, tid, nt, xy, best, match);
  double* sep1 = a.sep1 + (size_t)b * a.c1.cap;
  for (int i = tid; i < a.c1.cap; i += nt) sep1[i] = dev_nan();  // row i's lane also accepts it
  __syncthreads();
  if (st) atomicOr(&s_status, st);

  int mine = 0;
  const int max_rounds = (n1 < n2 ? n1 : n2) + 1;  // M4: the last one accepts nothing
  for (int round = 0; round < max_rounds; ++round) {
    for (int r = tid; r < rows; r += nt) {
      if (match[r] != -1) continue;
      const double2 p = xy[r];
      if (p.x != p.x) continue;  // takes no part
      const bool two = r >= R1;
      if (round) {  // rescan only a row whose partner was taken by another row
        const int o = best[r];
        if (o < 0 || match[two ? o : R1 + o] == -1) continue;
      }
      const double2* q = two ? xy : xy + R1;
      const int nq = two ? n1 : n2;
      double bd = a.d2_lim;
      int bj = -1;
#pragma unroll 4
      for (int j = 0; j < nq; ++j) {  // ascending: the first of equal d2 stays (M3)
        const double d2 = match_d2(p, q[j]);
        if (d2 < bd) bd = d2, bj = j;
      }
      best[r] = bj;
    }
    __syncthreads();
    int acc = 0;
    for (int i = tid; i < n1; i += nt) {
      if (match[i] != -1) continue;
      const int j = best[i];
      if (j < 0 || best[R1 + j] != i) continue;
      sep1[i] = __dsqrt_rn(match_d2(xy[i], xy[R1 + j]));
      match[i] = j;
      match[R1 + j] = i;
      xy[i].x = dev_nan();
      xy[R1 + j].x = dev_nan();
      acc = 1;
      ++mine;
    }
    if (!__syncthreads_or(acc)) break;
  }

  if (mine) atomicAdd(&s_pairs, mine);
  int* m1 = a.match1 + (size_t)b * a.c1.cap;
  int* m2 = a.match2 + (size_t)b * a.c2.cap;
  for (int i = tid; i < a.c1.cap; i += nt) m1[i] = i < n1 ? match[i] : -1;
  for (int j = tid; j < a.c2.cap; j += nt) m2[j] = j < n2 ? match[R1 + j] : -1;
  __syncthreads();
  if (tid == 0) a.npairs[b] = s_pairs, a.status[b] = s_status;
}

hipError_t launch_match(const MatchArgs& a, int B, bool lds, int block, hipStream_t s) {
  const size_t bytes = lds ? (size_t)match_rows(a.c1.cap, a.c2.cap) * kMatchRowBytes : 0;
  if (lds) {
    // the largest launch: cap1 + cap2 = kMatchLdsMax with 63 rows of padding
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_match<true>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)((kMatchLdsMax + 63) * kMatchRowBytes));
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_match<true>, dim3(B), dim3(block), bytes, s, a);
  } else {
    hipLaunchKernelGGL(k_match<false>, dim3(B), dim3(block), 0, s, a);
  }
  return hipGetLastError();
}

}  // namespace bsgp
