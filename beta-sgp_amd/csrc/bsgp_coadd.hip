// bsgp_coadd.hip — the background-matched co-add of subdivision tiles: what
// reproject_and_coadd(..., match_background=True) computes for tiles on one
// pixel grid (restoration/utils.py:392-397; include/bsgp.h and DESIGN §3.2,
// B1 to B4).  The pairs of overlapping tiles, their adjacency lists and the
// connected components (B1) are integer geometry and come from the host.
//
//  k_pair_offsets       B2, one workgroup per pair: the median of
//                       tile_i - tile_j over the intersection rectangle by a
//                       radix select on the order-preserving 64-bit key of
//                       the difference, eight passes of one byte, most
//                       significant first.  Every pass recomputes the
//                       differences from the two tiles (linear index over the
//                       rectangle, column fastest: lanes read along tile rows)
//                       and counts the byte of those that still carry the
//                       selected prefix in a 256-bin LDS histogram.  No scratch
//                       buffer, no cap on the overlap, one path from 1 pixel
//                       to a whole tile.  The passes leave the number of
//                       values below and equal to the lower middle value, so
//                       the upper middle value of an even count is either the
//                       same value or, from one more pass, the smallest value
//                       above it.
//  k_solve_corrections  B3, one workgroup: conjugate gradients on L c = b from
//                       c = 0 (L the graph Laplacian over the pairs with a
//                       finite offset, b_i = sum_j O_ij).  From c = 0 every
//                       iterate stays in the range of L, which is the
//                       zero-mean-per-component subspace: the limit is the
//                       minimum-norm least-squares solution.  Rows are walked
//                       through the adjacency lists by their owner thread, the
//                       dot products are reduced in a fixed order: no atomics,
//                       the same bits every run.  The search direction lives in
//                       LDS (neighbours gather from it), c / r / L p of a row
//                       only ever meet their owner thread and live in global
//                       memory.
//  coadd_tiles_matched_kernel   B4: coadd_tiles_kernel (bsgp_tiles.hip) with
//                       c_t taken off every value before it is added; the
//                       corrections are staged in LDS next to the box table.
#include <hip/hip_runtime.h>

#include "bsgp_apps.hpp"
#include "bsgp_prims.hpp"

#pragma clang fp contract(off)

namespace bsgp {

namespace {

constexpr int kCoaddBlock = 256;
constexpr int kCoaddWaves = kCoaddBlock / 64;

// Workgroup sum in a fixed order; every thread gets the total.
// (local: block_sum<1> of bsgp_reduce.hpp has a third barrier and grows k_solve_corrections' code)
__device__ __forceinline__ double coadd_block_sum(double v, double* red) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = red[0];
#pragma unroll
  for (int w = 1; w < kCoaddWaves; ++w) s += red[w];
  __syncthreads();
  return s;
}

}  // namespace

// ------------------------------------------------------------- B2 offsets
__global__ void __launch_bounds__(kCoaddBlock) k_pair_offsets(CoaddOffsetArgs a) {
  __shared__ unsigned int hist[256];
  __shared__ unsigned int wtot[kCoaddWaves];
  __shared__ unsigned long long s_prefix, s_min;
  __shared__ unsigned int s_rank, s_eq;
  __shared__ int s_bad;
  const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int ti = a.pairs[2 * p], tj = a.pairs[2 * p + 1];
  if (ti < 0 || ti >= a.n || tj < 0 || tj >= a.n) {  // not a pair of tiles: no offset
    if (tid == 0) a.offsets[p] = dev_nan();
    return;
  }
  const int xi = a.boxes[4 * ti], yi = a.boxes[4 * ti + 1];
  const int xj = a.boxes[4 * tj], yj = a.boxes[4 * tj + 1];
  // the intersection, kept inside both th x tw tiles whatever x1 / y1 say
  const int x0 = max(xi, xj), y0 = max(yi, yj);
  const int x1 = min(min(a.boxes[4 * ti + 2], a.boxes[4 * tj + 2]), min(xi, xj) + a.tw);
  const int y1 = min(min(a.boxes[4 * ti + 3], a.boxes[4 * tj + 3]), min(yi, yj) + a.th);
  const int rw = x1 - x0, rh = y1 - y0;
  if (rw <= 0 || rh <= 0) {
    if (tid == 0) a.offsets[p] = dev_nan();
    return;
  }
  const unsigned int cnt = (unsigned int)rw * (unsigned int)rh;  // th * tw < 2^31 (host)
  const double* pa = a.tiles + ((size_t)ti * a.th + (y0 - yi)) * a.tw + (x0 - xi);
  const double* pb = a.tiles + ((size_t)tj * a.th + (y0 - yj)) * a.tw + (x0 - xj);
  auto diff = [&](unsigned int e) {
    const unsigned int r = e / (unsigned int)rw, c = e - r * (unsigned int)rw;
    const size_t o = (size_t)r * a.tw + c;
    return pa[o] - pb[o];
  };

  hist[tid] = 0;
  if (tid == 0) s_bad = 0, s_min = ~0ULL;
  __syncthreads();
  unsigned long long prefix = 0;
  unsigned int rank = (cnt - 1) >> 1;  // the lower middle value (the middle one of an odd count)
  unsigned int below = 0, eq = cnt;    // values under the prefix, values carrying it
  for (int shift = 56; shift >= 0; shift -= 8) {
    const unsigned long long himask = shift == 56 ? 0ULL : ~0ULL << (shift + 8);
    for (unsigned int e0 = 0; e0 < cnt; e0 += kCoaddBlock) {
      const unsigned int e = e0 + tid;
      bool part = e < cnt;
      unsigned int digit = 0;
      if (part) {
        const double d = diff(e);
        if (shift == 56 && !__builtin_isfinite(d)) s_bad = 1;
        const unsigned long long k = order_key(d);
        part = (k & himask) == prefix;
        digit = (unsigned int)(k >> shift) & 255u;
      }
      // the leading bytes of a field's differences are nearly all equal: a wave
      // whose values share the byte adds its count once
      const unsigned long long m = __ballot(part);
      if (m) {
        const int first = __ffsll((long long)m) - 1;
        const unsigned int d0 = (unsigned int)__shfl((int)digit, first, 64);
        if (__all(!part || digit == d0)) {
          if (lane == first) atomicAdd(&hist[d0], (unsigned int)__popcll(m));
        } else if (part) {
          atomicAdd(&hist[digit], 1u);
        }
      }
    }
    __syncthreads();
    if (s_bad) break;  // (workgroup-uniform: read after the barrier)
    // the bin that holds the rank: inclusive scan of the 256 bins, one per thread
    // (inline: block_scan of bsgp_prims.hpp adds a total and a barrier, and changes the kernel's code)
    const unsigned int h = hist[tid];
    unsigned int inc = h;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const unsigned int u = (unsigned int)__shfl_up((int)inc, o, 64);
      if (lane >= o) inc += u;
    }
    if (lane == 63) wtot[w] = inc;
    __syncthreads();
    unsigned int base = 0;
    for (int k = 0; k < w; ++k) base += wtot[k];
    const unsigned int exc = base + inc - h;
    if (rank >= exc && rank < exc + h) {
      s_prefix = prefix | ((unsigned long long)tid << shift);
      s_rank = rank - exc;
      s_eq = h;
    }
    hist[tid] = 0;
    __syncthreads();
    below += rank - s_rank;
    prefix = s_prefix, rank = s_rank, eq = s_eq;
  }
  if (s_bad) {  // numpy's median would be NaN: the pair leaves the graph
    if (tid == 0) {
      a.offsets[p] = dev_nan();
      atomicOr(&a.status[ti], BSGP_COADD_NONFINITE);
      atomicOr(&a.status[tj], BSGP_COADD_NONFINITE);
    }
    return;
  }
  const double lo = order_value(prefix);
  double med = lo;
  if ((cnt & 1u) == 0) {
    double hi = lo;  // the upper middle value: rank cnt / 2
    if (below + eq <= cnt / 2) {  // ... lies above lo: the smallest such value
      unsigned long long mn = ~0ULL;
      for (unsigned int e = tid; e < cnt; e += kCoaddBlock) {
        const unsigned long long k = order_key(diff(e));
        if (k > prefix && k < mn) mn = k;
      }
      if (mn != ~0ULL) atomicMin(&s_min, mn);
      __syncthreads();
      hi = order_value(s_min);
    }
    med = (lo + hi) / 2.0;
  }
  if (tid == 0) a.offsets[p] = med;
}

// ---------------------------------------------------------- B3 corrections
__global__ void __launch_bounds__(kCoaddBlock) k_solve_corrections(CoaddSolveArgs a) {
  extern __shared__ double sp[];  // [n]: the search direction, then the corrections
  __shared__ double red[kCoaddWaves];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, n = a.n;
  double* r = a.ws;       // [n] residual
  double* q = a.ws + n;   // [n] L p
  double acc = 0.0;
  for (int i = tid; i < n; i += kCoaddBlock) {
    double b = 0.0;
    int deg = 0;
    for (int e = a.row_ptr[i]; e < a.row_ptr[i + 1]; ++e) {
      const double o = a.offsets[a.nbr_pair[e]];
      if (__builtin_isfinite(o)) {
        b += a.nbr_sign[e] < 0 ? -o : o;
        ++deg;
      }
    }
    a.c[i] = 0.0;
    r[i] = b;
    sp[i] = b;
    acc += b * b;
    if (deg == 0) a.status[i] |= BSGP_COADD_ISOLATED;
  }
  const double bb = coadd_block_sum(acc, red);  // (its barrier publishes sp)
  const double tol2 = kCoaddRtol * kCoaddRtol * bb;
  double rr = bb;
  int it = 0;
  while (rr > tol2 && it < n) {
    acc = 0.0;
    for (int i = tid; i < n; i += kCoaddBlock) {
      const double pi = sp[i];
      double s = 0.0;
      for (int e = a.row_ptr[i]; e < a.row_ptr[i + 1]; ++e)
        if (__builtin_isfinite(a.offsets[a.nbr_pair[e]])) s += pi - sp[a.nbr[e]];
      q[i] = s;
      acc += pi * s;
    }
    const double pq = coadd_block_sum(acc, red);
    if (!(pq > 0.0)) break;
    const double alpha = rr / pq;
    acc = 0.0;
    for (int i = tid; i < n; i += kCoaddBlock) {
      a.c[i] += alpha * sp[i];
      const double ri = r[i] - alpha * q[i];
      r[i] = ri;
      acc += ri * ri;
    }
    const double rn = coadd_block_sum(acc, red);  // (every row has gathered from sp by now)
    const double beta = rn / rr;
    for (int i = tid; i < n; i += kCoaddBlock) sp[i] = r[i] + beta * sp[i];
    rr = rn;
    ++it;
    __syncthreads();
  }
  const bool unconverged = rr > tol2;
  // rounding lets a component's mean drift from zero: take it off, one wave per
  // component, its members summed in index order
  for (int i = tid; i < n; i += kCoaddBlock) sp[i] = a.c[i];
  __syncthreads();
  for (int k = w; k < a.ncomp; k += kCoaddWaves) {
    double s = 0.0, m = 0.0;
    for (int i = lane; i < n; i += 64)
      if (a.component[i] == k) s += sp[i], m += 1.0;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o, 64), m += __shfl_xor(m, o, 64);
    if (m > 1.0) {  // (a tile alone in its component keeps its 0)
      const double mean = s / m;
      for (int i = lane; i < n; i += 64)
        if (a.component[i] == k) sp[i] -= mean;
    }
  }
  __syncthreads();
  // a tile every pair of which was dropped sits alone in the graph: exactly 0, like a tile
  // alone in its component
  for (int i = tid; i < n; i += kCoaddBlock)
    if (a.status[i] & BSGP_COADD_ISOLATED) sp[i] = 0.0;
  __syncthreads();
  const double ref = a.bref >= 0 ? sp[a.bref] : 0.0;
  for (int i = tid; i < n; i += kCoaddBlock) {
    a.c[i] = a.bref >= 0 ? sp[i] - ref : sp[i];
    if (unconverged) a.status[i] |= BSGP_COADD_NOT_CONVERGED;
  }
  if (tid == 0 && a.info) {
    a.info[0] = (double)it;
    a.info[1] = bb > 0.0 ? sqrt(rr / bb) : 0.0;
  }
}

// --------------------------------------------------------------- B4 mosaic
// coadd_tiles_kernel with the correction: mean = sum_t (tile_t - c_t) / count,
// tiles in index order.  CL: the corrections are staged in LDS in front of
// the box table (they fit next to it); else they are read where they are.
template <bool CL>
__global__ void __launch_bounds__(256) coadd_tiles_matched_kernel(const double* tiles, int n,
                                                                  int th, int tw,
                                                                  const int* boxes,
                                                                  const double* corr, int H, int W,
                                                                  double* mean, double* footprint) {
  extern __shared__ double smem[];
  double* scorr = smem;
  int* sbox = reinterpret_cast<int*>(smem + (CL ? n : 0));
  for (int i = threadIdx.x; i < 4 * n; i += 256) sbox[i] = boxes[i];
  if constexpr (CL)
    for (int i = threadIdx.x; i < n; i += 256) scorr[i] = corr[i];
  __syncthreads();
  const int64_t N = (int64_t)H * W;
  for (int64_t p = blockIdx.x * (int64_t)256 + threadIdx.x; p < N; p += (int64_t)gridDim.x * 256) {
    const int y = (int)(p / W), x = (int)(p % W);
    double s = 0.0;
    int cnt = 0;
    for (int t = 0; t < n; ++t) {
      const int x0 = sbox[4 * t], y0 = sbox[4 * t + 1], x1 = sbox[4 * t + 2], y1 = sbox[4 * t + 3];
      if (x >= x0 && x < x1 && y >= y0 && y < y1) {
        s += tiles[((size_t)t * th + (y - y0)) * tw + (x - x0)] - (CL ? scorr[t] : corr[t]);
        ++cnt;
      }
    }
    mean[p] = cnt ? s / cnt : 0.0;
    if (footprint) footprint[p] = (double)cnt;
  }
}

hipError_t launch_pair_offsets(const CoaddOffsetArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k_pair_offsets, dim3(a.npairs), dim3(kCoaddBlock), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_solve_corrections(const CoaddSolveArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k_solve_corrections, dim3(1), dim3(kCoaddBlock), (size_t)a.n * sizeof(double),
                     s, a);
  return hipGetLastError();
}

hipError_t launch_coadd_tiles_matched(const double* tiles, int n, int th, int tw, const int* boxes,
                                      const double* corr, int H, int W, double* mean,
                                      double* footprint, hipStream_t s) {
  const int64_t N = (int64_t)H * W;
  int64_t g = (N + 255) / 256;
  if (g > 8192) g = 8192;
  const size_t box_bytes = 4 * (size_t)n * sizeof(int), corr_bytes = (size_t)n * sizeof(double);
  const bool cl = box_bytes + corr_bytes <= (size_t)kCoaddLdsMax;
  const size_t lds = box_bytes + (cl ? corr_bytes : 0);
  const void* fn = cl ? reinterpret_cast<const void*>(coadd_tiles_matched_kernel<true>)
                      : reinterpret_cast<const void*>(coadd_tiles_matched_kernel<false>);
  hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, kCoaddLdsMax);
  if (e != hipSuccess) return e;
  if (cl)
    hipLaunchKernelGGL(coadd_tiles_matched_kernel<true>, dim3((unsigned)g), dim3(256), lds, s,
                       tiles, n, th, tw, boxes, corr, H, W, mean, footprint);
  else
    hipLaunchKernelGGL(coadd_tiles_matched_kernel<false>, dim3((unsigned)g), dim3(256), lds, s,
                       tiles, n, th, tw, boxes, corr, H, W, mean, footprint);
  return hipGetLastError();
}

}  // namespace bsgp
