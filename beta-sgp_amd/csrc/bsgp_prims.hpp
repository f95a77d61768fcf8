// bsgp_prims.hpp — the one copy of the small helpers the application kernels
// share: the quiet NaN and +infinity, the lock-free union-find, integer wave
// reductions, the 256-thread workgroup scan, the order-preserving key of a
// float64 and numpy's pairwise sums.  The BSGP_HD ones compile on the host
// too (tests/cpp/prims_test.cpp); the rest is device code.
#pragma once

#include <string.h>

#ifndef BSGP_HD  // as bsgp_fft.hpp defines it
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define BSGP_HD __host__ __device__ __forceinline__
#else
#define BSGP_HD inline
#endif
#endif

namespace bsgp {

// float64 bits -> a key that orders like the value (negatives flipped, sign bit set otherwise)
BSGP_HD unsigned long long order_key(double d) {
  unsigned long long u;
  memcpy(&u, &d, sizeof u);
  return (u >> 63) ? ~u : (u | 0x8000000000000000ULL);
}
BSGP_HD double order_value(unsigned long long k) {
  const unsigned long long u = (k >> 63) ? (k & 0x7fffffffffffffffULL) : ~k;
  double d;
  memcpy(&d, &u, sizeof d);
  return d;
}

// numpy's pairwise summation of a contiguous double array (what np.sum does):
// blocks of <= 128 with 8 accumulators, halves split at a multiple of 8,
// evaluated left half first.  Iterative (explicit stack).
// One leaf (n <= 128): a plain loop below 8, else 8 strided accumulators folded
// as ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)) and the remainder added.
BSGP_HD double np_pairwise_block(const double* a, int n) {
  if (n < 8) {
    double r = 0.0;
    for (int i = 0; i < n; ++i) r += a[i];
    return r;
  }
  double r[8];
  for (int j = 0; j < 8; ++j) r[j] = a[j];
  int i = 8;
  for (; i < n - (n % 8); i += 8)
    for (int j = 0; j < 8; ++j) r[j] += a[i + j];
  double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
  for (; i < n; ++i) res += a[i];
  return res;
}

BSGP_HD double np_pairwise_sum(const double* a, int n) {
  int off[40], len[40], stage[40];
  double left[40];
  int sp = 0;
  off[0] = 0;
  len[0] = n;
  stage[0] = 0;
  double ret = 0.0;
  for (;;) {
    if (len[sp] > 128 && stage[sp] == 0) {  // descend into the left half
      int n2 = len[sp] / 2;
      n2 -= n2 % 8;
      stage[sp] = 1;
      off[sp + 1] = off[sp];
      len[sp + 1] = n2;
      stage[sp + 1] = 0;
      ++sp;
      continue;
    }
    ret = np_pairwise_block(a + off[sp], len[sp]);
    for (;;) {  // hand `ret` up the stack
      if (sp == 0) return ret;
      --sp;
      if (stage[sp] == 1) {  // left half done: evaluate the right half
        left[sp] = ret;
        stage[sp] = 2;
        int n2 = len[sp] / 2;
        n2 -= n2 % 8;
        off[sp + 1] = off[sp] + n2;
        len[sp + 1] = len[sp] - n2;
        stage[sp + 1] = 0;
        ++sp;
        break;
      }
      ret = left[sp] + ret;
    }
  }
}

#if defined(__HIPCC__)

__device__ __forceinline__ double dev_nan() { return __longlong_as_double(0x7ff8000000000000LL); }
__device__ __forceinline__ double dev_inf() { return __longlong_as_double(0x7ff0000000000000LL); }

// ---- lock-free union-find over an int array of parents (root = smallest
// index).  SCOPE is the __HIP_MEMORY_SCOPE_* of the relaxed atomic loads: the
// scope of the integer atomics that write the array (agent in global memory,
// workgroup in LDS).
template <int SCOPE>
__device__ __forceinline__ int uf_load(const int* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, SCOPE);
}

// root of a: parents never increase along a path, so the walk ends.  On the
// way every visited pixel is moved to its grandparent (path halving; an
// atomicMin, since a concurrent link may already have moved it further up).
template <int SCOPE>
__device__ __forceinline__ int uf_find(int* L, int a) {
  int p = uf_load<SCOPE>(L + a);
  while (p != a) {
    const int g = uf_load<SCOPE>(L + p);
    if (g != p) atomicMin(L + a, g);
    a = p;
    p = g;
  }
  return a;
}

// unite the components of a and b: link the larger root to the smaller.  If
// another thread linked that root first (old != a), its link target and b are
// united instead, so no union is lost; both roots only ever decrease.
template <int SCOPE>
__device__ __forceinline__ void uf_unite(int* L, int a, int b) {
  for (;;) {
    a = uf_find<SCOPE>(L, a);
    b = uf_find<SCOPE>(L, b);
    if (a == b) return;
    if (a < b) {
      const int t = a;
      a = b;
      b = t;
    }
    const int old = atomicMin(L + a, b);
    if (old == a) return;
    a = old;
  }
}

// min / max of one int per lane over the wave, in every lane
__device__ __forceinline__ int wave_min(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int u = __shfl_xor(v, o, 64);
    v = u < v ? u : v;
  }
  return v;
}
__device__ __forceinline__ int wave_max(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int u = __shfl_xor(v, o, 64);
    v = u > v ? u : v;
  }
  return v;
}

// exclusive prefix of one count per thread over the 256-thread workgroup, in
// thread order; *total is the workgroup's sum (in every thread).  wsum: 4 ints
// of LDS; both barriers are inside, so rounds may follow one another.
__device__ __forceinline__ int block_scan(int c, int* wsum, int* total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int inc = c;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int u = __shfl_up(inc, o, 64);
    if (lane >= o) inc += u;
  }
  if (lane == 63) wsum[w] = inc;
  __syncthreads();
  int base = 0, tot = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int u = wsum[k];
    if (k < w) base += u;
    tot += u;
  }
  __syncthreads();
  *total = tot;
  return base + inc - c;
}

#endif  // __HIPCC__

}  // namespace bsgp
