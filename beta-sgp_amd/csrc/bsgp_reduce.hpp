// bsgp_reduce.hpp — the workgroup's size and the fixed-order wave and workgroup
// reductions (sum, max, min of doubles) that the solver (bsgp_device.hpp) and
// the application kernels share.  Nothing of the FFT core or the plan geometry.
//
// A unit that defines BSGP_BLOCK (and renames the namespace) before its
// includes gets the reductions of that workgroup size (bsgp_solver_c512.hip).
#pragma once

#include <hip/hip_runtime.h>

namespace bsgp {

#ifndef BSGP_BLOCK
#define BSGP_BLOCK 256
#endif
constexpr int kBlock = BSGP_BLOCK;  // threads per workgroup (one image per workgroup)
constexpr int kWaves = kBlock / 64;
constexpr int kMaxRed = 24;  // doubles reduced at once

// --------------------------------------------------------------- syncs
// LDS hand-off between lanes of ONE wavefront: wait for this wave's LDS ops
// and keep the compiler from moving LDS accesses across the point.
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0)
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

struct WaveSync {
  __device__ __forceinline__ void operator()() const { wave_sync(); }
};

// --------------------------------------------------------------- reductions
// v of lane (lane ^ O), every lane of the wave active: xor 1 and 2 by DPP
// quad permutes (VALU, no LDS pipe), xor 4 / 8 / 16 by ds_swizzle's bit mode
// (no address VGPR), xor 32 by ds_bpermute (__shfl_xor).  The same pairing as
// __shfl_xor for every O, so the reduction trees below keep their bits.
template <int O>
__device__ __forceinline__ double xor_lanes(double v) {
  if constexpr (O == 1 || O == 2) {
    constexpr int ctrl = O == 1 ? 0xB1 : 0x4E;  // quad_perm [1,0,3,2] / [2,3,0,1]
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), ctrl, 0xF, 0xF, false);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), ctrl, 0xF, 0xF, false);
    return __hiloint2double(hi, lo);
  } else if constexpr (O < 32) {
    constexpr int pat = (O << 10) | 0x1F;  // bit mode: and 0x1F, or 0, xor O
    const int lo = __builtin_amdgcn_ds_swizzle(__double2loint(v), pat);
    const int hi = __builtin_amdgcn_ds_swizzle(__double2hiint(v), pat);
    return __hiloint2double(hi, lo);
  } else {
    return __shfl_xor(v, O, 64);
  }
}
__device__ __forceinline__ double wave_sum(double v) {
  v += xor_lanes<32>(v);
  v += xor_lanes<16>(v);
  v += xor_lanes<8>(v);
  v += xor_lanes<4>(v);
  v += xor_lanes<2>(v);
  v += xor_lanes<1>(v);
  return v;
}
template <bool MAX>
__device__ __forceinline__ double wave_ext_step(double v, double u) {
  // NaN propagates like np.max / np.min
  return MAX ? ((u > v || u != u) ? u : v) : ((u < v || u != u) ? u : v);
}
template <bool MAX>
__device__ __forceinline__ double wave_ext(double v) {
  v = wave_ext_step<MAX>(v, xor_lanes<32>(v));
  v = wave_ext_step<MAX>(v, xor_lanes<16>(v));
  v = wave_ext_step<MAX>(v, xor_lanes<8>(v));
  v = wave_ext_step<MAX>(v, xor_lanes<4>(v));
  v = wave_ext_step<MAX>(v, xor_lanes<2>(v));
  v = wave_ext_step<MAX>(v, xor_lanes<1>(v));
  return v;
}
__device__ __forceinline__ double wave_max(double v) { return wave_ext<true>(v); }
__device__ __forceinline__ double wave_min(double v) { return wave_ext<false>(v); }

// Sum NV per-thread values over the workgroup; every thread gets the totals.
// Wave partials go to LDS, thread i < NV adds the kWaves partials of value i
// in a fixed order, and every thread reads the NV totals: deterministic and
// identical in every thread, with only NV LDS reads per thread.
template <int NV>
__device__ __forceinline__ void block_sum(double (&v)[NV], double* red) {
  static_assert(NV <= kMaxRed, "too many values");
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    double s = wave_sum(v[i]);
    if (lane == 0) red[w * kMaxRed + i] = s;
  }
  __syncthreads();
  if (threadIdx.x < NV) {
    const int i = threadIdx.x;
    double s = red[i];
#pragma unroll
    for (int k = 1; k < kWaves; ++k) s += red[k * kMaxRed + i];
    red[kWaves * kMaxRed + i] = s;
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < NV; ++i) v[i] = red[kWaves * kMaxRed + i];
  __syncthreads();
}

__device__ __forceinline__ double block_max(double v, double* red) {
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  v = wave_max(v);
  if (lane == 0) red[w * kMaxRed] = v;
  __syncthreads();
  double s = red[0];
  for (int k = 1; k < kWaves; ++k) {
    double u = red[k * kMaxRed];
    s = (u > s || u != u) ? u : s;
  }
  __syncthreads();
  return s;
}

__device__ __forceinline__ double block_min(double v, double* red) {
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  v = wave_min(v);
  if (lane == 0) red[w * kMaxRed] = v;
  __syncthreads();
  double s = red[0];
  for (int k = 1; k < kWaves; ++k) {
    double u = red[k * kMaxRed];
    s = (u < s || u != u) ? u : s;
  }
  __syncthreads();
  return s;
}

}  // namespace bsgp
