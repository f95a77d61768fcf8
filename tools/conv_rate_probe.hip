// conv_rate_probe.hip — the yardstick of tools/conv_timing.py: a register-only
// loop of separately rounded float64 multiplies and adds, eight independent
// chains per thread (what bsgp_convolve.hip's inner loop issues, without its
// LDS reads and kernel loads).  Built by the tool into tools/_conv_rate_probe.so.
#include <hip/hip_runtime.h>

__global__ void __launch_bounds__(256) k_rate(double* out, const double* kin, int iters) {
  double k[8], acc[8];
#pragma unroll
  for (int r = 0; r < 8; ++r) k[r] = kin[r], acc[r] = 1.0 + 1e-3 * (double)(threadIdx.x + r);
  for (int i = 0; i < iters; ++i) {
    double prev[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) prev[r] = acc[r];
#pragma unroll
    for (int r = 0; r < 8; ++r) acc[r] = __dadd_rn(prev[r], __dmul_rn(prev[(r + 1) & 7], k[r]));
  }
  double s = 0.0;
#pragma unroll
  for (int r = 0; r < 8; ++r) s += acc[r];
  out[(size_t)blockIdx.x * 256 + threadIdx.x] = s;
}

// 16 separately rounded operations per thread and iteration
extern "C" int conv_rate_probe(double* out, const double* kin, int blocks, int iters, void* stream) {
  hipLaunchKernelGGL(k_rate, dim3(blocks), dim3(256), 0, (hipStream_t)stream, out, kin, iters);
  return (int)hipGetLastError();
}
