// bsgp_segment.hip — source detection and per-segment measurement on the
// device: what restoration/utils.py:240-247 does with photutils
// (convolve, detect_sources, SourceCatalog) before deblending, restated from
// its parts:
//
//  k_seg_convolve  one thread per pixel: the zero-filled direct convolution of
//                  astropy.convolution.convolve (products rounded one by one,
//                  rows outer, columns inner, one division by the kernel's sum).
//  k_seg_init      detection mask (data > threshold, finite, not masked): a
//                  detected pixel starts as its own root (its linear index).
//  k_seg_union     every detected pixel unites with its detected neighbours to
//                  the west and in the row above (N, and NW / NE at
//                  connectivity 8, as few of them as close the component) in
//                  a union-find in global memory: the larger
//                  root is linked to the smaller with an integer atomicMin, so a
//                  component's root is its first pixel in raster order whatever
//                  order the unions ran in.  No thread waits for another: every
//                  walk follows strictly decreasing parents.
//  k_seg_flatten   every pixel moves to its root and counts into its area.
//  k_seg_count / k_seg_scan / k_seg_assign / k_seg_relabel
//                  roots with area >= npixels are numbered 1..n in raster order
//                  (per-chunk counts, one scan of the counts per image, ranks
//                  inside a chunk) and the int32 label image is written.
//  k_cat_init / k_cat_bbox / k_cat_measure
//                  area and inclusive bounding box per label (integer atomics),
//                  then one wave per segment scans its box in raster order:
//                  lane partials in a fixed order, a fixed-order wave reduction.
//
// No floating-point atomics; integer atomics only where their order does not
// matter (min, max, count): a batch gives each image the bits it gets alone.
#include <hip/hip_runtime.h>

#include "bsgp_apps.hpp"
#include "bsgp_prims.hpp"
#include "bsgp_reduce.hpp"

namespace bsgp {

namespace {
constexpr int kAgent = __HIP_MEMORY_SCOPE_AGENT;  // the union-find lives in global memory
}  // namespace

// -------------------------------------------------------------- convolution
template <typename T>
__global__ void __launch_bounds__(256) k_seg_convolve(SegConvArgs a) {
  __shared__ double K[kSegMaxKernel * kSegMaxKernel + 1];
  const int nk = a.kh * a.kw;
  if ((int)threadIdx.x < nk) K[threadIdx.x] = a.kernel[threadIdx.x];
  __syncthreads();
  if (threadIdx.x == 0) K[nk] = np_pairwise_block(K, nk);
  __syncthreads();
  const double ksum = K[nk];
  const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y, b = blockIdx.z;
  if (x >= a.W) return;
  const T* img = static_cast<const T*>(a.data) + (size_t)b * a.H * a.W;
  const int py = a.kh / 2, px = a.kw / 2;
  double acc = 0.0;
  for (int i = 0; i < a.kh; ++i) {
    const int yy = y + i - py;
    if (yy < 0 || yy >= a.H) continue;  // the zero fill adds exact zeros
    const T* row = img + (size_t)yy * a.W;
    for (int j = 0; j < a.kw; ++j) {
      const int xx = x + j - px;
      if (xx < 0 || xx >= a.W) continue;
      acc = __dadd_rn(acc, __dmul_rn((double)row[xx], K[nk - 1 - (i * a.kw + j)]));
    }
  }
  a.out[((size_t)b * a.H + y) * a.W + x] = acc / ksum;
}

hipError_t launch_seg_convolve(const SegConvArgs& a, int f32, hipStream_t s) {
  const dim3 grid((a.W + 255) / 256, a.H, a.B), block(256);
  if (f32)
    hipLaunchKernelGGL(k_seg_convolve<float>, grid, block, 0, s, a);
  else
    hipLaunchKernelGGL(k_seg_convolve<double>, grid, block, 0, s, a);
  return hipGetLastError();
}

// ---------------------------------------------------------------- labelling
template <typename T>
__global__ void __launch_bounds__(256) k_seg_init(SegArgs a) {
  const int hw = a.H * a.W;
  const unsigned pu = blockIdx.x * 256u + threadIdx.x;
  if (pu >= (unsigned)hw) return;
  const int p = (int)pu, b = blockIdx.y;
  const size_t o = (size_t)b * hw + p;
  const double v = (double)static_cast<const T*>(a.data)[o];
  const double t = a.thr_map ? a.thr_map[o] : a.thr;
  const bool det = v > t && __builtin_isfinite(v) && __builtin_isfinite(t) && !(a.mask && a.mask[o]);
  a.lab[o] = det ? p : -1;
  a.area[o] = 0;
}

__global__ void __launch_bounds__(256) k_seg_union(SegArgs a) {
  const int hw = a.H * a.W;
  const unsigned pu = blockIdx.x * 256u + threadIdx.x;
  if (pu >= (unsigned)hw) return;
  const int p = (int)pu, b = blockIdx.y;
  int* L = a.lab + (size_t)b * hw;
  if (uf_load<kAgent>(L + p) < 0) return;
  const int y = p / a.W, x = p - y * a.W;
  const bool w = x > 0 && uf_load<kAgent>(L + p - 1) >= 0;
  const int q = p - a.W;  // the pixel above
  const bool n = y > 0 && uf_load<kAgent>(L + q) >= 0;
  if (a.conn == 4) {
    if (w) uf_unite<kAgent>(L, p, p - 1);
    if (n) uf_unite<kAgent>(L, p, q);
    return;
  }
  // connectivity 8: W, NW and NE all touch N, and those contacts are united
  // by N's, NE's and W's own threads, so with N one union is enough; without
  // N, NE still has to be joined with NW or W (Wu, Otoo and Suzuki's tree)
  if (n) {
    uf_unite<kAgent>(L, p, q);
    return;
  }
  const bool nw = y > 0 && x > 0 && uf_load<kAgent>(L + q - 1) >= 0;
  const bool ne = y > 0 && x < a.W - 1 && uf_load<kAgent>(L + q + 1) >= 0;
  if (ne) uf_unite<kAgent>(L, p, q + 1);
  if (nw) uf_unite<kAgent>(L, p, q - 1);
  else if (w) uf_unite<kAgent>(L, p, p - 1);
}

__global__ void __launch_bounds__(256) k_seg_flatten(SegArgs a) {
  const int hw = a.H * a.W, b = blockIdx.y;
  const unsigned pu = blockIdx.x * 256u + threadIdx.x;
  int* L = a.lab + (size_t)b * hw;
  const int p = (int)pu;
  const bool det = pu < (unsigned)hw && uf_load<kAgent>(L + p) >= 0;
  int r = -1;
  if (det) {
    r = uf_find<kAgent>(L, p);
    // a root keeps its own index; any other pixel's parent only moves up its path
    if (r != p) __hip_atomic_store(L + p, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  // area: one atomic per wave where its detected lanes share one root (the
  // inside of a large segment), one per lane otherwise
  const unsigned long long m = __ballot(det);
  if (m == 0) return;
  const int first = __ffsll((long long)m) - 1;
  const int r0 = __shfl(r, first, 64);
  int* area = a.area + (size_t)b * hw;
  if (__ballot(det && r != r0) == 0) {
    if ((int)(threadIdx.x & 63) == first) atomicAdd(area + r0, __popcll(m));
  } else if (det) {
    atomicAdd(area + r, 1);
  }
}

// ---------------------------------------------------------------- compaction
// a workgroup covers kSegChunk = 2048 consecutive pixels, 8 per thread
__device__ __forceinline__ int seg_flags(const SegArgs& a, int b, unsigned p0, unsigned* bits) {
  const int hw = a.H * a.W;
  const int* L = a.lab + (size_t)b * hw;
  const int* A = a.area + (size_t)b * hw;
  int c = 0;
  unsigned m = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const unsigned p = p0 + k;
    if (p < (unsigned)hw && L[p] == (int)p && A[p] >= a.npixels) {
      m |= 1u << k;
      ++c;
    }
  }
  *bits = m;
  return c;
}

__global__ void __launch_bounds__(256) k_seg_count(SegArgs a) {
  __shared__ int wsum[4];
  const int b = blockIdx.y;
  unsigned bits;
  const int c = seg_flags(a, b, blockIdx.x * (unsigned)kSegChunk + threadIdx.x * 8u, &bits);
  int total;
  (void)block_scan(c, wsum, &total);
  if (threadIdx.x == 0) a.blk[(size_t)b * a.nblk + blockIdx.x] = total;
}

// one workgroup per image: exclusive scan of its chunk counts, in place
__global__ void __launch_bounds__(256) k_seg_scan(SegArgs a) {
  __shared__ int wsum[4];
  const int b = blockIdx.x;
  int* blk = a.blk + (size_t)b * a.nblk;
  int carry = 0;
  for (int base = 0; base < a.nblk; base += 256) {
    const int i = base + threadIdx.x;
    const int c = i < a.nblk ? blk[i] : 0;
    int total;
    const int ex = block_scan(c, wsum, &total);
    if (i < a.nblk) blk[i] = carry + ex;
    carry += total;
  }
  if (threadIdx.x == 0) a.nlabels_out[b] = carry;
}

// a kept root's area becomes its final label, any other root's 0
__global__ void __launch_bounds__(256) k_seg_assign(SegArgs a) {
  __shared__ int wsum[4];
  const int hw = a.H * a.W, b = blockIdx.y;
  const unsigned p0 = blockIdx.x * (unsigned)kSegChunk + threadIdx.x * 8u;
  unsigned bits;
  const int c = seg_flags(a, b, p0, &bits);
  int total;
  int rank = a.blk[(size_t)b * a.nblk + blockIdx.x] + block_scan(c, wsum, &total);
  const int* L = a.lab + (size_t)b * hw;
  int* A = a.area + (size_t)b * hw;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const unsigned p = p0 + k;
    if (p < (unsigned)hw && L[p] == (int)p) A[p] = (bits >> k & 1u) ? ++rank : 0;
  }
}

__global__ void __launch_bounds__(256) k_seg_relabel(SegArgs a) {
  const int hw = a.H * a.W;
  const unsigned pu = blockIdx.x * 256u + threadIdx.x;
  if (pu >= (unsigned)hw) return;
  const int p = (int)pu, b = blockIdx.y;
  const size_t o = (size_t)b * hw;
  const int r = a.lab[o + p];
  a.labels_out[o + p] = r >= 0 ? a.area[o + r] : 0;
}

hipError_t launch_seg_detect(const SegArgs& a, int f32, hipStream_t s) {
  const int hw = a.H * a.W;
  const dim3 px((unsigned)(((size_t)hw + 255) / 256), a.B), ch(a.nblk, a.B), block(256);
  if (f32)
    hipLaunchKernelGGL(k_seg_init<float>, px, block, 0, s, a);
  else
    hipLaunchKernelGGL(k_seg_init<double>, px, block, 0, s, a);
  hipLaunchKernelGGL(k_seg_union, px, block, 0, s, a);
  hipLaunchKernelGGL(k_seg_flatten, px, block, 0, s, a);
  hipLaunchKernelGGL(k_seg_count, ch, block, 0, s, a);
  hipLaunchKernelGGL(k_seg_scan, dim3(a.B), block, 0, s, a);
  hipLaunchKernelGGL(k_seg_assign, ch, block, 0, s, a);
  hipLaunchKernelGGL(k_seg_relabel, px, block, 0, s, a);
  return hipGetLastError();
}

// ----------------------------------------------------------------- catalogue
// rows of image b that are measured: labels 1..rows
__device__ __forceinline__ int cat_rows(const SegCatArgs& a, int b) {
  int n = a.cap;
  if (a.nlabels) {
    const int m = a.nlabels[b];
    n = m < n ? (m < 0 ? 0 : m) : n;
  }
  return n;
}

__global__ void __launch_bounds__(256) k_cat_init(SegCatArgs a) {
  const int i = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  if (i == 0) a.status[b] = (a.nlabels && a.nlabels[b] > a.cap) ? 1 : 0;
  if (i >= a.cap) return;
  int* ic = a.icols + ((size_t)b * a.cap + i) * 5;
  ic[0] = 0;
  ic[1] = 0x7fffffff;
  ic[2] = -1;
  ic[3] = 0x7fffffff;
  ic[4] = -1;
  double* fc = a.fcols + ((size_t)b * a.cap + i) * 8;
#pragma unroll
  for (int k = 0; k < 8; ++k) fc[k] = 0.0;
}

__global__ void __launch_bounds__(256) k_cat_bbox(SegCatArgs a) {
  const int hw = a.H * a.W, b = blockIdx.y;
  const unsigned pu = blockIdx.x * 256u + threadIdx.x;
  const int p = (int)pu;
  int l = pu < (unsigned)hw ? a.labels[(size_t)b * hw + p] : 0;
  if (l != 0 && (l < 0 || l > cat_rows(a, b))) {  // a label without a row: reported, never written
    atomicOr(a.status + b, 2);
    l = 0;
  }
  const bool valid = l != 0;
  const unsigned long long m = __ballot(valid);
  if (m == 0) return;
  const int y = p / a.W, x = p - y * a.W;
  // one set of atomics per wave where its labelled lanes share one label
  const int first = __ffsll((long long)m) - 1;
  const int l0 = __shfl(l, first, 64);
  const bool same = __ballot(valid && l != l0) == 0;
  const int xmn = wave_min(valid ? x : 0x7fffffff), xmx = wave_max(valid ? x : -1);
  const int ymn = wave_min(valid ? y : 0x7fffffff), ymx = wave_max(valid ? y : -1);
  if (same) {
    if ((int)(threadIdx.x & 63) == first) {
      int* ic = a.icols + ((size_t)b * a.cap + (l0 - 1)) * 5;
      atomicAdd(ic, __popcll(m));
      atomicMin(ic + 1, xmn);
      atomicMax(ic + 2, xmx);
      atomicMin(ic + 3, ymn);
      atomicMax(ic + 4, ymx);
    }
  } else if (valid) {
    int* ic = a.icols + ((size_t)b * a.cap + (l - 1)) * 5;
    atomicAdd(ic, 1);
    atomicMin(ic + 1, x);
    atomicMax(ic + 2, x);
    atomicMin(ic + 3, y);
    atomicMax(ic + 4, y);
  }
}

// one wave per segment
__global__ void __launch_bounds__(256) k_cat_measure(SegCatArgs a) {
  const int lane = threadIdx.x & 63;
  const int sgm = blockIdx.x * 4 + (threadIdx.x >> 6), b = blockIdx.y;
  if (sgm >= cat_rows(a, b)) return;
  const int* ic = a.icols + ((size_t)b * a.cap + sgm) * 5;
  double* fc = a.fcols + ((size_t)b * a.cap + sgm) * 8;
  if (ic[0] == 0) return;  // a label the image does not hold: zeros
  const int x0 = ic[1], y0 = ic[3], bw = ic[2] - x0 + 1, n = bw * (ic[4] - y0 + 1);
  const size_t o = (size_t)b * a.H * a.W;
  const int* lab = a.labels + o;
  const double* dat = a.data + o;
  const double* cnv = (a.conv ? a.conv : a.data) + o;
  const int want = sgm + 1;

  double flux = 0.0, mn = dev_inf(), mx = -dev_inf(), sc = 0.0, sx = 0.0, sy = 0.0;
  for (int k = lane; k < n; k += 64) {
    const int r = k / bw, c = k - r * bw;
    const size_t q = (size_t)(y0 + r) * a.W + (x0 + c);
    if (lab[q] != want) continue;
    const double v = dat[q], w = cnv[q];
    flux += v;
    mn = v < mn ? v : mn;
    mx = v > mx ? v : mx;
    sc += w;
    sx += w * (double)c;
    sy += w * (double)r;
  }
  flux = wave_sum(flux);
  sc = wave_sum(sc);
  sx = wave_sum(sx);
  sy = wave_sum(sy);
  mn = wave_min(mn);
  mx = wave_max(mx);
  const double xc = sx / sc, yc = sy / sc;  // relative to the box's corner

  double mxx = 0.0, mxy = 0.0, myy = 0.0;
  for (int k = lane; k < n; k += 64) {
    const int r = k / bw, c = k - r * bw;
    const size_t q = (size_t)(y0 + r) * a.W + (x0 + c);
    if (lab[q] != want) continue;
    const double w = cnv[q], dx = (double)c - xc, dy = (double)r - yc;
    mxx += w * dx * dx;
    mxy += w * dx * dy;
    myy += w * dy * dy;
  }
  mxx = wave_sum(mxx);
  mxy = wave_sum(mxy);
  myy = wave_sum(myy);
  if (lane == 0) {
    fc[0] = flux;
    fc[1] = mn;
    fc[2] = mx;
    fc[3] = (double)x0 + xc;
    fc[4] = (double)y0 + yc;
    fc[5] = mxx / sc;
    fc[6] = mxy / sc;
    fc[7] = myy / sc;
  }
}

hipError_t launch_seg_catalog(const SegCatArgs& a, hipStream_t s) {
  const int hw = a.H * a.W;
  const dim3 block(256);
  hipLaunchKernelGGL(k_cat_init, dim3((a.cap + 255) / 256, a.B), block, 0, s, a);
  hipLaunchKernelGGL(k_cat_bbox, dim3((unsigned)(((size_t)hw + 255) / 256), a.B), block, 0, s, a);
  hipLaunchKernelGGL(k_cat_measure, dim3((a.cap + 3) / 4, a.B), block, 0, s, a);
  return hipGetLastError();
}

}  // namespace bsgp
