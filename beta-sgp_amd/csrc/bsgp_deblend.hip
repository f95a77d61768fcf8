// bsgp_deblend.hip — deblending of detected sources on the device: what
// SourceFinder(deblend=True) adds to detect_sources in restoration/utils.py:235,
// modelled on photutils' deblend_sources (multi-threshold tree + watershed) and
// restated from its parts:
//
//  k_deblend_parent  one workgroup per parent segment.  The parent's box of
//                    data and its mask are staged in LDS; D1 statistics by one
//                    wave in a fixed lane order; per level (D3) a union-find
//                    over the box in LDS with k_seg_union's neighbour tree
//                    (root = smallest index, integer atomicMin only, areas by
//                    integer atomicAdd); the marker tree (D4) by counting the
//                    level's kept roots per current region (integer atomicAdd);
//                    the flood (D5) on one lane with a binary heap in LDS keyed
//                    by (-v, index); the contrast loop (D6) with one wave per
//                    child summing in a fixed order.  Writes the parent's child
//                    count and, for a split parent, every pixel's child rank
//                    into labels_out.
//  k_deblend_large   the same for a parent whose box is over the LDS cap
//                    (bsgp_deblend_sources_large): one workgroup per parent,
//                    the working set in global memory keyed by image pixel,
//                    the heap's first levels in LDS with the key in the entry,
//                    the frontier collected and heapified by all threads, the
//                    flood itself on one lane.  Same identities, orders and
//                    sums: a parent gets the same labels from either kernel.
//  k_deblend_number  one workgroup per image: D7's numbering from the child
//                    counts (two scans in label order).
//  k_deblend_relabel one thread per pixel: the final int32 label image.
//
// No floating-point atomics, no kernel waits for another workgroup; a parent's
// result depends only on its own pixels and box.
#include <hip/hip_runtime.h>

#include "bsgp_apps.hpp"
#include "bsgp_prims.hpp"
#include "bsgp_reduce.hpp"

namespace bsgp {

namespace {

constexpr int kBox = kDeblendMaxBox;
constexpr int kOutside = -1;  // not a pixel of the parent
constexpr int kFree = -2;     // a pixel of the parent in no region / not yet flooded

// scope of the union-find's loads: k_deblend_parent's array is in LDS,
// k_deblend_large's in global memory
constexpr int kLds = __HIP_MEMORY_SCOPE_WORKGROUP, kAgent = __HIP_MEMORY_SCOPE_AGENT;

// a table of kBox 16-bit counters, two per int (a count is at most kBox)
__device__ __forceinline__ void t16_add(int* t, int i) { atomicAdd(t + (i >> 1), 1 << ((i & 1) << 4)); }
__device__ __forceinline__ int t16_get(const int* t, int i) {
  return (t[i >> 1] >> ((i & 1) << 4)) & 0xffff;
}

// neighbour k = 0..7 of box pixel p (row-major, NW first), or -1
__device__ __forceinline__ int db_nbr(int p, int x, int y, int k, int bw, int bh, int conn) {
  const int kk = k < 4 ? k : k + 1;
  const int dy = kk / 3 - 1, dx = kk - (kk / 3) * 3 - 1;
  if (conn == 4 && dx != 0 && dy != 0) return -1;
  const int xx = x + dx, yy = y + dy;
  if (xx < 0 || xx >= bw || yy < 0 || yy >= bh) return -1;
  return p + dy * bw + dx;
}

// heap order: the larger value first (the smaller key -v), then the smaller index
__device__ __forceinline__ bool db_before(const double* v, int a, int b) {
  const double x = v[a], y = v[b];
  return x > y || (x == y && a < b);
}

__device__ __forceinline__ void db_push(short* h, int& n, const double* v, int p) {
  int i = n++;
  while (i > 0) {
    const int up = (i - 1) >> 1, q = h[up];
    if (!db_before(v, p, q)) break;
    h[i] = (short)q;
    i = up;
  }
  h[i] = (short)p;
}

__device__ __forceinline__ int db_pop(short* h, int& n, const double* v) {
  const int top = h[0], last = h[--n];
  int i = 0;
  for (;;) {
    int c = 2 * i + 1;
    if (c >= n) break;
    int q = h[c];
    if (c + 1 < n) {
      const int q2 = h[c + 1];
      if (db_before(v, q2, q)) {
        ++c;
        q = q2;
      }
    }
    if (!db_before(v, q, last)) break;
    h[i] = (short)q;
    i = c;
  }
  h[i] = (short)last;
  return top;
}

// D5 on the calling lane: lab holds a marker identity (>= 0), kFree or
// kOutside per box pixel.  A labelled pixel without a free neighbour can give
// its label to nobody, now or later, so it is not entered; every pixel enters
// the heap at most once, so the heap holds at most the box.
__device__ __forceinline__ void db_flood(const double* v, int* lab, short* heap, int bw, int bh,
                                         int conn) {
  int hn = 0;
  for (int y = 0, p = 0; y < bh; ++y) {
    for (int x = 0; x < bw; ++x, ++p) {
      if (lab[p] < 0) continue;
      bool open = false;
      for (int k = 0; k < 8; ++k) {
        const int q = db_nbr(p, x, y, k, bw, bh, conn);
        if (q >= 0 && lab[q] == kFree) open = true;
      }
      if (open) db_push(heap, hn, v, p);
    }
  }
  while (hn > 0) {
    const int p = db_pop(heap, hn, v);
    const int y = p / bw, x = p - y * bw, l = lab[p];
    for (int k = 0; k < 8; ++k) {
      const int q = db_nbr(p, x, y, k, bw, bh, conn);
      if (q >= 0 && lab[q] == kFree) {
        lab[q] = l;
        db_push(heap, hn, v, q);
      }
    }
  }
}

// sum of v over the box pixels with lab == want by the calling wave: lane
// partials in raster order, one fixed-order wave reduction
__device__ __forceinline__ double db_wave_sum_of(const double* v, const int* lab, int want, int n) {
  const int lane = threadIdx.x & 63;
  double s = 0.0;
  for (int k = lane; k < n; k += 64)
    if (lab[k] == want) s += v[k];
  return wave_sum(s);
}

__device__ __forceinline__ int db_rows(const DeblendArgs& a, int b) {
  const int m = a.nlabels[b];
  return m < a.cap ? (m < 0 ? 0 : m) : a.cap;
}

}  // namespace

__global__ void __launch_bounds__(256) k_deblend_parent(DeblendArgs a) {
  __shared__ double v[kBox];
  __shared__ int lev[kBox];    // D3: union-find parents of the level; D5: flood labels
  __shared__ short reg[kBox];  // the region (its root) a pixel is in, kFree or kOutside
  __shared__ int bufA[kBox / 2];  // D3: areas (16-bit); then the marker list (shorts)
  __shared__ int bufB[kBox / 2];  // D4: kept roots per region (16-bit); the heap; the ranks
  __shared__ double thr[256];  // D2: thresholds of 256 levels
  __shared__ double sred[8];
  __shared__ int sint[8];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i = blockIdx.x, b = blockIdx.y;
  if (i >= db_rows(a, b)) return;
  const size_t row = (size_t)b * a.cap + i;
  const int* ic = a.icols + row * 5;
  const int area = ic[0];
  if (area <= 0 || area < 2 * (long long)a.npixels || (a.sel && !a.sel[row])) return;
  const int x0 = ic[1], y0 = ic[3], bw = ic[2] - x0 + 1, bh = ic[4] - y0 + 1;
  if (x0 < 0 || y0 < 0 || bw < 1 || bh < 1 || ic[2] >= a.W || ic[4] >= a.H) return;
  if ((long long)bw * bh > a.lds_max_box) {  // at most kBox; k_deblend_large's when there is one
    if (!a.large && tid == 0) atomicOr(a.status + b, BSGP_DEBLEND_OVER_CAP);
    return;
  }
  const int n = bw * bh, want = i + 1;
  const size_t o = (size_t)b * a.H * a.W;

  // staging
  if (tid == 0) sint[0] = n, sint[1] = 0, sint[5] = 0;
  __syncthreads();
  for (int k = tid; k < n; k += 256) {
    const int r = k / bw, c = k - r * bw;
    const size_t q = o + (size_t)(y0 + r) * a.W + (x0 + c);
    const bool in = a.labels[q] == want;
    v[k] = a.data[q];
    reg[k] = in ? 0 : kOutside;
    if (in) atomicMin(&sint[0], k);
  }
  __syncthreads();
  const int root0 = sint[0];
  if (root0 >= n) return;
  for (int k = tid; k < n; k += 256)
    if (reg[k] != kOutside) reg[k] = (short)root0;
  __syncthreads();

  // D1
  if (wave == 0) {
    double s = 0.0, mn = dev_inf(), mx = -dev_inf();
    for (int k = lane; k < n; k += 64) {
      if (reg[k] == kOutside) continue;
      const double x = v[k];
      s += x;
      mn = x < mn ? x : mn;
      mx = x > mx ? x : mx;
    }
    s = wave_sum(s);
    mn = wave_min(mn);
    mx = wave_max(mx);
    if (lane == 0) sred[0] = mn, sred[1] = mx, sred[2] = s;
  }
  __syncthreads();
  const double smin = sred[0], smax = sred[1], ssum = sred[2];
  if (!(smin < smax)) return;

  // D2 to D4
  const bool linear = a.mode == BSGP_DEBLEND_LINEAR || smin < 0.0;
  const double m = smin != 0.0 ? smin : 0.01 * smax;
  const double den = (double)(a.nlevels + 1);
  const int half = (n + 1) >> 1;
  for (int lv = 1; lv <= a.nlevels; ++lv) {
    // the next 256 thresholds, one per thread (a pow per level and wave would
    // cost as much as the level's labelling); the last level ended at a barrier
    if (((lv - 1) & 255) == 0) {
      const double k = (double)(lv + tid);
      thr[tid] = linear ? smin + (smax - smin) / den * k : m * pow(smax / m, k / den);
      __syncthreads();
    }
    const double t = thr[(lv - 1) & 255];
    int above = 0;
    for (int p = tid; p < n; p += 256) {
      const bool on = reg[p] != kOutside && v[p] > t;
      lev[p] = on ? p : -1;
      above += on;
    }
    if (above) atomicAdd(&sint[5], above);
    for (int j = tid; j < half; j += 256) bufA[j] = 0, bufB[j] = 0;
    __syncthreads();
    // two components of npixels pixels need 2 * npixels pixels above the
    // level, and the levels rise: nothing can split from here on
    if (sint[5] < 2 * (long long)a.npixels) break;
    for (int p = tid; p < n; p += 256) {
      if (uf_load<kLds>(lev + p) < 0) continue;
      const int y = p / bw, x = p - y * bw, q = p - bw;
      const bool w = x > 0 && uf_load<kLds>(lev + p - 1) >= 0;
      const bool nn = y > 0 && uf_load<kLds>(lev + q) >= 0;
      if (a.conn == 4) {
        if (w) uf_unite<kLds>(lev, p, p - 1);
        if (nn) uf_unite<kLds>(lev, p, q);
        continue;
      }
      if (nn) {
        uf_unite<kLds>(lev, p, q);
        continue;
      }
      const bool nw = y > 0 && x > 0 && uf_load<kLds>(lev + q - 1) >= 0;
      const bool ne = y > 0 && x < bw - 1 && uf_load<kLds>(lev + q + 1) >= 0;
      if (ne) uf_unite<kLds>(lev, p, q + 1);
      if (nw) uf_unite<kLds>(lev, p, q - 1);
      else if (w) uf_unite<kLds>(lev, p, p - 1);
    }
    __syncthreads();
    for (int p = tid; p < n; p += 256) {
      if (uf_load<kLds>(lev + p) < 0) continue;
      const int r = uf_find<kLds>(lev, p);
      if (r != p) __hip_atomic_store(lev + p, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      t16_add(bufA, r);
    }
    if (tid == 0) sint[5] = 0;  // every thread read it before the barrier above
    __syncthreads();
    // a kept component lies inside one region: count it there
    for (int p = tid; p < n; p += 256)
      if (lev[p] == p && t16_get(bufA, p) >= a.npixels && reg[p] >= 0) t16_add(bufB, reg[p]);
    __syncthreads();
    // a region holding two or more is replaced by them
    for (int p = tid; p < n; p += 256) {
      const int R = reg[p];
      if (R < 0 || t16_get(bufB, R) < 2) continue;
      const int l = lev[p];
      reg[p] = (l >= 0 && t16_get(bufA, l) >= a.npixels) ? (short)l : (short)kFree;
      sint[1] = 1;
    }
    __syncthreads();
  }
  if (!sint[1]) return;

  // the markers, in raster order
  short* mk = reinterpret_cast<short*>(bufA);
  short* hp = reinterpret_cast<short*>(bufB);
  for (int p = tid; p < n; p += 256) lev[p] = reg[p];
  if (wave == 0) {
    int nm = 0;
    for (int base = 0; base < n; base += 64) {
      const int p = base + lane;
      const bool f = p < n && reg[p] == p;
      const unsigned long long bal = __ballot(f);
      if (f) mk[nm + __popcll(bal & ((1ull << lane) - 1ull))] = (short)p;
      nm += __popcll(bal);
    }
    if (lane == 0) sint[2] = nm;
  }
  __syncthreads();
  const int nm = sint[2];
  int alive = nm;

  // D5, D6
  for (;;) {
    if (tid == 0) {
      db_flood(v, lev, hp, bw, bh, a.conn);
      sint[3] = 0;
    }
    __syncthreads();
    double bf = dev_inf();
    int bc = 0x7fffffff, below = 0;
    for (int ci = wave; ci < nm; ci += 4) {
      const int c = mk[ci];
      if (c < 0) continue;
      const double frac = db_wave_sum_of(v, lev, c, n) / ssum;
      if (frac < a.contrast) below = 1;
      if (frac < bf || (frac == bf && c < bc)) bf = frac, bc = c;
    }
    if (lane == 0) {
      sred[4 + wave] = bf, sint[4 + wave] = bc;
      if (below) atomicOr(&sint[3], 1);
    }
    __syncthreads();
    if (!sint[3]) break;
    bf = sred[4], bc = sint[4];
    for (int k = 1; k < 4; ++k) {
      const double f = sred[4 + k];
      const int c = sint[4 + k];
      if (f < bf || (f == bf && c < bc)) bf = f, bc = c;
    }
    for (int p = tid; p < n; p += 256)
      if (lev[p] == bc) lev[p] = kFree;
    for (int ci = tid; ci < nm; ci += 256)
      if (mk[ci] == bc) mk[ci] = -1;
    --alive;
    __syncthreads();
    if (alive < 2) break;  // one child or none: the parent stays
  }
  if (alive < 2) return;

  // child ranks in marker order, into labels_out (k_deblend_relabel adds the base)
  if (wave == 0) {
    int r = 0;
    for (int base = 0; base < nm; base += 64) {
      const int ci = base + lane;
      const int c = ci < nm ? mk[ci] : -1;
      const unsigned long long bal = __ballot(c >= 0);
      if (c >= 0) hp[c] = (short)(r + __popcll(bal & ((1ull << lane) - 1ull)));
      r += __popcll(bal);
    }
  }
  __syncthreads();
  for (int k = tid; k < n; k += 256) {
    const int l = lev[k];
    if (l == kOutside) continue;
    const int r = k / bw, c = k - r * bw;
    // a pixel the flood did not reach (connectivity 4 inside an 8-connected
    // parent) is dropped, as the watershed leaves it 0
    a.labels_out[o + (size_t)(y0 + r) * a.W + (x0 + c)] = l >= 0 ? hp[l] : -1;
  }
  if (tid == 0) a.nchild[row] = alive;
}

// ---- parents over the LDS cap: the same steps with the working set in global
// memory, keyed by image pixel (DeblendArgs).  Boxes of parents overlap, their
// pixel sets do not: a parent writes its own pixels' entries before it reads
// them and reads a neighbour's only after labels[q] == want, so the arrays are
// shared by all parents of a call and never initialised.  Identities are pixel
// indices of the image, whose order inside a box is the box's raster order;
// every float sum runs over box indices k with stride 64, as in k_deblend_parent.
namespace {

constexpr int kHeapLds = 5120;               // heap entries in LDS: the heap's first levels
constexpr int kAccSlots = kHeapLds / 64 / 4;  // D6: children one wave sums in one pass over the box

// the arrays integer atomics write are read (uf_load<kAgent>) and written at the
// scope of those atomics
__device__ __forceinline__ void gl_store(int* p, int v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The flood's heap: entries (value, pixel) in db_before's order, the key inside
// the entry.  Entry i < kHeapLds lives in LDS, the others in the parent's slice
// of the global arrays (at most `area` entries: a pixel enters at most once).
struct LHeap {
  double* lk;
  int* li;
  double* gk;
  int* gi;
  __device__ __forceinline__ void get(int i, double& v, int& p) const {
    if (i < kHeapLds) v = lk[i], p = li[i];
    else v = gk[i], p = gi[i];
  }
  __device__ __forceinline__ void set(int i, double v, int p) const {
    if (i < kHeapLds) lk[i] = v, li[i] = p;
    else gk[i] = v, gi[i] = p;
  }
};

__device__ __forceinline__ bool lh_before(double x, int a, double y, int b) {
  return x > y || (x == y && a < b);
}

// entry (v, p) sinks from the hole at i
__device__ __forceinline__ void lh_sift_down(const LHeap& h, int n, int i, double v, int p) {
  for (;;) {
    int c = 2 * i + 1;
    if (c >= n) break;
    double cv;
    int cp;
    h.get(c, cv, cp);
    if (c + 1 < n) {
      double v2;
      int p2;
      h.get(c + 1, v2, p2);
      if (lh_before(v2, p2, cv, cp)) ++c, cv = v2, cp = p2;
    }
    if (!lh_before(cv, cp, v, p)) break;
    h.set(i, cv, cp);
    i = c;
  }
  h.set(i, v, p);
}

__device__ __forceinline__ void lh_push(const LHeap& h, int& n, double v, int p) {
  int i = n++;
  while (i > 0) {
    const int up = (i - 1) >> 1;
    double uv;
    int uq;
    h.get(up, uv, uq);
    if (!lh_before(v, p, uv, uq)) break;
    h.set(i, uv, uq);
    i = up;
  }
  h.set(i, v, p);
}

// image pixel of box pixel k
struct LBox {
  int x0, y0, bw, W;
  __device__ __forceinline__ int pix(int k) const {
    const int r = k / bw;
    return (y0 + r) * W + x0 + (k - r * bw);
  }
};

}  // namespace

__global__ void __launch_bounds__(256) k_deblend_large(DeblendArgs a) {
  __shared__ double lk[kHeapLds];  // D5: heap keys; D6: lane partials [wave][slot][lane]
  __shared__ int li[kHeapLds];     // D5: heap pixels
  __shared__ double thr[256];
  __shared__ double sred[8];
  __shared__ int sint[12];
  __shared__ unsigned long long soff;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i = blockIdx.x, b = blockIdx.y;
  if (i >= db_rows(a, b)) return;
  const size_t row = (size_t)b * a.cap + i;
  const int* ic = a.icols + row * 5;
  const int area = ic[0];
  if (area <= 0 || area < 2 * (long long)a.npixels || (a.sel && !a.sel[row])) return;
  const int x0 = ic[1], y0 = ic[3], bw = ic[2] - x0 + 1, bh = ic[4] - y0 + 1;
  if (x0 < 0 || y0 < 0 || bw < 1 || bh < 1 || ic[2] >= a.W || ic[4] >= a.H) return;
  if ((long long)bw * bh <= a.lds_max_box) return;  // k_deblend_parent's
  if (area > kDeblendLargeMaxArea) {
    if (tid == 0) atomicOr(a.status + b, BSGP_DEBLEND_OVER_CAP);
    return;
  }
  const int n = bw * bh, want = i + 1, hw = a.H * a.W;  // the box lies in the image: n <= hw < 2^31
  const size_t o = (size_t)b * hw;
  const LBox bx{x0, y0, bw, a.W};
  const int* labs = a.labels + o;
  const double* dat = a.data + o;
  int *lev = a.lev + o, *reg = a.reg + o, *cnt = a.cnt + o, *kept = a.kept + o;
  int* fl = a.labels_out + o;  // D5: flood labels; then the child ranks

  // the parent's slice of the marker and heap arrays starts at the sum of the
  // image's lower areas; the root; the pixel count that slice relies on
  if (tid == 0) sint[0] = hw, sint[1] = 0, sint[5] = 0, sint[6] = 0, soff = 0ull;
  __syncthreads();
  {
    unsigned long long part = 0ull;
    for (int j = tid; j < i; j += 256) {
      const int ar = a.icols[((size_t)b * a.cap + j) * 5];
      part += ar > 0 ? (unsigned long long)(ar < hw ? ar : hw) : 0ull;
    }
    if (part) atomicAdd(&soff, part);
    int own = 0, mn = hw;
    for (int k = tid; k < n; k += 256) {
      const int q = bx.pix(k);
      if (labs[q] != want) continue;
      ++own;
      mn = q < mn ? q : mn;
    }
    if (own) atomicAdd(&sint[6], own), atomicMin(&sint[0], mn);
  }
  __syncthreads();
  const int root0 = sint[0];
  // int_cols that do not describe labels: the slice is not the parent's
  if (sint[6] != area || soff + (unsigned long long)area > (unsigned long long)hw) return;
  const size_t off = o + (size_t)soff;
  int* mk = a.mk + off;
  const LHeap heap{lk, li, a.hkey + off, a.hidx + off};
  for (int k = tid; k < n; k += 256) {
    const int q = bx.pix(k);
    if (labs[q] == want) reg[q] = root0;
  }

  // D1
  if (wave == 0) {
    double s = 0.0, mn = dev_inf(), mx = -dev_inf();
    for (int k = lane; k < n; k += 64) {
      const int q = bx.pix(k);
      if (labs[q] != want) continue;
      const double x = dat[q];
      s += x;
      mn = x < mn ? x : mn;
      mx = x > mx ? x : mx;
    }
    s = wave_sum(s);
    mn = wave_min(mn);
    mx = wave_max(mx);
    if (lane == 0) sred[0] = mn, sred[1] = mx, sred[2] = s;
  }
  __syncthreads();
  const double smin = sred[0], smax = sred[1], ssum = sred[2];
  if (!(smin < smax)) return;

  // D2 to D4
  const bool linear = a.mode == BSGP_DEBLEND_LINEAR || smin < 0.0;
  const double m = smin != 0.0 ? smin : 0.01 * smax;
  const double den = (double)(a.nlevels + 1);
  for (int lv = 1; lv <= a.nlevels; ++lv) {
    if (((lv - 1) & 255) == 0) {
      const double k = (double)(lv + tid);
      thr[tid] = linear ? smin + (smax - smin) / den * k : m * pow(smax / m, k / den);
      __syncthreads();
    }
    const double t = thr[(lv - 1) & 255];
    int above = 0;
    for (int k = tid; k < n; k += 256) {
      const int q = bx.pix(k);
      if (labs[q] != want) continue;
      const bool on = dat[q] > t;
      gl_store(lev + q, on ? q : -1);
      gl_store(cnt + q, 0);
      gl_store(kept + q, 0);
      above += on;
    }
    if (above) atomicAdd(&sint[5], above);
    __syncthreads();
    if (sint[5] < 2 * (long long)a.npixels) break;
    for (int k = tid; k < n; k += 256) {
      const int y = k / bw, x = k - y * bw, p = (y0 + y) * a.W + x0 + x, q = p - a.W;
      if (labs[p] != want || uf_load<kAgent>(lev + p) < 0) continue;
      const bool w = x > 0 && labs[p - 1] == want && uf_load<kAgent>(lev + p - 1) >= 0;
      const bool nn = y > 0 && labs[q] == want && uf_load<kAgent>(lev + q) >= 0;
      if (a.conn == 4) {
        if (w) uf_unite<kAgent>(lev, p, p - 1);
        if (nn) uf_unite<kAgent>(lev, p, q);
        continue;
      }
      if (nn) {
        uf_unite<kAgent>(lev, p, q);
        continue;
      }
      const bool nw = y > 0 && x > 0 && labs[q - 1] == want && uf_load<kAgent>(lev + q - 1) >= 0;
      const bool ne =
          y > 0 && x < bw - 1 && labs[q + 1] == want && uf_load<kAgent>(lev + q + 1) >= 0;
      if (ne) uf_unite<kAgent>(lev, p, q + 1);
      if (nw) uf_unite<kAgent>(lev, p, q - 1);
      else if (w) uf_unite<kAgent>(lev, p, p - 1);
    }
    __syncthreads();
    for (int k = tid; k < n; k += 256) {
      const int p = bx.pix(k);
      if (labs[p] != want || uf_load<kAgent>(lev + p) < 0) continue;
      const int r = uf_find<kAgent>(lev, p);
      if (r != p) gl_store(lev + p, r);
      atomicAdd(cnt + r, 1);
    }
    if (tid == 0) sint[5] = 0;  // every thread read it before the barrier above
    __syncthreads();
    for (int k = tid; k < n; k += 256) {
      const int p = bx.pix(k);
      if (labs[p] != want) continue;
      if (uf_load<kAgent>(lev + p) == p && uf_load<kAgent>(cnt + p) >= a.npixels && reg[p] >= 0)
        atomicAdd(kept + reg[p], 1);
    }
    __syncthreads();
    for (int k = tid; k < n; k += 256) {
      const int p = bx.pix(k);
      if (labs[p] != want) continue;
      const int R = reg[p];
      if (R < 0 || uf_load<kAgent>(kept + R) < 2) continue;
      const int l = uf_load<kAgent>(lev + p);
      reg[p] = (l >= 0 && uf_load<kAgent>(cnt + l) >= a.npixels) ? l : kFree;
      sint[1] = 1;
    }
    __syncthreads();
  }
  if (!sint[1]) return;

  // the markers, in raster order; kept[c] = the list index of marker c
  for (int k = tid; k < n; k += 256) {
    const int p = bx.pix(k);
    if (labs[p] == want) fl[p] = reg[p];
  }
  if (wave == 0) {
    int nm = 0;
    for (int base = 0; base < n; base += 64) {
      const int k = base + lane, p = k < n ? bx.pix(k) : 0;
      const bool f = k < n && labs[p] == want && reg[p] == p;
      const unsigned long long bal = __ballot(f);
      if (f) {
        const int ci = nm + __popcll(bal & ((1ull << lane) - 1ull));
        mk[ci] = p;
        gl_store(kept + p, ci);
      }
      nm += __popcll(bal);
    }
    if (lane == 0) sint[2] = nm;
  }
  __syncthreads();
  const int nm = sint[2];
  int alive = nm;

  // D5, D6
  for (;;) {
    // the frontier, labelled pixels with a free neighbour, by all threads; the
    // heap's order is total and strict, so the pops do not depend on the order
    // the entries arrive in
    if (tid == 0) sint[8] = 0;
    __syncthreads();
    for (int k = tid; k < n; k += 256) {
      const int y = k / bw + y0, x = k - (k / bw) * bw + x0, p = y * a.W + x;
      if (labs[p] != want || fl[p] < 0) continue;
      bool open = false;
      for (int j = 0; j < 8; ++j) {
        const int jj = j < 4 ? j : j + 1;
        const int dy = jj / 3 - 1, dx = jj - (jj / 3) * 3 - 1;
        if (a.conn == 4 && dx != 0 && dy != 0) continue;
        const int xx = x + dx, yy = y + dy;
        if (xx < 0 || xx >= a.W || yy < 0 || yy >= a.H) continue;
        const int q = p + dy * a.W + dx;
        if (labs[q] == want && fl[q] == kFree) open = true;
      }
      if (open) heap.set(atomicAdd(&sint[8], 1), dat[p], p);
    }
    __syncthreads();
    int hn = sint[8];
    // heapify: the nodes of one depth sink at once, their subtrees are disjoint
    for (int d = 30 - __clz(hn | 1); d >= 0; --d) {
      const int lo = (1 << d) - 1, hi = 2 * lo + 1 < hn ? 2 * lo + 1 : hn;
      for (int j = lo + tid; j < hi; j += 256) {
        double v;
        int p;
        heap.get(j, v, p);
        lh_sift_down(heap, hn, j, v, p);
      }
      __syncthreads();
    }
    if (tid == 0) {
      while (hn > 0) {
        double v, lv;
        int p, lp;
        heap.get(0, v, p);
        heap.get(--hn, lv, lp);
        if (hn > 0) lh_sift_down(heap, hn, 0, lv, lp);
        const int y = p / a.W, x = p - y * a.W, l = fl[p];
        // the eight neighbours' label, flood label and value in one batch of
        // independent loads (the lane waits once, not per neighbour); a
        // neighbour outside the image reads p itself, which is labelled
        int nq[8], nl[8], nf[8];
        double nv[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int jj = j < 4 ? j : j + 1;
          const int dy = jj / 3 - 1, dx = jj - (jj / 3) * 3 - 1;
          const int xx = x + dx, yy = y + dy;
          const bool ok = !(a.conn == 4 && dx != 0 && dy != 0) && xx >= 0 && xx < a.W && yy >= 0 &&
                          yy < a.H;
          nq[j] = ok ? p + dy * a.W + dx : p;
          nl[j] = labs[nq[j]];
          nf[j] = fl[nq[j]];
          nv[j] = dat[nq[j]];
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          if (nl[j] == want && nf[j] == kFree) {
            fl[nq[j]] = l;
            lh_push(heap, hn, nv[j], nq[j]);
          }
        }
      }
      sint[3] = 0;
    }
    __syncthreads();
    // every child's fraction: a wave takes kAccSlots children per pass over the
    // box, lane partials in box raster order with stride 64 (db_wave_sum_of's sums)
    double bf = dev_inf();
    int bc = 0x7fffffff, below = 0;
    double* acc = lk + wave * (kAccSlots * 64);
    for (int base = wave * kAccSlots; base < nm; base += 4 * kAccSlots) {
      const int ng = nm - base < kAccSlots ? nm - base : kAccSlots;
      for (int s = 0; s < ng; ++s) acc[s * 64 + lane] = 0.0;
      for (int k = lane; k < n; k += 64) {
        const int p = bx.pix(k);
        if (labs[p] != want) continue;
        const int l = fl[p];
        if (l < 0) continue;
        const int s = uf_load<kAgent>(kept + l) - base;
        if (s >= 0 && s < ng) acc[s * 64 + lane] += dat[p];
      }
      for (int s = 0; s < ng; ++s) {
        const int c = mk[base + s];
        if (c < 0) continue;
        const double frac = wave_sum(acc[s * 64 + lane]) / ssum;
        if (frac < a.contrast) below = 1;
        if (frac < bf || (frac == bf && c < bc)) bf = frac, bc = c;
      }
    }
    if (lane == 0) {
      sred[4 + wave] = bf, sint[4 + wave] = bc;
      if (below) atomicOr(&sint[3], 1);
    }
    __syncthreads();
    if (!sint[3]) break;
    bf = sred[4], bc = sint[4];
    for (int k = 1; k < 4; ++k) {
      const double f = sred[4 + k];
      const int c = sint[4 + k];
      if (f < bf || (f == bf && c < bc)) bf = f, bc = c;
    }
    for (int k = tid; k < n; k += 256) {
      const int p = bx.pix(k);
      if (labs[p] == want && fl[p] == bc) fl[p] = kFree;
    }
    for (int ci = tid; ci < nm; ci += 256)
      if (mk[ci] == bc) mk[ci] = -1;
    --alive;
    __syncthreads();
    if (alive < 2) break;  // one child or none: the parent stays
  }
  if (alive < 2) return;

  // child ranks in marker order (kept[c]), into labels_out
  if (wave == 0) {
    int r = 0;
    for (int base = 0; base < nm; base += 64) {
      const int ci = base + lane;
      const int c = ci < nm ? mk[ci] : -1;
      const unsigned long long bal = __ballot(c >= 0);
      if (c >= 0) gl_store(kept + c, r + __popcll(bal & ((1ull << lane) - 1ull)));
      r += __popcll(bal);
    }
  }
  __syncthreads();
  for (int k = tid; k < n; k += 256) {
    const int p = bx.pix(k);
    if (labs[p] != want) continue;
    const int l = fl[p];
    fl[p] = l >= 0 ? uf_load<kAgent>(kept + l) : -1;
  }
  if (tid == 0) a.nchild[row] = alive;
}

// D7: parents left as they are first, in label order, then the children by parent
__global__ void __launch_bounds__(256) k_deblend_number(DeblendArgs a) {
  __shared__ int wsum[4];
  const int b = blockIdx.x, n = db_rows(a, b);
  const size_t row0 = (size_t)b * a.cap;
  int cu = 0, cc = 0;
  for (int base = 0; base < n; base += 256) {
    const int i = base + threadIdx.x;
    const bool valid = i < n && a.icols[(row0 + i) * 5] > 0;
    const int c = valid ? a.nchild[row0 + i] : 0;
    const int u = valid && c == 0;
    int tu, tc;
    const int eu = block_scan(u, wsum, &tu), ec = block_scan(c, wsum, &tc);
    if (i < n) a.base[row0 + i] = !valid ? 0 : (u ? cu + eu + 1 : cc + ec);
    cu += tu;
    cc += tc;
  }
  for (int i = threadIdx.x; i < n; i += 256)
    if (a.nchild[row0 + i] > 0) a.base[row0 + i] += cu + 1;
  if (threadIdx.x == 0) a.nlabels_out[b] = cu + cc;
}

__global__ void __launch_bounds__(256) k_deblend_relabel(DeblendArgs a) {
  const int hw = a.H * a.W;
  const unsigned pu = blockIdx.x * 256u + threadIdx.x;
  if (pu >= (unsigned)hw) return;
  const int b = blockIdx.y;
  const size_t q = (size_t)b * hw + pu;
  const int l = a.labels[q];
  int out = 0;
  if (l < 0 || l > db_rows(a, b)) {
    atomicOr(a.status + b, BSGP_DEBLEND_BAD_LABEL);
  } else if (l > 0) {
    const size_t row = (size_t)b * a.cap + (l - 1);
    const int base = a.base[row];
    if (a.nchild[row] == 0) {
      out = base;
    } else {
      const int r = a.labels_out[q];
      out = r < 0 ? 0 : base + r;
    }
  }
  a.labels_out[q] = out;
}

hipError_t launch_deblend(const DeblendArgs& a, hipStream_t s) {
  const int hw = a.H * a.W;
  const dim3 block(256);
  hipLaunchKernelGGL(k_deblend_parent, dim3(a.cap, a.B), block, 0, s, a);
  if (a.large) hipLaunchKernelGGL(k_deblend_large, dim3(a.cap, a.B), block, 0, s, a);
  hipLaunchKernelGGL(k_deblend_number, dim3(a.B), block, 0, s, a);
  hipLaunchKernelGGL(k_deblend_relabel, dim3((unsigned)(((size_t)hw + 255) / 256), a.B), block, 0,
                     s, a);
  return hipGetLastError();
}

}  // namespace bsgp
