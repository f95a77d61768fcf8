// bsgp_starfind.hip — finding and measuring the stars of a frame: what the
// reference leaves to DIAPL's sfind and fwhmm (psf/psf_estimation.bash with the
// parameters of psf/psf_steps_and_params.MD), and the choice of PSF stars that
// getpsf makes before it fits (include/bsgp.h and DESIGN §3.15, F1 to F10).
//
//  k_star_maps<T>   a 32 x 16 tile of output pixels per 256-thread workgroup,
//                 two per lane.  The tile and its halo of R are staged in LDS
//                 as float64, a pixel that is outside the frame, not finite
//                 or masked as NaN; the template is staged beside it.  Each
//                 lane runs the whole F3 loop for its pixels in the support's
//                 row-major order, so a sum does not depend on the tiling.
//  k_star_peaks<T>  F4 on the maps, a lane per 8 consecutive pixels of a chunk
//                 of 2048: correlation, the window maximum of amp with the
//                 raster-order tie rule, and for the pixels that pass both the
//                 matched filter's sum again from the frame (the same
//                 operations in the same order as the map's) for the
//                 significance test.  Writes a byte of flags per lane and the
//                 chunk's count.
//  k_star_scan    one workgroup per frame: exclusive scan of the chunk counts,
//                 the frame's count and its OVER_CAP bit.
//  k_star_write   a chunk's candidates at their raster-order rank (block_scan
//                 over the flag bytes): the compaction of bsgp_segment.hip.
//  k_star_measure<T>  one workgroup per (star, frame).  The annulus is
//                 gathered into dynamic LDS as k_localbkg does, sorted and
//                 clipped through bsgp_sigclip.hpp (F6); then one lane per
//                 support row adds the row's aperture sums left to right and
//                 lane 0 adds the rows top to bottom (F7) and sets the bits
//                 (F8).
//  k_star_select  F9 in two launches, a lane per star, all stars passing
//                 through LDS in tiles of 256: eligibility (isolation against
//                 every kept star), then the rank among the eligible.
#include <hip/hip_runtime.h>

#include <cmath>

#include "bsgp_apps.hpp"
#include "bsgp_prims.hpp"
#include "bsgp_reduce.hpp"
#include "bsgp_sigclip.hpp"

#pragma clang fp contract(off)

namespace bsgp {

namespace {
constexpr int kMapTX = 32, kMapTY = 16;  // output pixels of one workgroup
constexpr int kMapLds = (kMapTX + 2 * kStarMaxR) * (kMapTY + 2 * kStarMaxR);
constexpr int kStarRows = 2 * kStarMaxR + 1;
constexpr int kStarMaxN = kStarRows * kStarRows;
constexpr int kStarLimit = 1 << 30;  // |box centre| of F9: centre +- hw stays an int
constexpr double kSigmaToFwhm = 2.3548200450309493;  // 2 sqrt(2 ln 2)
}  // namespace

// ------------------------------------------------------------------ F2, F3
template <typename T>
__global__ void __launch_bounds__(256) k_star_maps(StarMapArgs a) {
  __shared__ double tile[kMapLds];
  __shared__ double st[kStarMaxN];
  __shared__ int shw[kStarRows];
  const int tid = threadIdx.x, b = blockIdx.z, R = a.tp.R, n = a.tp.n;
  const int x0 = blockIdx.x * kMapTX, y0 = blockIdx.y * kMapTY;
  const int LW = kMapTX + 2 * R, LH = kMapTY + 2 * R;
  const size_t img_off = (size_t)b * a.H * a.W;
  const T* img = static_cast<const T*>(a.data) + img_off;
  const unsigned char* mask = a.mask ? a.mask + img_off : nullptr;
  for (int k = tid; k < n; k += 256) st[k] = a.tp.t[k];
  if (tid < 2 * R + 1) shw[tid] = a.tp.halfw[tid];
  for (int k = tid; k < LW * LH; k += 256) {
    const int ly = k / LW, lx = k - ly * LW, y = y0 - R + ly, x = x0 - R + lx;
    double v = dev_nan();
    if (y >= 0 && y < a.H && x >= 0 && x < a.W) {
      const size_t o = (size_t)y * a.W + x;
      const double u = (double)img[o];
      if (__builtin_isfinite(u) && !(mask && mask[o])) v = u;
    }
    tile[k] = v;
  }
  __syncthreads();

  const int lx = tid & 31, ly = tid >> 5;  // the lane's pixels: rows ly and ly + 8 of the tile
  double s1[2] = {0.0, 0.0}, s2[2] = {0.0, 0.0}, sc[2] = {0.0, 0.0};
  bool bad[2] = {false, false};
  int k = 0;
  for (int r = 0; r <= 2 * R; ++r) {
    const int w = shw[r];
    const double* ra = tile + (ly + r) * LW + lx + R;
    const double* rb = ra + 8 * LW;
    for (int dx = -w; dx <= w; ++dx, ++k) {
      const double t = st[k], va = ra[dx], vb = rb[dx];
      bad[0] |= va != va;
      bad[1] |= vb != vb;
      s1[0] += va;
      s1[1] += vb;
      s2[0] += va * va;
      s2[1] += vb * vb;
      sc[0] += t * va;
      sc[1] += t * vb;
    }
  }
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int y = y0 + ly + 8 * q, x = x0 + lx;
    if (y >= a.H || x >= a.W) continue;
    double corr = dev_nan(), amp = dev_nan();
    if (!bad[q]) {
      const double var = s2[q] - s1[q] * s1[q] / (double)n;
      amp = sc[q] / a.tp.tt;
      corr = var > 0.0 ? sc[q] / sqrt(a.tp.tt * var) : 0.0;
    }
    const size_t o = img_off + (size_t)y * a.W + x;
    a.corr[o] = corr;
    a.amp[o] = amp;
  }
}

// ---------------------------------------------------------------------- F4
namespace {

template <typename T>
__device__ __forceinline__ bool star_candidate(const StarPeakArgs& a, int b, int p) {
  const size_t img_off = (size_t)b * a.H * a.W;
  const double* A = a.amp + img_off;
  const double amp = A[p];
  if (!(amp == amp)) return false;
  if (!(a.corr[img_off + p] >= a.c_min)) return false;
  const int y = p / a.W, x = p - y * a.W, R = a.tp.R;
  if (y < R || y >= a.H - R || x < R || x >= a.W - R) return false;  // maps not k_star_maps'
  for (int wy = -a.peak_hw; wy <= a.peak_hw; ++wy) {
    const int yy = y + wy;
    if (yy < 0 || yy >= a.H) continue;
    for (int wx = -a.peak_hw; wx <= a.peak_hw; ++wx) {
      const int xx = x + wx;
      if (xx < 0 || xx >= a.W || (wy == 0 && wx == 0)) continue;
      const double u = A[(size_t)yy * a.W + xx];
      if (u != u) continue;
      const bool earlier = wy < 0 || (wy == 0 && wx < 0);
      if (earlier ? !(amp > u) : !(amp >= u)) return false;
    }
  }
  // the matched filter's sum as k_star_maps added it (a valid pixel: its
  // support is inside the frame)
  const T* img = static_cast<const T*>(a.data) + img_off;
  double sc = 0.0;
  int k = 0;
  for (int r = 0; r <= 2 * R; ++r) {
    const int w = a.tp.halfw[r];
    const T* row = img + (size_t)(y + r - R) * a.W + x;
    for (int dx = -w; dx <= w; ++dx, ++k) sc += a.tp.t[k] * (double)row[dx];
  }
  const double noise = a.noise_map ? a.noise[img_off + p] : a.noise[b];
  return sc >= (a.thresh * noise) * a.tp.sqrt_tt;
}

}  // namespace

template <typename T>
__global__ void __launch_bounds__(256) k_star_peaks(StarPeakArgs a) {
  __shared__ int wsum[4];
  const int b = blockIdx.y, hw = a.H * a.W;
  const unsigned p0 = blockIdx.x * (unsigned)kStarChunk + threadIdx.x * 8u;
  unsigned bits = 0;
  int c = 0;
  for (int k = 0; k < 8; ++k) {
    const unsigned p = p0 + k;
    if (p < (unsigned)hw && star_candidate<T>(a, b, (int)p)) {
      bits |= 1u << k;
      ++c;
    }
  }
  const size_t chunk = (size_t)b * a.nblk + blockIdx.x;
  a.flag[chunk * 256 + threadIdx.x] = (unsigned char)bits;
  int total;
  (void)block_scan(c, wsum, &total);
  if (threadIdx.x == 0) a.blk[chunk] = total;
}

// F5: one workgroup per frame, exclusive scan of its chunk counts, in place
__global__ void __launch_bounds__(256) k_star_scan(StarPeakArgs a) {
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
  if (threadIdx.x == 0) {
    a.n[b] = carry < a.cap ? carry : a.cap;
    a.status[b] = carry > a.cap ? BSGP_STARFIND_OVER_CAP : 0;
  }
}

__global__ void __launch_bounds__(256) k_star_write(StarPeakArgs a) {
  __shared__ int wsum[4];
  const int b = blockIdx.y, hw = a.H * a.W;
  const size_t chunk = (size_t)b * a.nblk + blockIdx.x;
  const unsigned p0 = blockIdx.x * (unsigned)kStarChunk + threadIdx.x * 8u;
  const unsigned bits = a.flag[chunk * 256 + threadIdx.x];
  int total;
  int rank = a.blk[chunk] + block_scan(__popc(bits), wsum, &total);
  for (int k = 0; k < 8; ++k) {
    const unsigned p = p0 + k;
    if (!(bits >> k & 1u) || p >= (unsigned)hw) continue;
    if (rank < a.cap) {
      int* out = a.peaks + ((size_t)b * a.cap + rank) * 2;
      out[0] = (int)(p % (unsigned)a.W);
      out[1] = (int)(p / (unsigned)a.W);
    }
    ++rank;
  }
}

// --------------------------------------------------------------- F6 to F8
// lds_cap: the values the dynamic LDS holds, a power of two that holds the
// whole annulus unless that has more than kLocalBkgMax pixels
template <typename T>
__global__ void __launch_bounds__(256) k_star_measure(StarMeasureArgs a, int lds_cap) {
  extern __shared__ double s[];
  __shared__ double red[(kWaves + 1) * kMaxRed];
  __shared__ int count;
  __shared__ double rsum[kStarRows][6];
  __shared__ double rmax[kStarRows];
  __shared__ int rarg[kStarRows], rsat[kStarRows];
  const int tid = threadIdx.x, lane = tid & 63, star = blockIdx.x, b = blockIdx.y;
  int nr = a.n[b];
  nr = nr < a.cap ? nr : a.cap;
  if (star >= nr) return;
  const size_t rr = (size_t)b * a.cap + star;
  const int ic = a.peaks[2 * rr], ir = a.peaks[2 * rr + 1];
  const size_t img_off = (size_t)b * a.H * a.W;
  const T* img = static_cast<const T*>(a.data) + img_off;
  const unsigned char* mask = a.mask ? a.mask + img_off : nullptr;
  const int R = a.R;
  if (ic < R || ic >= a.W - R || ir < R || ir >= a.H - R) {  // not a peak of k_star_peaks
    if (tid == 0) {
      int* icol = a.icols + rr * 4;
      icol[0] = ic, icol[1] = ir, icol[2] = 0, icol[3] = BSGP_STARFIND_BAD_FLUX;
    }
    return;
  }

  // F6: gather the annulus (its bounding box clipped to the frame)
  if (tid == 0) count = 0;
  __syncthreads();
  const int xa = ic - a.box > 0 ? ic - a.box : 0, xb = ic + a.box < a.W - 1 ? ic + a.box : a.W - 1;
  const int ya = ir - a.box > 0 ? ir - a.box : 0, yb = ir + a.box < a.H - 1 ? ir + a.box : a.H - 1;
  const int rw = xb - xa + 1, nrect = rw * (yb - ya + 1);
  for (int k0 = 0; k0 < nrect; k0 += 256) {
    const int k = k0 + tid;
    bool pass = false;
    double u = 0.0;
    if (k < nrect) {
      const int yy = k / rw, dy = ya + yy - ir, dx = xa + (k - yy * rw) - ic;
      const double d2 = (double)(dx * dx + dy * dy);
      if (d2 >= a.r1sq && d2 <= a.r2sq) {
        const size_t o = (size_t)(ir + dy) * a.W + (ic + dx);
        u = (double)img[o];
        pass = __builtin_isfinite(u) && !(mask && mask[o]) && !(a.has_sat && u >= a.sat_level);
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
  const int nsky = count;
  int status = 0;
  double bkg = dev_nan();
  if (nsky > lds_cap) {
    status |= BSGP_STARFIND_SKY_OVER_CAP;
  } else if (nsky < a.min_sky) {
    status |= BSGP_STARFIND_FEW_SKY;
  } else {
    int P = 1;
    while (P < nsky) P <<= 1;
    for (int k = nsky + tid; k < P; k += 256) s[k] = dev_inf();
    __syncthreads();
    bkg_sort(s, P);
    const SigClip c = sigma_clip_sorted(s, nsky, a.sigma, a.maxiters, red);
    if (a.bkg_alg == BSGP_STARFIND_BKG_MEDIAN)
      bkg = c.med;
    else if (a.bkg_alg == BSGP_STARFIND_BKG_MEAN)
      bkg = c.mean;
    else if (c.sd == 0.0)
      bkg = c.mean;
    else if (fabs(c.mean - c.med) / c.sd < 0.3)
      bkg = 2.5 * c.med - 1.5 * c.mean;
    else
      bkg = c.med;
  }

  // F7: a lane per support row, left to right
  if (tid < 2 * R + 1) {
    const int dy = tid - R, w = a.halfw[tid];
    const T* row = img + (size_t)(ir + dy) * a.W + ic;
    double f = 0.0, sx = 0.0, sy = 0.0, sxx = 0.0, syy = 0.0, sxy = 0.0, mx = 0.0;
    int arg = 0, ns = 0;
    for (int dx = -w; dx <= w; ++dx) {
      const double I = (double)row[dx], J = I - bkg;
      f += J;
      sx += (double)dx * J;
      sy += (double)dy * J;
      sxx += (double)(dx * dx) * J;
      syy += (double)(dy * dy) * J;
      sxy += (double)(dx * dy) * J;
      if (dx == -w || I > mx) mx = I, arg = dx;
      if (a.has_sat && I >= a.sat_level) ++ns;
    }
    rsum[tid][0] = f, rsum[tid][1] = sx, rsum[tid][2] = sy;
    rsum[tid][3] = sxx, rsum[tid][4] = syy, rsum[tid][5] = sxy;
    rmax[tid] = mx, rarg[tid] = arg, rsat[tid] = ns;
  }
  __syncthreads();
  if (tid != 0) return;
  double S[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, mx = 0.0;
  int bx = 0, by = 0, nsat = 0;
  for (int r = 0; r <= 2 * R; ++r) {
#pragma unroll
    for (int q = 0; q < 6; ++q) S[q] += rsum[r][q];
    if (r == 0 || rmax[r] > mx) mx = rmax[r], bx = rarg[r], by = r - R;
    nsat += rsat[r];
  }
  const double F = S[0], mxx = S[1] / F, myy = S[2] / F;
  const double x = (double)ic + mxx, y = (double)ir + myy;
  const double arg = ((S[3] / F - mxx * mxx) + (S[4] / F - myy * myy)) / 2.0;
  const double fwhm = arg > 0.0 ? kSigmaToFwhm * sqrt(arg) : dev_nan();
  // F8
  if (!(__builtin_isfinite(F) && F > 0.0)) status |= BSGP_STARFIND_BAD_FLUX;
  const double ex = (double)(ic + bx) - x, ey = (double)(ir + by) - y;
  if (ex * ex + ey * ey > a.dxy2) status |= BSGP_STARFIND_OFF_CENTRE;
  double* fc = a.fcols + rr * 8;
  fc[0] = x, fc[1] = y, fc[2] = F, fc[3] = bkg, fc[4] = mx - bkg;
  const size_t o = img_off + (size_t)ir * a.W + ic;
  fc[5] = a.corr[o], fc[6] = a.amp[o], fc[7] = fwhm;
  int* icol = a.icols + rr * 4;
  icol[0] = ic, icol[1] = ir, icol[2] = nsat, icol[3] = status;
}

// ---------------------------------------------------------------------- F9
namespace {
__device__ __forceinline__ int star_centre(double pos) {
  double e = floor(pos + 0.5);
  const double lim = (double)kStarLimit;
  e = e < -lim ? -lim : (e > lim ? lim : e);
  return (int)e;
}
}  // namespace

// phase 0: eligible; phase 1: rank and selected
__global__ void __launch_bounds__(256) k_star_select(StarSelectArgs a, int phase) {
  __shared__ double sx[256], sy[256], sf[256];
  __shared__ int sk[256];
  const int tid = threadIdx.x, b = blockIdx.y, i = blockIdx.x * 256 + tid;
  int nr = a.n ? a.n[b] : a.cap;
  nr = nr < a.cap ? (nr < 0 ? 0 : nr) : a.cap;
  if ((int)blockIdx.x * 256 >= nr) return;
  const size_t r0 = (size_t)b * a.cap;
  const bool own = i < nr;
  double x = 0.0, y = 0.0, flux = 0.0;
  bool pre = false;
  if (own) {
    const double* fc = a.fcols + (r0 + i) * 8;
    const int* icol = a.icols + (r0 + i) * 4;
    x = fc[0], y = fc[1], flux = fc[2];
    if (phase == 0) {
      pre = !(icol[3] & BSGP_STARFIND_REJECTED) && flux >= a.min_flux && icol[2] == 0 &&
            !(a.has_max_peak && !(fc[4] <= a.max_peak));
      if (pre) {  // fit_psf's P1: the whole box inside the frame
        const int cx = star_centre(x), cy = star_centre(y);
        pre = cx - a.hw >= 0 && cx + a.hw < a.W && cy - a.hw >= 0 && cy + a.hw < a.H;
      }
    } else {
      pre = a.eligible[r0 + i] != 0;
    }
  }
  bool iso = true;
  int rank = 0;
  for (int base = 0; base < nr; base += 256) {
    const int j = base + tid;
    if (j < nr) {
      const double* fc = a.fcols + (r0 + j) * 8;
      sx[tid] = fc[0], sy[tid] = fc[1], sf[tid] = fc[2];
      sk[tid] = phase == 0 ? !(a.icols[(r0 + j) * 4 + 3] & BSGP_STARFIND_REJECTED)
                           : a.eligible[r0 + j] != 0;
    }
    __syncthreads();
    if (pre) {
      const int m = nr - base < 256 ? nr - base : 256;
      for (int q = 0; q < m; ++q) {
        const int t = base + q;
        if (t == i || !sk[q]) continue;
        if (phase == 0) {
          if (sf[q] >= a.rat_thresh * flux) {
            const double dx = sx[q] - x, dy = sy[q] - y;
            if (dx * dx + dy * dy <= a.iso2) iso = false;
          }
        } else if (sf[q] > flux || (sf[q] == flux && t < i)) {
          ++rank;
        }
      }
    }
    __syncthreads();
  }
  if (!own) return;
  if (phase == 0) {
    a.eligible[r0 + i] = pre && iso;
  } else {
    a.rank[r0 + i] = pre ? rank : -1;
    a.selected[r0 + i] = pre && rank < a.npsf_max;
  }
}

// ----------------------------------------------------------------- launches
hipError_t launch_star_maps(const StarMapArgs& a, int f32, hipStream_t s) {
  const dim3 grid((a.W + kMapTX - 1) / kMapTX, (a.H + kMapTY - 1) / kMapTY, a.B);
  hipLaunchKernelGGL(f32 ? k_star_maps<float> : k_star_maps<double>, grid, dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_star_peaks(const StarPeakArgs& a, int f32, hipStream_t s) {
  const dim3 ch(a.nblk, a.B), block(256);
  hipLaunchKernelGGL(f32 ? k_star_peaks<float> : k_star_peaks<double>, ch, block, 0, s, a);
  hipLaunchKernelGGL(k_star_scan, dim3(a.B), block, 0, s, a);
  hipLaunchKernelGGL(k_star_write, ch, block, 0, s, a);
  return hipGetLastError();
}

int star_annulus_pixels(double r1sq, double r2sq, int box) {
  int64_t n = 0;
  for (int dy = -box; dy <= box; ++dy)
    for (int dx = -box; dx <= box; ++dx) {
      const double d2 = (double)((int64_t)dx * dx + (int64_t)dy * dy);
      n += d2 >= r1sq && d2 <= r2sq;
    }
  return n > 0x7fffffff ? 0x7fffffff : (int)n;
}

hipError_t launch_star_measure(const StarMeasureArgs& a, int f32, hipStream_t s) {
  const int ngeo = star_annulus_pixels(a.r1sq, a.r2sq, a.box);
  int lds_cap = 64;
  while (lds_cap < ngeo && lds_cap < kLocalBkgMax) lds_cap <<= 1;
  auto* kern = f32 ? k_star_measure<float> : k_star_measure<double>;
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                                     hipFuncAttributeMaxDynamicSharedMemorySize,
                                     kLocalBkgMax * (int)sizeof(double));
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(kern, dim3(a.cap, a.B), dim3(256), (size_t)lds_cap * sizeof(double), s, a,
                     lds_cap);
  return hipGetLastError();
}

hipError_t launch_star_select(const StarSelectArgs& a, hipStream_t s) {
  const dim3 grid((a.cap + 255) / 256, a.B), block(256);
  hipLaunchKernelGGL(k_star_select, grid, block, 0, s, a, 0);
  hipLaunchKernelGGL(k_star_select, grid, block, 0, s, a, 1);
  return hipGetLastError();
}

}  // namespace bsgp
