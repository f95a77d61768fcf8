// bsgp_psffit.hip — fitting the DIAPL PSF model to the stars of a frame: what
// the reference leaves to DIAPL's getpsf (psf/psf_estimation.bash with the
// parameters of psf/psf_steps_and_params.MD), for the fixed shape parameters
// of getpsf.par, as one weighted linear least-squares problem per frame
// (include/bsgp.h and DESIGN §3.14, P1 to P8).
//
//  k_psffit_moments<T>  one 256-thread workgroup per (star, frame); the only
//                 pass over pixels.  The box is walked in row-major order in
//                 chunks of C candidates (C = 256, 128 or 64 by ncomp); a
//                 workgroup scan numbers the fit pixels of a chunk in that
//                 order and each writes z = (phi_0 .. phi_{ncomp-1}, v) to
//                 LDS, phi through psf_terms (bsgp_psf.hpp), the function
//                 psf_pix evaluates with.  Every lane owns up to kFitQ fixed
//                 entries (i, j) of the packed upper triangle of sum z z^T
//                 (G, then h as the column j = ncomp, then vv) in registers
//                 and adds z_i z_j over the staged pixels in order: the sums
//                 run in pixel order whatever C and the lane count are.  With
//                 no flux given, a first walk adds I - sky in the same order
//                 (one lane) and the second divides by it; the box then comes
//                 from the cache.
//  k_psffit_solve  one 256-thread workgroup per frame, everything in LDS:
//                 N = sum w (S S^T) (x) G and b = sum w S (x) h over the
//                 active stars in index order (one lane per entry), diagonal
//                 scaling, Cholesky, two triangular solves (bsgp_psffit.hpp),
//                 per-star rss and rms from the moments, and the clipping
//                 rounds: rms of the active stars sorted in LDS (bkg_sort) for
//                 the two medians, the rule applied, the fit repeated.
#include <hip/hip_runtime.h>

#include "bsgp_apps.hpp"
#include "bsgp_prims.hpp"
#include "bsgp_psffit.hpp"
#include "bsgp_sigclip.hpp"  // bkg_sort

#pragma clang fp contract(off)

namespace bsgp {

constexpr int kFitQ = 24;  // entries of sum z z^T one lane owns
static_assert((kPsfFitMaxCoef + 1) * (kPsfFitMaxCoef + 2) / 2 <= kFitQ * 256,
              "every entry of the moments has a lane");
constexpr int kFitLimit = 1 << 30;  // |box centre|: centre +- hw stays an int

namespace {

__device__ __forceinline__ int fit_centre(double pos) {
  double e = floor(pos + 0.5);
  const double lim = (double)kFitLimit;
  e = e < -lim ? -lim : (e > lim ? lim : e);
  return (int)e;
}

// entry e of the packed upper triangle of the (n + 1)-square sum z z^T, in the
// order G (rows of the n-square triangle), h, vv -> i | j << 8
__device__ __forceinline__ int fit_entry(int e, int n) {
  const int T = n * (n + 1) / 2;
  if (e >= T + n + 1) return 0;  // no entry: a product nobody stores
  if (e == T + n) return n | (n << 8);
  if (e >= T) return (e - T) | (n << 8);
  int i = 0;
  while (psffit_upper(n, i + 1, i + 1) <= e) ++i;
  return i | ((i + (e - psffit_upper(n, i, i))) << 8);
}

}  // namespace

template <typename T>
__global__ void __launch_bounds__(256) k_psffit_moments(PsfFitMomentArgs a) {
  extern __shared__ double s[];  // C rows of z, ncomp + 1 values each
  __shared__ int wsum[4];
  __shared__ double s_flux;
  const int tid = threadIdx.x, star = blockIdx.x, b = blockIdx.y;
  int nr = a.n ? a.n[b] : a.cap;
  nr = nr < a.cap ? nr : a.cap;
  if (star >= nr) return;
  const size_t rr = (size_t)b * a.cap + star;
  const PsfShape& M = a.shape;
  const int nc = M.ncomp, st = nc + 1, hw = M.hw;
  const double px = a.xy[2 * rr], py = a.xy[2 * rr + 1];

  // P1: the box and its status (uniform over the workgroup)
  int status = 0, ic = 0, ir = 0;
  if (!(__builtin_isfinite(px) && __builtin_isfinite(py))) {
    status = BSGP_PSFFIT_BAD_POSITION;
  } else {
    ic = fit_centre(px), ir = fit_centre(py);
    if (ic + hw < 0 || ic - hw >= a.W || ir + hw < 0 || ir - hw >= a.H)
      status = BSGP_PSFFIT_NO_OVERLAP;
    else if (ic - hw < 0 || ic + hw >= a.W || ir - hw < 0 || ir + hw >= a.H)
      status = BSGP_PSFFIT_PARTIAL;
  }
  double F = a.flux ? a.flux[rr] : 1.0;
  if (!(status & BSGP_PSFFIT_EXCLUDED) && a.flux && !(F > 0.0 && __builtin_isfinite(F)))
    status |= BSGP_PSFFIT_BAD_FLUX;
  if (status & BSGP_PSFFIT_EXCLUDED) {
    if (tid == 0) a.status[rr] = status, a.flux_out[rr] = a.flux ? F : dev_nan();
    return;
  }

  const size_t img_off = (size_t)b * a.H * a.W;
  const T* img = static_cast<const T*>(a.img) + img_off;
  const unsigned char* mask = a.mask ? a.mask + img_off : nullptr;
  const double star_sky = a.sky_mode == 1 ? a.sky[rr] : 0.0;
  const double* skymap = a.sky_mode == 2 ? a.sky + img_off : nullptr;
  const int S = 2 * hw + 1, S2 = S * S, C = a.chunk;

  int ij[kFitQ];
  double acc[kFitQ];
  const int nq = ((nc + 1) * (nc + 2) / 2 + 255) >> 8;  // <= kFitQ (checked on the host)
#pragma unroll
  for (int q = 0; q < kFitQ; ++q) {
    ij[q] = q < nq ? fit_entry(q * 256 + tid, nc) : 0;
    acc[q] = 0.0;
  }

  int npix = 0;
  // walk 0 (only without a given flux): F = sum of I - sky; walk 1: the moments
  for (int walk = a.flux ? 1 : 0; walk < 2; ++walk) {
    npix = 0;
    if (walk == 0 && tid == 0) s_flux = 0.0;
    for (int base = 0; base < S2; base += C) {
      const int p = base + tid;
      bool ok = false;
      double d = 0.0, x = 0.0, y = 0.0;
      if (tid < C && p < S2) {
        const int r = ir - hw + p / S, c = ic - hw + p % S;
        if (r >= 0 && r < a.H && c >= 0 && c < a.W) {
          x = (double)c - px, y = (double)r - py;
          if (x * x + y * y <= a.fitrad2) {
            const size_t o = (size_t)r * a.W + c;
            const double I = (double)img[o];
            d = I - (skymap ? skymap[o] : star_sky);
            ok = __builtin_isfinite(d) && !(mask && mask[o]) && !(a.has_sat && I >= a.sat_level);
          }
        }
      }
      int cnt;
      const int pos = block_scan(ok ? 1 : 0, wsum, &cnt);
      if (ok) {
        if (walk == 0) {
          s[pos] = d;
        } else {
          double* z = s + pos * st;
          psf_terms(M, x, y, [&](int k, double e, double a1, double a2) { z[k] = e * a1 * a2; });
          z[nc] = d / F;
        }
      }
      __syncthreads();
      if (walk == 0) {
        if (tid == 0) {
          double f = s_flux;
          for (int q = 0; q < cnt; ++q) f += s[q];
          s_flux = f;
        }
      } else {
        for (int q = 0; q < cnt; ++q) {
          const double* z = s + q * st;
#pragma unroll
          for (int k = 0; k < kFitQ; ++k)
            if (k < nq) acc[k] += z[ij[k] & 0xff] * z[ij[k] >> 8];
        }
      }
      npix += cnt;
      __syncthreads();
    }
    if (walk == 0) {
      F = s_flux;  // published by the loop's last barrier (S2 >= 1)
      if (!(F > 0.0 && __builtin_isfinite(F)) || npix < nc) break;
    }
  }

  if (!(F > 0.0 && __builtin_isfinite(F)))
    status |= BSGP_PSFFIT_BAD_FLUX;
  else if (npix < nc)
    status |= BSGP_PSFFIT_FEW_PIXELS;
  if (tid == 0) a.status[rr] = status, a.flux_out[rr] = F, a.npix[rr] = npix;
  if (status & BSGP_PSFFIT_EXCLUDED) return;  // the moments stay 0
  const int Tn = nc * (nc + 1) / 2;
  double* G = a.G + rr * Tn;
  double* h = a.h + rr * nc;
#pragma unroll
  for (int k = 0; k < kFitQ; ++k) {
    const int e = k * 256 + tid;
    if (k < nq && e <= Tn + nc) {
      if (e < Tn)
        G[e] = acc[k];
      else if (e < Tn + nc)
        h[e - Tn] = acc[k];
      else
        a.vv[rr] = acc[k];
    }
  }
}

// ---------------------------------------------------------------- the solve
namespace {

// S_t(dx, dy): spatial term t in psf_spatial_terms' order
__device__ __forceinline__ double fit_spatial(int sdeg, int t, double dx, double dy) {
  double v = 0.0;
  psf_spatial_terms(sdeg, dx, dy, [&](int term, double a1, double a2) {
    if (term == t) v = a1 * a2;
  });
  return v;
}

}  // namespace

__global__ void __launch_bounds__(256) k_psffit_solve(PsfFitSolveArgs a) {
  extern __shared__ double lds[];
  __shared__ int s_cnt[2];  // active stars, stars a round would drop
  const int tid = threadIdx.x, b = blockIdx.x;
  const PsfShape& M = a.shape;
  const int nc = M.ncomp, nt = M.nterm, P = nc * nt, Tn = nc * (nc + 1) / 2;
  double* A = lds;                        // P (P + 1) / 2: N, scaled, then its factor
  double* x = A + P * (P + 1) / 2;        // P: b, then the solution
  double* dsc = x + P;                    // P: sqrt(N_ii)
  double* srt = dsc + P;                  // a.sortP: rms of the active stars
  unsigned char* act = reinterpret_cast<unsigned char*>(srt + a.sortP);  // cap
  unsigned char* sig = act + a.cap;                                      // cap
  int nr = a.n ? a.n[b] : a.cap;
  nr = nr < a.cap ? nr : a.cap;
  nr = nr < 0 ? 0 : nr;
  const size_t r0 = (size_t)b * a.cap;
  const double* xy = a.xy + 2 * r0;
  auto sync = [] { __syncthreads(); };

  // P4: the active stars
  for (int sidx = tid; sidx < a.cap; sidx += 256) {
    int stt = 0, on = 0;
    if (sidx < nr) {
      stt = a.mstatus[r0 + sidx];
      const double w = a.weights ? a.weights[r0 + sidx] : 1.0;
      if (!(stt & BSGP_PSFFIT_EXCLUDED) && !(w > 0.0 && __builtin_isfinite(w)))
        stt |= BSGP_PSFFIT_BAD_WEIGHT;
      on = !(stt & BSGP_PSFFIT_EXCLUDED);
      a.status[r0 + sidx] = stt;
      a.rms[r0 + sidx] = dev_nan();
    }
    act[sidx] = (unsigned char)on;
    sig[sidx] = 0;
  }
  __syncthreads();

  int rounds = 0, fstatus = 0;
  for (;;) {
    // P4: N and b over the active stars in index order, one lane per entry
    for (int e = tid; e < P * (P + 1) / 2 + P; e += 256) {
      const bool rhs = e >= P * (P + 1) / 2;
      int I = 0, J = 0;
      if (rhs) {
        I = e - P * (P + 1) / 2;
      } else {
        while (psffit_lower(I + 1, 0) <= e) ++I;
        J = e - psffit_lower(I, 0);
      }
      const int t = I / nc, k = I % nc, u = J / nc, l = J % nc;
      double sum = 0.0;
      for (int sidx = 0; sidx < nr; ++sidx) {
        if (!act[sidx]) continue;
        const double w = a.weights ? a.weights[r0 + sidx] : 1.0;
        const double dx = xy[2 * sidx] - M.x_orig, dy = xy[2 * sidx + 1] - M.y_orig;
        const double St = fit_spatial(M.sdeg, t, dx, dy);
        if (rhs)
          sum += w * St * a.h[(r0 + sidx) * nc + k];
        else
          sum += w * (St * fit_spatial(M.sdeg, u, dx, dy)) *
                 psffit_sym(a.G + (r0 + sidx) * Tn, nc, k, l);
      }
      if (rhs) x[I] = sum; else A[e] = sum;
    }
    __syncthreads();

    // P5, P6
    psffit_scale(A, dsc, P, tid, 256, sync);
    const bool ok = psffit_cholesky(A, P, tid, 256, sync);
    if (!ok) {
      fstatus |= BSGP_PSFFIT_SINGULAR;
      break;
    }
    for (int i = tid; i < P; i += 256) x[i] = x[i] / dsc[i];
    __syncthreads();
    psffit_solve(A, x, P, tid, 256, sync);
    for (int i = tid; i < P; i += 256) x[i] = x[i] / dsc[i];
    if (tid < 2) s_cnt[tid] = 0;
    __syncthreads();

    // P7: rss and rms of every active star, its rms into the sort's array
    for (int sidx = tid; sidx < a.sortP; sidx += 256) {
      double key = dev_inf();
      if (sidx < nr && act[sidx]) {
        const size_t rr = r0 + sidx;
        const double vv = a.vv[rr];
        const double rss = psffit_rss(x, nc, M.sdeg, xy[2 * sidx] - M.x_orig,
                                      xy[2 * sidx + 1] - M.y_orig, a.G + rr * Tn, a.h + rr * nc, vv);
        key = sqrt(rss / (double)a.npix[rr]);
        a.rms[rr] = key;
        sig[sidx] = psffit_rss_significant(rss, vv) ? 1 : 0;
        atomicAdd(&s_cnt[0], 1);
      }
      srt[sidx] = key;
    }
    __syncthreads();
    const int nact = s_cnt[0];
    if (rounds >= a.niter || nact < 1) break;

    // P8: the two medians, then the rule
    bkg_sort(srt, a.sortP);
    if (a.sortP < 2) __syncthreads();
    const double med = psffit_median_sorted(srt, nact);
    __syncthreads();
    for (int sidx = tid; sidx < a.sortP; sidx += 256) {
      double key = dev_inf();
      if (sidx < nr && act[sidx]) key = fabs(a.rms[r0 + sidx] - med);
      srt[sidx] = key;
    }
    __syncthreads();
    bkg_sort(srt, a.sortP);
    if (a.sortP < 2) __syncthreads();
    const double thr = psffit_clip_threshold(med, psffit_median_sorted(srt, nact), a.nsig);
    int ndrop = 0;
    for (int sidx = tid; sidx < nr; sidx += 256)
      if (act[sidx] && sig[sidx] && a.rms[r0 + sidx] > thr) ++ndrop;
    if (ndrop) atomicAdd(&s_cnt[1], ndrop);
    __syncthreads();
    if (!psffit_round_applies(nact, s_cnt[1], nt, a.min_stars)) break;
    for (int sidx = tid; sidx < nr; sidx += 256)
      if (act[sidx] && sig[sidx] && a.rms[r0 + sidx] > thr) {
        act[sidx] = 0;
        a.status[r0 + sidx] |= BSGP_PSFFIT_CLIPPED;
      }
    ++rounds;
    __syncthreads();
  }

  // outputs
  __syncthreads();
  if (tid < 2) s_cnt[tid] = 0;
  __syncthreads();
  int mine = 0;
  for (int sidx = tid; sidx < a.cap; sidx += 256) {
    const int on = sidx < nr && act[sidx];
    a.used[r0 + sidx] = on;
    if (sidx < nr && (fstatus & BSGP_PSFFIT_SINGULAR)) a.rms[r0 + sidx] = dev_nan();
    mine += on;
  }
  if (mine) atomicAdd(&s_cnt[0], mine);
  for (int i = tid; i < P; i += 256)
    a.coef[(size_t)b * P + i] = (fstatus & BSGP_PSFFIT_SINGULAR) ? dev_nan() : x[i];
  __syncthreads();
  if (tid == 0) {
    a.frame[3 * b] = fstatus;
    a.frame[3 * b + 1] = rounds;
    a.frame[3 * b + 2] = s_cnt[0];
  }
}

int psffit_chunk(int ncomp) { return ncomp + 1 <= 24 ? 256 : (ncomp + 1 <= 48 ? 128 : 64); }

hipError_t launch_psffit_moments(PsfFitMomentArgs a, int f32, hipStream_t s) {
  a.chunk = psffit_chunk(a.shape.ncomp);
  const size_t lds = (size_t)a.chunk * (a.shape.ncomp + 1) * sizeof(double);  // <= 55808
  hipLaunchKernelGGL(f32 ? k_psffit_moments<float> : k_psffit_moments<double>, dim3(a.cap, a.B),
                     dim3(256), lds, s, a);
  return hipGetLastError();
}

size_t psffit_solve_lds(int P, int sortP, int cap) {
  return ((size_t)P * (P + 1) / 2 + 2 * (size_t)P + sortP) * sizeof(double) + 2 * (size_t)cap;
}

hipError_t launch_psffit_solve(PsfFitSolveArgs a, hipStream_t s) {
  a.sortP = 1;
  while (a.sortP < a.cap) a.sortP <<= 1;
  const int P = a.shape.ncomp * a.shape.nterm;
  hipError_t e = hipFuncSetAttribute(
      reinterpret_cast<const void*>(k_psffit_solve), hipFuncAttributeMaxDynamicSharedMemorySize,
      (int)psffit_solve_lds(kPsfFitMaxCoef, kPsfFitMaxStars, kPsfFitMaxStars));
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_psffit_solve, dim3(a.B), dim3(256), psffit_solve_lds(P, a.sortP, a.cap), s,
                     a);
  return hipGetLastError();
}

}  // namespace bsgp
