// bsgp_psffit.hpp — the pieces of the DIAPL PSF fit (bsgp_psffit.hip, DESIGN
// §3.14, P1 to P8) that compile on the host as well: the shape header the
// kernels carry, the packed index rules, the scaled Cholesky with its two
// triangular solves, the residual from the moments and the clipping rule
// (tests/cpp/psffit_test.cpp).
//
// The linear algebra is written once for a team of nt workers, worker `tid`
// calling with a `sync` that is __syncthreads() on the device and a no-op for
// the host's team of one.  Every entry is updated by one worker in an order
// that does not depend on nt, so the host program and the 256-thread
// workgroup compute the same bits.
#pragma once

#include <cmath>

#include "bsgp_prims.hpp"
#include "bsgp_psf.hpp"  // psf_terms, psf_spatial_terms, psf_local_coef_at

namespace bsgp {

// What a fit knows of the model: everything of PsfModel but the coefficients.
struct PsfShape {
  double cosv, sinv, ax, ay;
  double sig2;            // sigma_inc * sigma_inc
  double x_orig, y_orig;  // origin of the spatial expansion
  int ngauss, ldeg, sdeg, hw;
  int ncomp;  // ngauss * (ldeg+1)(ldeg+2)/2
  int nterm;  // (sdeg+1)(sdeg+2)/2
};

// G_s, packed upper triangle in row-major order: (i, j), i <= j < n
BSGP_HD int psffit_upper(int n, int i, int j) { return i * n - i * (i - 1) / 2 + (j - i); }
BSGP_HD double psffit_sym(const double* G, int n, int i, int j) {
  return i <= j ? G[psffit_upper(n, i, j)] : G[psffit_upper(n, j, i)];
}
// the normal matrix and its factor, packed lower triangle in row-major order: (i, j), j <= i
BSGP_HD int psffit_lower(int i, int j) { return i * (i + 1) / 2 + j; }

// the smallest scaled pivot the factorisation accepts is above P * 2^-52 (P6)
BSGP_HD double psffit_pivot_floor(int P) { return (double)P * 2.220446049250313e-16; }

// P5: A_ij = N_ij / sqrt(N_ii N_jj) in place, d_i = sqrt(N_ii).  A diagonal
// that is not a positive finite number leaves NaNs that the factorisation's
// pivot test reports.
template <class Sync>
BSGP_HD void psffit_scale(double* A, double* d, int P, int tid, int nt, Sync&& sync) {
  for (int i = tid; i < P; i += nt) d[i] = A[psffit_lower(i, i)];
  sync();
  for (int i = tid; i < P; i += nt)
    for (int j = 0; j <= i; ++j) A[psffit_lower(i, j)] = A[psffit_lower(i, j)] / sqrt(d[i] * d[j]);
  sync();
  for (int i = tid; i < P; i += nt) d[i] = sqrt(d[i]);
  sync();
}

// P6: Cholesky factor L (A = L L^T) over the packed lower triangle, in place,
// column by column; entry (i, k) loses L_ij * L_kj for j = 0 .. k - 1 in that
// order.  False, in every worker, at the first pivot that is not a finite
// number above psffit_pivot_floor(P).
template <class Sync>
BSGP_HD bool psffit_cholesky(double* A, int P, int tid, int nt, Sync&& sync) {
  const double floor_ = psffit_pivot_floor(P);
  const int lpr = nt >= 4 ? 4 : 1;  // workers per row of the trailing update
  const int row0 = tid / lpr, col0 = tid % lpr, rows = nt / lpr;
  for (int j = 0; j < P; ++j) {
    const double piv = A[psffit_lower(j, j)];
    if (!(piv > floor_) || !(piv < HUGE_VAL)) return false;
    const double r = sqrt(piv);
    sync();  // every worker has read the pivot
    for (int i = j + tid; i < P; i += nt)
      A[psffit_lower(i, j)] = i == j ? r : A[psffit_lower(i, j)] / r;
    sync();
    for (int i = j + 1 + row0; i < P; i += rows) {
      const double lij = A[psffit_lower(i, j)];
      for (int k = j + 1 + col0; k <= i; k += lpr)
        A[psffit_lower(i, k)] = A[psffit_lower(i, k)] - lij * A[psffit_lower(k, j)];
    }
    sync();
  }
  return true;
}

// P6: x <- the solution of (L L^T) z = x, by columns: forward with k
// ascending, backward with k descending; entry i loses L_ik * x_k one k at a time.
template <class Sync>
BSGP_HD void psffit_solve(const double* L, double* x, int P, int tid, int nt, Sync&& sync) {
  for (int k = 0; k < P; ++k) {
    if (tid == 0) x[k] = x[k] / L[psffit_lower(k, k)];
    sync();
    const double xk = x[k];
    for (int i = k + 1 + tid; i < P; i += nt) x[i] = x[i] - L[psffit_lower(i, k)] * xk;
    sync();
  }
  for (int k = P - 1; k >= 0; --k) {
    if (tid == 0) x[k] = x[k] / L[psffit_lower(k, k)];
    sync();
    const double xk = x[k];
    for (int i = tid; i < k; i += nt) x[i] = x[i] - L[psffit_lower(k, i)] * xk;
    sync();
  }
}

// P7: a star's residual sum of squares from its moments and the coefficients:
// max(0, (vv - 2 c.h) + c.(G c)) with c the local coefficients at the star's
// offset (dx, dy) from the origin, every sum in index order.
BSGP_HD double psffit_rss(const double* coef, int ncomp, int sdeg, double dx, double dy,
                          const double* G, const double* h, double vv) {
  double ch = 0.0, cgc = 0.0;
  for (int i = 0; i < ncomp; ++i) {
    const double ci = psf_local_coef_at(coef, ncomp, sdeg, i, dx, dy);
    double gc = 0.0;
    for (int j = 0; j < ncomp; ++j)
      gc += psffit_sym(G, ncomp, i, j) * psf_local_coef_at(coef, ncomp, sdeg, j, dx, dy);
    ch += ci * h[i];
    cgc += ci * gc;
  }
  const double rss = (vv - 2.0 * ch) + cgc;
  return rss > 0.0 ? rss : 0.0;  // a NaN becomes 0 only with NaN coefficients, which are not evaluated
}

// numpy's median of m >= 1 sorted values
BSGP_HD double psffit_median_sorted(const double* s, int m) {
  return (m & 1) ? s[m / 2] : (s[m / 2 - 1] + s[m / 2]) / 2.0;
}

// P8: the clipping rule.  A star goes when its rms is above the threshold and
// its rss is more than the rounding noise of the cancellation that formed it.
BSGP_HD double psffit_clip_threshold(double med, double mad, double nsig) {
  return med + nsig * 1.4826 * mad;
}
BSGP_HD bool psffit_rss_significant(double rss, double vv) {
  return rss > 4096.0 * 2.220446049250313e-16 * vv;
}
BSGP_HD bool psffit_drop(double rms, double thr, double rss, double vv) {
  return rms > thr && psffit_rss_significant(rss, vv);
}
// a round that drops ndrop of nactive stars is applied when it drops any and
// leaves at least max(nterm, min_stars)
BSGP_HD bool psffit_round_applies(int nactive, int ndrop, int nterm, int min_stars) {
  const int need = nterm > min_stars ? nterm : min_stars;
  return ndrop > 0 && nactive - ndrop >= need;
}

}  // namespace bsgp
