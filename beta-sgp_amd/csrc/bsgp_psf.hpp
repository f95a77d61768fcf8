// bsgp_psf.hpp — DIAPL PSF model evaluation (host + device), SURVEY §8f row 4.
//
// The reference turns DIAPL PSF coefficient files into 31x31 stamps with
// psf/psf_calculate.py: a sum of ngauss Gaussians, each times a local
// polynomial of degree ldeg in the pixel offsets (calc_psf_pix, :52-87), whose
// coefficients are themselves polynomials of degree sdeg in the field position
// (init_psf, :140-165: the spatial expansion about (x_orig, y_orig)).  The
// stamp is normalised by its numpy sum (normalize_psf_mat, :129-137).
//
// Everything here follows the reference's operation order (no FMA contraction
// in the build), and the normalising sum is numpy's pairwise summation
// (np_pairwise_sum, bsgp_prims.hpp), so a stamp differs from the reference's
// only by the exp() implementation.
#pragma once

#include <cmath>

#include "bsgp_prims.hpp"  // BSGP_HD, np_pairwise_sum

namespace bsgp {

constexpr int kPsfMaxCoef = 384;  // coefficients carried in the kernel arguments
constexpr int kPsfMaxLocal = 128; // ngauss * (ldeg+1)(ldeg+2)/2

struct PsfModel {
  double cosv, sinv, ax, ay;  // rotation and Gaussian widths (file values 5-8)
  double sig2;                // sigma_inc * sigma_inc (psf_calculate.py:87)
  double x_orig, y_orig;      // spatial expansion origin (values 12-13)
  int ngauss, ldeg, sdeg, hw;
  int ncomp;                  // ngauss * (ldeg+1)(ldeg+2)/2 local coefficients
  int ncoef;                  // coefficients supplied
  double coef[kPsfMaxCoef];
};

// The spatial terms of init_psf (:154-165) in its loop order: f(term, a1, a2)
// with a1 = dx^m and a2 = dy^n as its running products form them.  Evaluation
// (psf_local_coef) and fitting (bsgp_psffit.hpp) both go through here.
template <class F>
BSGP_HD void psf_spatial_terms(int sdeg, double dx, double dy, F&& f) {
  int term = 0;
  double a1 = 1.0;
  for (int m = 0; m <= sdeg; ++m) {
    double a2 = 1.0;
    for (int n = 0; n <= sdeg - m; ++n) {
      f(term, a1, a2);
      ++term;
      a2 *= dy;
    }
    a1 *= dx;
  }
}

// Local coefficient icomp at field offset (dx, dy) from the expansion origin:
// sum over spatial terms of coef[term * ncomp + icomp] * dx^m * dy^n.
BSGP_HD double psf_local_coef_at(const double* coef, int ncomp, int sdeg, int icomp, double dx,
                                 double dy) {
  double v = 0.0;
  psf_spatial_terms(sdeg, dx, dy, [&](int term, double a1, double a2) {
    v += coef[term * ncomp + icomp] * a1 * a2;
  });
  return v;
}

// Local coefficient vector at field position (x, y): init_psf (:154-165) —
// local[icomp] = sum over spatial terms (m, n) of coef[itot] * dx^m * dy^n,
// itot running over (term, icomp) with icomp fastest.
BSGP_HD double psf_local_coef(const PsfModel& M, int icomp, double x, double y) {
  return psf_local_coef_at(M.coef, M.ncomp, M.sdeg, icomp, x - M.x_orig, y - M.y_orig);
}

// The terms of calc_psf_pix (:52-87) at pixel offset (x, y) in its loop order:
// f(icomp, e, a1, a2) with e = exp(rr_g), a1 = x^m, a2 = y^n.  Shape is
// anything with cosv, sinv, ax, ay, sig2, ngauss and ldeg (PsfModel, PsfShape).
// The one statement of the basis: evaluation (psf_pix) multiplies a coefficient
// in, fitting (bsgp_psffit.hip) takes phi = e * a1 * a2.
template <class Shape, class F>
BSGP_HD void psf_terms(const Shape& M, double x, double y, F&& f) {
  const double x1 = M.cosv * x - M.sinv * y;
  const double y1 = M.sinv * x + M.cosv * y;
  double rr = M.ax * x1 * x1 + M.ay * y1 * y1;
  int icomp = 0;
  for (int g = 0; g < M.ngauss; ++g) {
    const double e = exp(rr);
    double a1 = 1.0;
    for (int m = 0; m <= M.ldeg; ++m) {
      double a2 = 1.0;
      for (int n = 0; n <= M.ldeg - m; ++n) {
        f(icomp, e, a1, a2);
        ++icomp;
        a2 *= y;
      }
      a1 *= x;
    }
    rr *= M.sig2;
  }
}

// calc_psf_pix (:52-87) at pixel offset (x, y) with local coefficients `loc`.
template <class Coef>
BSGP_HD double psf_pix(const PsfModel& M, const Coef& loc, double x, double y) {
  double pix = 0.0;
  psf_terms(M, x, y, [&](int icomp, double e, double a1, double a2) {
    pix += loc[icomp] * e * a1 * a2;
  });
  return pix;
}

}  // namespace bsgp
