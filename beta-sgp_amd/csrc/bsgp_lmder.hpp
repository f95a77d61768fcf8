// bsgp_lmder.hpp — MINPACK's lmder for the three-parameter Gaussian1D fit of
// a radial profile: what scipy.optimize.leastsq runs when
// astropy's LevMarLSQFitter fits the reference's model (restoration/utils.py:
// 180-202).  A port of the published algorithm (More, Garbow, Hillstrom,
// "User Guide for MINPACK-1", ANL-80-74): lmder, qrfac with column pivoting,
// lmpar, qrsolv and enorm, with the same tests, the same updates of delta and
// par, the same counting of function evaluations and the same exit codes.
//
// One team of LM_NL lanes runs one fit.  The m-vectors (residuals, Jacobian
// columns) are shared arrays that the lanes walk with stride LM_NL; sums and
// maxima over them go through LM_SUM / LM_MAX, which return the same bits to
// every lane.  Everything of size 3 or 3 x 3 is computed by every lane alike
// from shared arrays, so that no lane holds an array it indexes dynamically.
// The includer defines, before including this header:
//   LM_FN      function qualifiers      LM_LANE   this lane's index
//   LM_NL      lanes of a team          LM_SYNC() make the team's writes visible
//   LM_SUM(v) / LM_MAX(v)  team sum / maximum of v
// A device build sets them to a wave's; a host build to one lane (tests/cpp).
#pragma once
#include <math.h>

namespace bsgp_lm {

constexpr int kN = 3;                            // parameters: amplitude, mean, stddev
constexpr double kTiny32 = 1.1754943508222875e-38;  // the model's lower bound of stddev
constexpr double kEpsMch = 2.220446049250313e-16;   // dpmpar(1)
constexpr double kDwarf = 2.2250738585072014e-308;  // dpmpar(2)
constexpr double kRdwarf = 3.834e-20, kRgiant = 1.304e19;
constexpr double kFwhmPerSigma = 2.3548200450309493;  // 2 sqrt(2 ln 2)

// shared arrays of one fit
struct Work {
  double* y;     // [m] the profile
  double* fvec;  // [m]
  double* wa4;   // [m]
  double* fjac;  // [3][ld]: column j at fjac + j * ld
  int ld;
  // [3] each; wa1 .. wa3 as in lmder, sdiag / xs / wq are lmpar's sdiag, wa1, wa2
  double *x, *diag, *qtf, *wa1, *wa2, *wa3, *sdiag, *xs, *wq;
  int* ipvt;                                                    // [3]
};
constexpr int kSmallDoubles = 9 * kN;

// enorm of a[i0 .. m): the three scaled accumulators of MINPACK's enorm, each
// summed over the team (the scales are the maxima, taken first)
LM_FN double enorm_team(const double* a, int i0, int m) {
  const double agiant = kRgiant / (double)(m - i0);
  double s2 = 0.0, x1max = 0.0, x3max = 0.0;
  for (int i = i0 + LM_LANE; i < m; i += LM_NL) {
    const double xabs = fabs(a[i]);
    if (xabs > kRdwarf && xabs < agiant) s2 += xabs * xabs;
    else if (xabs <= kRdwarf) x3max = xabs > x3max ? xabs : x3max;
    else x1max = (xabs > x1max || xabs != xabs) ? xabs : x1max;
  }
  s2 = LM_SUM(s2);
  x1max = LM_MAX(x1max);
  x3max = LM_MAX(x3max);
  if (x1max == 0.0 && x3max == 0.0) return sqrt(s2);
  double s1 = 0.0, s3 = 0.0;
  for (int i = i0 + LM_LANE; i < m; i += LM_NL) {
    const double xabs = fabs(a[i]);
    if (xabs > kRdwarf && xabs < agiant) continue;
    if (xabs <= kRdwarf) {
      if (xabs != 0.0) { const double t = xabs / x3max; s3 += t * t; }
    } else {
      // (one infinite value counts 1, as where MINPACK rescales by it; two give
      // its inf / inf)
      const double t = xabs == x1max ? 1.0 : xabs / x1max;
      s1 += t * t;
    }
  }
  s1 = LM_SUM(s1);
  s3 = LM_SUM(s3);
  if (x1max > 1.79769313486231570815e308 && s1 > 1.0) return NAN;
  if (s1 != 0.0) return x1max * sqrt(s1 + (s2 / x1max) / x1max);
  if (s2 != 0.0) {
    if (s2 >= x3max) return sqrt(s2 * (1.0 + (x3max / s2) * (x3max * s3)));
    return sqrt(x3max * ((s2 / x3max) + (x3max * s3)));
  }
  return x3max * sqrt(s3);
}

// enorm of three values, in MINPACK's own order
LM_FN double enorm3(const double* v) {
  const double agiant = kRgiant / 3.0;
  double s1 = 0.0, s2 = 0.0, s3 = 0.0, x1max = 0.0, x3max = 0.0;
  for (int i = 0; i < kN; ++i) {
    const double xabs = fabs(v[i]);
    if (xabs > kRdwarf && xabs < agiant) {
      s2 += xabs * xabs;
    } else if (xabs <= kRdwarf) {
      if (xabs > x3max) {
        const double t = x3max / xabs;
        s3 = 1.0 + s3 * (t * t);
        x3max = xabs;
      } else if (xabs != 0.0) {
        const double t = xabs / x3max;
        s3 += t * t;
      }
    } else if (xabs > x1max) {
      const double t = x1max / xabs;
      s1 = 1.0 + s1 * (t * t);
      x1max = xabs;
    } else {
      const double t = xabs / x1max;
      s1 += t * t;
    }
  }
  if (s1 != 0.0) return x1max * sqrt(s1 + (s2 / x1max) / x1max);
  if (s2 != 0.0) {
    if (s2 >= x3max) return sqrt(s2 * (1.0 + (x3max / s2) * (x3max * s3)));
    return sqrt(x3max * ((s2 / x3max) + (x3max * s3)));
  }
  return x3max * sqrt(s3);
}

// residuals model(p) - y, with stddev clipped below as the fitter applies the
// model's bound (fmax: a NaN becomes the bound)
LM_FN void residuals(const Work& w, int m, const double* p, double* out) {
  const double a = p[0], mu = p[1];
  const double s = p[2] >= kTiny32 ? p[2] : kTiny32;
  const double ss = s * s;
  for (int i = LM_LANE; i < m; i += LM_NL) {
    const double d = (double)i - mu;
    out[i] = a * exp((-0.5 * (d * d)) / ss) - w.y[i];
  }
  LM_SYNC();
}

// the analytic Jacobian at p, stddev as it is (not clipped)
LM_FN void jacobian(const Work& w, int m, const double* p) {
  const double a = p[0], mu = p[1], s = p[2];
  const double ss = s * s, sss = ss * s;
  for (int i = LM_LANE; i < m; i += LM_NL) {
    const double d = (double)i - mu;
    const double e = exp((-0.5 * (d * d)) / ss);
    const double ae = a * e;
    w.fjac[i] = e;
    w.fjac[w.ld + i] = (ae * d) / ss;
    w.fjac[2 * w.ld + i] = (ae * (d * d)) / sss;
  }
  LM_SYNC();
}

// qrfac(m, 3, fjac, pivot = true): rdiag, acnorm, wa as in MINPACK
LM_FN void qrfac(const Work& w, int m, double* rdiag, double* acnorm, double* wa) {
  double* a = w.fjac;
  const int ld = w.ld;
  for (int j = 0; j < kN; ++j) {
    const double c = enorm_team(a + j * ld, 0, m);
    acnorm[j] = c;
    rdiag[j] = c;
    wa[j] = c;
    w.ipvt[j] = j;
  }
  LM_SYNC();
  for (int j = 0; j < kN; ++j) {
    int kmax = j;
    for (int k = j; k < kN; ++k)
      if (rdiag[k] > rdiag[kmax]) kmax = k;
    if (kmax != j) {
      for (int i = LM_LANE; i < m; i += LM_NL) {
        const double t = a[j * ld + i];
        a[j * ld + i] = a[kmax * ld + i];
        a[kmax * ld + i] = t;
      }
      LM_SYNC();
      rdiag[kmax] = rdiag[j];
      wa[kmax] = wa[j];
      const int k = w.ipvt[j];
      w.ipvt[j] = w.ipvt[kmax];
      w.ipvt[kmax] = k;
      LM_SYNC();
    }
    double ajnorm = enorm_team(a + j * ld, j, m);
    if (ajnorm != 0.0) {
      if (a[j * ld + j] < 0.0) ajnorm = -ajnorm;
      LM_SYNC();
      for (int i = j + LM_LANE; i < m; i += LM_NL) {
        double v = a[j * ld + i] / ajnorm;
        if (i == j) v += 1.0;
        a[j * ld + i] = v;
      }
      LM_SYNC();
      for (int k = j + 1; k < kN; ++k) {
        double sum = 0.0;
        for (int i = j + LM_LANE; i < m; i += LM_NL) sum += a[j * ld + i] * a[k * ld + i];
        sum = LM_SUM(sum);
        const double temp = sum / a[j * ld + j];
        for (int i = j + LM_LANE; i < m; i += LM_NL) a[k * ld + i] -= temp * a[j * ld + i];
        LM_SYNC();
        if (rdiag[k] != 0.0) {
          const double t = a[k * ld + j] / rdiag[k];
          const double u = 1.0 - t * t;
          const double r = rdiag[k] * sqrt(u > 0.0 ? u : 0.0);
          const double q = r / wa[k];
          LM_SYNC();
          rdiag[k] = r;
          if (!(0.05 * (q * q) > kEpsMch)) {
            const double e = enorm_team(a + k * ld, j + 1, m);
            rdiag[k] = e;
            wa[k] = e;
          }
          LM_SYNC();
        }
      }
    }
    rdiag[j] = -ajnorm;
    LM_SYNC();
  }
}

// r(i, j) of the 3 x 3 triangle kept in the first rows of fjac
#define LM_R(i, j) r[(j) * ld + (i)]

LM_FN void qrsolv(double* r, int ld, const int* ipvt, const double* diag, const double* qtb,
                  double* x, double* sdiag, double* wa) {
  for (int j = 0; j < kN; ++j) {
    for (int i = j; i < kN; ++i) LM_R(i, j) = LM_R(j, i);
    x[j] = LM_R(j, j);
    wa[j] = qtb[j];
  }
  LM_SYNC();
  for (int j = 0; j < kN; ++j) {
    const int l = ipvt[j];
    if (diag[l] != 0.0) {
      for (int k = j; k < kN; ++k) sdiag[k] = 0.0;
      sdiag[j] = diag[l];
      LM_SYNC();
      double qtbpj = 0.0;
      for (int k = j; k < kN; ++k) {
        if (sdiag[k] == 0.0) continue;
        double sn, cs;
        if (fabs(LM_R(k, k)) < fabs(sdiag[k])) {
          const double cotan = LM_R(k, k) / sdiag[k];
          sn = 0.5 / sqrt(0.25 + 0.25 * (cotan * cotan));
          cs = sn * cotan;
        } else {
          const double tn = sdiag[k] / LM_R(k, k);
          cs = 0.5 / sqrt(0.25 + 0.25 * (tn * tn));
          sn = cs * tn;
        }
        const double rkk = cs * LM_R(k, k) + sn * sdiag[k];
        const double temp = cs * wa[k] + sn * qtbpj;
        qtbpj = -sn * wa[k] + cs * qtbpj;
        LM_SYNC();
        LM_R(k, k) = rkk;
        wa[k] = temp;
        for (int i = k + 1; i < kN; ++i) {
          const double t = cs * LM_R(i, k) + sn * sdiag[i];
          const double sd = -sn * LM_R(i, k) + cs * sdiag[i];
          LM_SYNC();
          sdiag[i] = sd;
          LM_R(i, k) = t;
        }
        LM_SYNC();
      }
    }
    const double rjj = LM_R(j, j);
    LM_SYNC();
    sdiag[j] = rjj;
    LM_R(j, j) = x[j];
    LM_SYNC();
  }
  int nsing = kN;
  for (int j = 0; j < kN; ++j) {
    if (sdiag[j] == 0.0 && nsing == kN) nsing = j;
    if (nsing < kN) wa[j] = 0.0;
  }
  LM_SYNC();
  for (int k = 1; k <= nsing; ++k) {
    const int j = nsing - k;
    double sum = 0.0;
    for (int i = j + 1; i < nsing; ++i) sum += LM_R(i, j) * wa[i];
    const double v = (wa[j] - sum) / sdiag[j];
    LM_SYNC();
    wa[j] = v;
    LM_SYNC();
  }
  for (int j = 0; j < kN; ++j) x[ipvt[j]] = wa[j];
  LM_SYNC();
}

// lmpar: x = the step, sdiag, par updated; wa1, wa2 work
LM_FN double lmpar(double* r, int ld, const int* ipvt, const double* diag, const double* qtb,
                   double delta, double par, double* x, double* sdiag, double* wa1, double* wa2) {
  int nsing = kN;
  for (int j = 0; j < kN; ++j) {
    wa1[j] = qtb[j];
    if (LM_R(j, j) == 0.0 && nsing == kN) nsing = j;
    if (nsing < kN) wa1[j] = 0.0;
  }
  LM_SYNC();
  for (int k = 1; k <= nsing; ++k) {
    const int j = nsing - k;
    const double temp = wa1[j] / LM_R(j, j);
    LM_SYNC();
    wa1[j] = temp;
    for (int i = 0; i < j; ++i) {
      const double v = wa1[i] - LM_R(i, j) * temp;
      LM_SYNC();
      wa1[i] = v;
    }
    LM_SYNC();
  }
  for (int j = 0; j < kN; ++j) x[ipvt[j]] = wa1[j];
  LM_SYNC();
  int iter = 0;
  for (int j = 0; j < kN; ++j) wa2[j] = diag[j] * x[j];
  LM_SYNC();
  double dxnorm = enorm3(wa2);
  double fp = dxnorm - delta;
  if (fp <= 0.1 * delta) return 0.0;  // (iter == 0: par = 0)
  double parl = 0.0;
  if (nsing >= kN) {
    for (int j = 0; j < kN; ++j) {
      const int l = ipvt[j];
      wa1[j] = diag[l] * (wa2[l] / dxnorm);
    }
    LM_SYNC();
    for (int j = 0; j < kN; ++j) {
      double sum = 0.0;
      for (int i = 0; i < j; ++i) sum += LM_R(i, j) * wa1[i];
      const double v = (wa1[j] - sum) / LM_R(j, j);
      LM_SYNC();
      wa1[j] = v;
      LM_SYNC();
    }
    const double temp = enorm3(wa1);
    parl = ((fp / delta) / temp) / temp;
  }
  LM_SYNC();
  for (int j = 0; j < kN; ++j) {
    double sum = 0.0;
    for (int i = 0; i <= j; ++i) sum += LM_R(i, j) * qtb[i];
    wa1[j] = sum / diag[ipvt[j]];
  }
  LM_SYNC();
  const double gnorm = enorm3(wa1);
  double paru = gnorm / delta;
  if (paru == 0.0) paru = kDwarf / (delta < 0.1 ? delta : 0.1);
  par = par > parl ? par : parl;
  par = par < paru ? par : paru;
  if (par == 0.0) par = gnorm / dxnorm;
  for (;;) {
    ++iter;
    if (par == 0.0) par = kDwarf > 0.001 * paru ? kDwarf : 0.001 * paru;
    double temp = sqrt(par);
    LM_SYNC();
    for (int j = 0; j < kN; ++j) wa1[j] = temp * diag[j];
    LM_SYNC();
    qrsolv(r, ld, ipvt, wa1, qtb, x, sdiag, wa2);
    for (int j = 0; j < kN; ++j) wa2[j] = diag[j] * x[j];
    LM_SYNC();
    dxnorm = enorm3(wa2);
    temp = fp;
    fp = dxnorm - delta;
    if (fabs(fp) <= 0.1 * delta || (parl == 0.0 && fp <= temp && temp < 0.0) || iter == 10) break;
    for (int j = 0; j < kN; ++j) {
      const int l = ipvt[j];
      wa1[j] = diag[l] * (wa2[l] / dxnorm);
    }
    LM_SYNC();
    for (int j = 0; j < kN; ++j) {
      const double t = wa1[j] / sdiag[j];
      LM_SYNC();
      wa1[j] = t;
      for (int i = j + 1; i < kN; ++i) {
        const double v = wa1[i] - LM_R(i, j) * t;
        LM_SYNC();
        wa1[i] = v;
      }
      LM_SYNC();
    }
    temp = enorm3(wa1);
    const double parc = ((fp / delta) / temp) / temp;
    if (fp > 0.0) parl = parl > par ? parl : par;
    if (fp < 0.0) paru = paru < par ? paru : par;
    par = parl > par + parc ? parl : par + parc;
  }
  return par;
}

// lmder with mode 1 and gtol 0: w.x holds the start point, then the solution;
// w.fvec the final residuals; the first rows of w.fjac and w.ipvt the final R
// and permutation.  Returns info (MINPACK's 1..8, 5 = maxfev reached).
LM_FN int lmder(const Work& w, int m, double ftol, double xtol, int maxfev, double factor,
                int* nfev_out) {
  double* r = w.fjac;
  const int ld = w.ld;
  int info = 0, nfev = 1, iter = 1;
  residuals(w, m, w.x, w.fvec);
  double fnorm = enorm_team(w.fvec, 0, m);
  double par = 0.0, delta = 0.0, xnorm = 0.0;
  for (;;) {
    jacobian(w, m, w.x);
    qrfac(w, m, w.wa1, w.wa2, w.wa3);
    if (iter == 1) {
      for (int j = 0; j < kN; ++j) w.diag[j] = w.wa2[j] == 0.0 ? 1.0 : w.wa2[j];
      LM_SYNC();
      for (int j = 0; j < kN; ++j) w.wa3[j] = w.diag[j] * w.x[j];
      LM_SYNC();
      xnorm = enorm3(w.wa3);
      delta = factor * xnorm;
      if (delta == 0.0) delta = factor;
    }
    // the first three components of (q transpose) * fvec
    for (int i = LM_LANE; i < m; i += LM_NL) w.wa4[i] = w.fvec[i];
    LM_SYNC();
    for (int j = 0; j < kN; ++j) {
      const double ajj = r[j * ld + j];
      if (ajj != 0.0) {
        double sum = 0.0;
        for (int i = j + LM_LANE; i < m; i += LM_NL) sum += r[j * ld + i] * w.wa4[i];
        sum = LM_SUM(sum);
        const double temp = -sum / ajj;
        for (int i = j + LM_LANE; i < m; i += LM_NL) w.wa4[i] += r[j * ld + i] * temp;
        LM_SYNC();
      }
      const double q = w.wa4[j];
      LM_SYNC();
      r[j * ld + j] = w.wa1[j];
      w.qtf[j] = q;
      LM_SYNC();
    }
    double gnorm = 0.0;
    if (fnorm != 0.0) {
      for (int j = 0; j < kN; ++j) {
        const int l = w.ipvt[j];
        if (w.wa2[l] == 0.0) continue;
        double sum = 0.0;
        for (int i = 0; i <= j; ++i) sum += LM_R(i, j) * (w.qtf[i] / fnorm);
        const double g = fabs(sum / w.wa2[l]);
        gnorm = gnorm > g ? gnorm : g;
      }
    }
    if (gnorm <= 0.0) info = 4;  // gtol = 0
    if (info != 0) break;
    LM_SYNC();
    for (int j = 0; j < kN; ++j) w.diag[j] = w.diag[j] > w.wa2[j] ? w.diag[j] : w.wa2[j];
    LM_SYNC();
    double ratio;
    do {
      par = lmpar(r, ld, w.ipvt, w.diag, w.qtf, delta, par, w.wa1, w.sdiag, w.xs, w.wq);
      LM_SYNC();
      for (int j = 0; j < kN; ++j) {
        const double p = -w.wa1[j];
        w.wa1[j] = p;
        w.wa2[j] = w.x[j] + p;
        w.wa3[j] = w.diag[j] * p;
      }
      LM_SYNC();
      const double pnorm = enorm3(w.wa3);
      if (iter == 1) delta = delta < pnorm ? delta : pnorm;
      residuals(w, m, w.wa2, w.wa4);
      ++nfev;
      const double fnorm1 = enorm_team(w.wa4, 0, m);
      double actred = -1.0;
      // (as MINPACK writes it: a NaN fnorm1 leaves actred at -1, so the trial is
      // rejected and delta shrinks)
      if (0.1 * fnorm1 < fnorm) {
        const double t = fnorm1 / fnorm;
        actred = 1.0 - t * t;
      }
      LM_SYNC();
      for (int j = 0; j < kN; ++j) w.wa3[j] = 0.0;
      LM_SYNC();
      for (int j = 0; j < kN; ++j) {
        const double temp = w.wa1[w.ipvt[j]];
        for (int i = 0; i <= j; ++i) {
          const double v = w.wa3[i] + LM_R(i, j) * temp;
          LM_SYNC();
          w.wa3[i] = v;
          LM_SYNC();
        }
      }
      const double temp1 = enorm3(w.wa3) / fnorm;
      const double temp2 = (sqrt(par) * pnorm) / fnorm;
      const double prered = temp1 * temp1 + (temp2 * temp2) / 0.5;
      const double dirder = -(temp1 * temp1 + temp2 * temp2);
      ratio = 0.0;
      if (prered != 0.0) ratio = actred / prered;
      if (!(ratio > 0.25)) {
        double temp = 0.5;  // (actred >= 0; a NaN keeps it too)
        if (actred < 0.0) temp = 0.5 * dirder / (dirder + 0.5 * actred);
        if (0.1 * fnorm1 >= fnorm || temp < 0.1) temp = 0.1;
        const double pn = pnorm / 0.1;
        delta = temp * (delta < pn ? delta : pn);
        par = par / temp;
      } else if (!(par != 0.0 && ratio < 0.75)) {
        delta = pnorm / 0.5;
        par = 0.5 * par;
      }
      if (!(ratio < 1e-4)) {
        LM_SYNC();
        for (int j = 0; j < kN; ++j) {
          const double xj = w.wa2[j];
          w.x[j] = xj;
        }
        LM_SYNC();
        for (int j = 0; j < kN; ++j) w.wa2[j] = w.diag[j] * w.x[j];
        for (int i = LM_LANE; i < m; i += LM_NL) w.fvec[i] = w.wa4[i];
        LM_SYNC();
        xnorm = enorm3(w.wa2);
        fnorm = fnorm1;
        ++iter;
      }
      const bool fconv = fabs(actred) <= ftol && prered <= ftol && 0.5 * ratio <= 1.0;
      if (fconv) info = 1;
      if (delta <= xtol * xnorm) info = 2;
      if (fconv && info == 2) info = 3;
      if (info != 0) break;
      if (nfev >= maxfev) info = 5;
      if (fabs(actred) <= kEpsMch && prered <= kEpsMch && 0.5 * ratio <= 1.0) info = 6;
      if (delta <= kEpsMch * xnorm) info = 7;
      if (gnorm <= kEpsMch) info = 8;
      if (info != 0) break;
    } while (ratio < 1e-4);
    if (info != 0) break;
  }
  *nfev_out = nfev;
  return info;
}

// The whole fit of one profile y[0 .. m) (already in w.y): start point, lmder,
// the model at the clipped solution, and the parameter errors as
// scipy.optimize.leastsq and astropy form them: cov_x = P inv(R) inv(R)^T P^T
// from the final R and permutation (LAPACK trtri's column order), times
// sum(fvec^2) / (m - 3).  fitted [rcap] (NaN beyond m), params [3], perr [3],
// info [2] = ier, nfev.  m < 3 or a non-finite value: ier 0, everything NaN;
// perr is NaN where leastsq returns no cov_x (singular R, exit code not 1 .. 4)
// and for m <= 3.
LM_FN void fit_gauss1d(const Work& w, int m, int rcap, double fwhm, double* fitted,
                       double* params, double* perr, int* info) {
  const double nan = NAN;
  double bad = (m < 3 || m > rcap) ? 1.0 : 0.0, ymax = -INFINITY;
  if (bad == 0.0) {
    for (int i = LM_LANE; i < m; i += LM_NL) {
      const double v = w.y[i];
      if (!(fabs(v) <= 1.79769313486231570815e308)) bad = 1.0;
      ymax = v > ymax ? v : ymax;
    }
  }
  bad = LM_MAX(bad);
  ymax = LM_MAX(ymax);
  if (bad != 0.0) {
    for (int i = LM_LANE; i < rcap; i += LM_NL) fitted[i] = nan;
    if (LM_LANE == 0) {
      for (int j = 0; j < kN; ++j) params[j] = nan, perr[j] = nan;
      info[0] = 0, info[1] = 0;
    }
    return;
  }
  w.x[0] = 0.8 * ymax;
  w.x[1] = 0.0;
  w.x[2] = fwhm / kFwhmPerSigma;
  LM_SYNC();
  int nfev = 0;
  const int ier = lmder(w, m, 1.49012e-8, 1e-7, 100, 100.0, &nfev);
  LM_SYNC();
  const double a = w.x[0], mu = w.x[1];
  const double s = w.x[2] >= kTiny32 ? w.x[2] : kTiny32;
  const double ss = s * s;
  for (int i = LM_LANE; i < rcap; i += LM_NL) {
    const double d = (double)i - mu;
    fitted[i] = i < m ? a * exp((-0.5 * (d * d)) / ss) : nan;
  }
  double ssq = 0.0;
  for (int i = LM_LANE; i < m; i += LM_NL) ssq += w.fvec[i] * w.fvec[i];
  ssq = LM_SUM(ssq);
  const double* r = w.fjac;
  const int ld = w.ld;
  const double r00 = r[0], r01 = r[ld], r02 = r[2 * ld], r11 = r[ld + 1], r12 = r[2 * ld + 1],
               r22 = r[2 * ld + 2];
  // inv(R), column by column (x = T x for the triangle already inverted, then
  // scaled by minus the new diagonal entry)
  const double i00 = 1.0 / r00, i11 = 1.0 / r11, i22 = 1.0 / r22;
  const double i01 = (r01 * i00) * -i11;
  const double i02 = (r02 * i00 + r12 * i01) * -i22;
  const double i12 = (r12 * i11) * -i22;
  // (leastsq forms cov_x only after the exit codes 1 .. 4)
  const bool singular = r00 == 0.0 || r11 == 0.0 || r22 == 0.0 || m <= kN || ier < 1 || ier > 4;
  const double scale = ssq / (double)(m - kN);
  w.wq[0] = (i00 * i00 + i01 * i01 + i02 * i02) * scale;
  w.wq[1] = (i11 * i11 + i12 * i12) * scale;
  w.wq[2] = (i22 * i22) * scale;
  LM_SYNC();
  if (LM_LANE == 0) {
    params[0] = a, params[1] = mu, params[2] = s;
    for (int j = 0; j < kN; ++j) perr[w.ipvt[j]] = singular ? nan : sqrt(fabs(w.wq[j]));
    info[0] = ier, info[1] = nfev;
  }
}

#undef LM_R

}  // namespace bsgp_lm
