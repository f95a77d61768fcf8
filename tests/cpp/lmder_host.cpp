// Host build of the Gaussian1D profile fit (csrc/bsgp_lmder.hpp) with a team
// of one lane: tests/test_stamps.py compiles this file into a shared library
// and compares it with the scipy.optimize.leastsq results of the fixture.
#include <cmath>
#include <vector>

#define LM_FN static inline
#define LM_LANE 0
#define LM_NL 1
#define LM_SYNC() ((void)0)
#define LM_SUM(v) (v)
#define LM_MAX(v) (v)
#include "bsgp_lmder.hpp"

extern "C" void lmder_host_fit(const double* prof, int m, int rcap, double fwhm, double* fitted,
                               double* params, double* perr, int* info) {
  const int ld = rcap > 0 ? rcap : 1;
  std::vector<double> buf(6 * (size_t)ld + bsgp_lm::kSmallDoubles);
  int ipvt[bsgp_lm::kN] = {0, 0, 0};
  bsgp_lm::Work w{};
  w.y = buf.data();
  w.fvec = w.y + ld;
  w.wa4 = w.fvec + ld;
  w.fjac = w.wa4 + ld;
  w.ld = ld;
  double* sm = w.fjac + 3 * ld;
  w.x = sm, w.diag = sm + 3, w.qtf = sm + 6, w.wa1 = sm + 9, w.wa2 = sm + 12, w.wa3 = sm + 15;
  w.sdiag = sm + 18, w.xs = sm + 21, w.wq = sm + 24;
  w.ipvt = ipvt;
  for (int i = 0; i < m && i < rcap; ++i) w.y[i] = prof[i];
  bsgp_lm::fit_gauss1d(w, m, rcap, fwhm, fitted, params, perr, info);
}
