// Host test of the PSF fit's host-compilable pieces (csrc/bsgp_psffit.hpp and
// the basis of csrc/bsgp_psf.hpp), against matrices worked out by hand:
//  1. the packed index rules;
//  2. psffit_scale, psffit_cholesky and psffit_solve on a 3 x 3 matrix whose
//     factor and solution are small integers (every step exact), the pivot
//     test on singular, negative, NaN, infinite and rounding-size pivots, and
//     a random well-conditioned system against its residual;
//  3. psffit_rss on a two-coefficient model, with and without spatial terms;
//  4. the median and the clipping rule;
//  5. psf_terms against psf_pix: the basis is what the evaluation multiplies
//     its coefficients with, term by term in the same order.
#include <cmath>
#include <cstdio>
#include <limits>
#include <random>
#include <vector>

#include "bsgp_psffit.hpp"

using namespace bsgp;

static int fails = 0;
#define CHECK(c)                                               \
  do {                                                         \
    if (!(c)) {                                                \
      if (++fails < 20) printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
    }                                                          \
  } while (0)

static void nosync() {}

static void test_index() {
  int e = 0;
  for (int i = 0; i < 5; ++i)
    for (int j = i; j < 5; ++j) CHECK(psffit_upper(5, i, j) == e++);
  e = 0;
  for (int i = 0; i < 5; ++i)
    for (int j = 0; j <= i; ++j) CHECK(psffit_lower(i, j) == e++);
  const double G[6] = {10, 11, 12, 13, 14, 15};  // 3 x 3
  CHECK(psffit_sym(G, 3, 0, 2) == 12 && psffit_sym(G, 3, 2, 0) == 12);
  CHECK(psffit_sym(G, 3, 1, 1) == 13 && psffit_sym(G, 3, 2, 1) == 14 && psffit_sym(G, 3, 2, 2) == 15);
}

static void test_cholesky() {
  // A = L L^T with L = [2; 1 2; 1 1 2]; A z = b for z = (1, 2, 3)
  double A[6] = {4, 2, 5, 2, 3, 6};
  CHECK(psffit_cholesky(A, 3, 0, 1, nosync));
  const double L[6] = {2, 1, 2, 1, 1, 2};
  for (int i = 0; i < 6; ++i) CHECK(A[i] == L[i]);
  double x[3] = {14, 21, 26};
  psffit_solve(A, x, 3, 0, 1, nosync);
  CHECK(x[0] == 1 && x[1] == 2 && x[2] == 3);

  // scaling: N = [16 8; 8 25] -> d = (4, 5), A = [1 .4; .4 1]
  double N[3] = {16, 8, 25}, d[2];
  psffit_scale(N, d, 2, 0, 1, nosync);
  CHECK(d[0] == 4 && d[1] == 5 && N[0] == 1 && N[2] == 1 && N[1] == 8.0 / 20.0);

  // pivots the factorisation refuses
  const double eps = std::numeric_limits<double>::epsilon();  // 2^-52
  CHECK(psffit_pivot_floor(36) == 36 * eps);
  double S1[3] = {1, 1, 1};  // second pivot 0
  CHECK(!psffit_cholesky(S1, 2, 0, 1, nosync));
  double S2[3] = {1, 1, 1 + eps};  // second pivot 2^-52 <= 2 * 2^-52
  CHECK(!psffit_cholesky(S2, 2, 0, 1, nosync));
  double S3[3] = {1, 1, 1 + 4 * eps};  // 4 * 2^-52 > 2 * 2^-52
  CHECK(psffit_cholesky(S3, 2, 0, 1, nosync));
  double S4[3] = {-1, 0, 1};
  CHECK(!psffit_cholesky(S4, 2, 0, 1, nosync));
  double S5[3] = {std::nan(""), 0, 1};
  CHECK(!psffit_cholesky(S5, 2, 0, 1, nosync));
  double S6[3] = {1, 0, std::numeric_limits<double>::infinity()};
  CHECK(!psffit_cholesky(S6, 2, 0, 1, nosync));
  double Z[3] = {0, 0, 0}, dz[2];  // no stars: 0 / 0 on the diagonal
  psffit_scale(Z, dz, 2, 0, 1, nosync);
  CHECK(!psffit_cholesky(Z, 2, 0, 1, nosync));

  // a random system: M = B B^T + P I, scaled, factored, solved; the residual is rounding
  const int P = 36;
  std::mt19937_64 rng(5);
  std::uniform_real_distribution<double> u(-1.0, 1.0);
  std::vector<double> B(P * P), M(P * (P + 1) / 2), M0, rhs(P), z(P), dd(P);
  for (auto& v : B) v = u(rng);
  for (int i = 0; i < P; ++i)
    for (int j = 0; j <= i; ++j) {
      double s = i == j ? (double)P : 0.0;
      for (int k = 0; k < P; ++k) s += B[i * P + k] * B[j * P + k];
      M[psffit_lower(i, j)] = s * (1.0 + i) * (1.0 + j);  // rows of very different size
    }
  M0 = M;
  for (int i = 0; i < P; ++i) rhs[i] = z[i] = u(rng) * (1.0 + i);
  psffit_scale(M.data(), dd.data(), P, 0, 1, nosync);
  for (int i = 0; i < P; ++i) CHECK(std::fabs(M[psffit_lower(i, i)] - 1.0) <= 2e-16);
  CHECK(psffit_cholesky(M.data(), P, 0, 1, nosync));
  for (int i = 0; i < P; ++i) z[i] = z[i] / dd[i];
  psffit_solve(M.data(), z.data(), P, 0, 1, nosync);
  for (int i = 0; i < P; ++i) z[i] = z[i] / dd[i];
  double worst = 0.0;
  for (int i = 0; i < P; ++i) {
    double s = 0.0;
    for (int j = 0; j < P; ++j) s += M0[i >= j ? psffit_lower(i, j) : psffit_lower(j, i)] * z[j];
    worst = std::fmax(worst, std::fabs(s - rhs[i]) / (1.0 + i));
  }
  printf("random %d x %d system: largest scaled residual %.3g\n", P, P, worst);
  CHECK(worst < 1e-12);
}

static void test_rss() {
  // c = (2, 3), G = [1 2; 2 5], h = (1, 1), vv = 100: c.h = 5, c.G c = 4 + 24 + 45 = 73
  const double c0[2] = {2, 3}, G[3] = {1, 2, 5}, h[2] = {1, 1};
  CHECK(psffit_rss(c0, 2, 0, 7.0, -3.0, G, h, 100.0) == 163.0);
  CHECK(psffit_rss(c0, 2, 0, 0.0, 0.0, G, h, -100.0) == 0.0);  // clamped
  // sdeg = 1, terms 1, dy, dx: c(dx, dy) = (1 + 1 dy + 0.5 dx, 1 + 0 dy + 1 dx) = (2, 3) at (2, 0)... dy = 0
  const double c1[6] = {1, 1, 1, 0, 0.5, 1};
  CHECK(psf_local_coef_at(c1, 2, 1, 0, 2.0, 0.0) == 2.0);
  CHECK(psf_local_coef_at(c1, 2, 1, 1, 2.0, 0.0) == 3.0);
  CHECK(psf_local_coef_at(c1, 2, 1, 0, 0.0, 4.0) == 5.0);
  CHECK(psffit_rss(c1, 2, 1, 2.0, 0.0, G, h, 100.0) == 163.0);
}

static void test_clip() {
  const double s[5] = {1, 2, 4, 8, 16};
  CHECK(psffit_median_sorted(s, 5) == 4 && psffit_median_sorted(s, 4) == 3);
  CHECK(psffit_median_sorted(s, 1) == 1 && psffit_median_sorted(s, 2) == 1.5);
  const double thr = psffit_clip_threshold(1.0, 0.5, 2.0);
  CHECK(thr == 1.0 + 2.0 * 1.4826 * 0.5);
  const double eps = std::numeric_limits<double>::epsilon();
  CHECK(psffit_drop(3.0, thr, 1.0, 1.0));
  CHECK(!psffit_drop(thr, thr, 1.0, 1.0));                  // strict
  CHECK(!psffit_drop(3.0, thr, 4096 * eps * 7.0, 7.0));     // rounding noise of vv = 7
  CHECK(psffit_drop(3.0, thr, 4097 * eps * 7.0, 7.0));
  CHECK(!psffit_drop(std::nan(""), thr, 1.0, 1.0));
  CHECK(!psffit_round_applies(10, 0, 3, 0));  // nothing dropped
  CHECK(psffit_round_applies(10, 7, 3, 0));   // 3 remain, nterm = 3
  CHECK(!psffit_round_applies(10, 8, 3, 0));
  CHECK(!psffit_round_applies(10, 5, 3, 6) && psffit_round_applies(10, 4, 3, 6));
}

static void test_basis() {
  PsfModel M{};
  M.cosv = 0.8, M.sinv = 0.6, M.ax = -0.11, M.ay = -0.07, M.sig2 = 0.548 * 0.548;
  M.ngauss = 2, M.ldeg = 2, M.sdeg = 0, M.ncomp = 12;
  double loc[12], phi[12];
  for (int k = 0; k < 12; ++k) loc[k] = 0.3 * (k + 1) * ((k & 1) ? -1 : 1);
  const double x = 1.37, y = -2.61;
  double manual = 0.0;
  int seen = 0;
  psf_terms(M, x, y, [&](int k, double e, double a1, double a2) {
    CHECK(k == seen++);
    phi[k] = e * a1 * a2;
    manual += loc[k] * e * a1 * a2;
  });
  CHECK(seen == 12);
  CHECK(manual == psf_pix(M, loc, x, y));
  // the first Gaussian's terms: 1, y, y^2, x, x y, x^2 times exp(rr)
  const double x1 = 0.8 * x - 0.6 * y, y1 = 0.6 * x + 0.8 * y;
  const double e0 = std::exp(-0.11 * x1 * x1 + -0.07 * y1 * y1);
  CHECK(phi[0] == e0 && phi[1] == e0 * 1.0 * y && phi[2] == e0 * 1.0 * (y * y));
  CHECK(phi[3] == e0 * x && phi[4] == e0 * x * y && phi[5] == e0 * (x * x));
  // at the origin only the constant terms are left
  psf_terms(M, 0.0, 0.0, [&](int k, double e, double a1, double a2) { phi[k] = e * a1 * a2; });
  for (int k = 0; k < 12; ++k) CHECK(phi[k] == ((k % 6) == 0 ? 1.0 : 0.0));
  // the same function serves a PsfShape
  PsfShape S{};
  S.cosv = M.cosv, S.sinv = M.sinv, S.ax = M.ax, S.ay = M.ay, S.sig2 = M.sig2;
  S.ngauss = 2, S.ldeg = 2;
  double q[12];
  psf_terms(M, x, y, [&](int k, double e, double a1, double a2) { phi[k] = e * a1 * a2; });
  psf_terms(S, x, y, [&](int k, double e, double a1, double a2) { q[k] = e * a1 * a2; });
  for (int k = 0; k < 12; ++k) CHECK(q[k] == phi[k]);
}

int main() {
  test_index();
  test_cholesky();
  test_rss();
  test_clip();
  test_basis();
  if (fails) {
    printf("%d checks failed\n", fails);
    return 1;
  }
  printf("all ok\n");
  return 0;
}
