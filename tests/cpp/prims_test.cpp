// Host test of the application kernels' shared helpers that compile on the
// host (csrc/bsgp_prims.hpp):
//  1. order_key / order_value: the round trip keeps every bit, and the key is
//     strictly increasing over a sorted list from -inf to +inf through both
//     zeros and the denormals (-0.0 before +0.0).
//  2. np_pairwise_sum is np_pairwise_block up to one leaf (n <= 128), and
//     np_pairwise_block is numpy's leaf: a plain loop below 8 values, else
//     eight strided accumulators, their fixed fold, then the remainder.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>

#include "bsgp_prims.hpp"

using namespace bsgp;

static int fails = 0;
#define CHECK(c)                                               \
  do {                                                         \
    if (!(c)) {                                                \
      if (++fails < 20) printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
    }                                                          \
  } while (0)

static uint64_t bits(double v) {
  uint64_t u;
  memcpy(&u, &v, 8);
  return u;
}

static void test_order_key() {
  using lim = std::numeric_limits<double>;
  const double sorted[] = {-lim::infinity(), -lim::max(), -1.0, -lim::denorm_min(), -0.0, 0.0,
                           lim::denorm_min(), 1.0, lim::max(), lim::infinity()};
  const int n = (int)(sizeof sorted / sizeof sorted[0]);
  for (int i = 0; i < n; ++i) {
    CHECK(bits(order_value(order_key(sorted[i]))) == bits(sorted[i]));
    if (i > 0) CHECK(order_key(sorted[i - 1]) < order_key(sorted[i]));
  }
  CHECK(order_key(-0.0) < order_key(0.0));
  std::mt19937_64 rng(11);
  for (int t = 0; t < 100000; ++t) {  // any bit pattern, NaNs included
    const uint64_t u = rng();
    double d;
    memcpy(&d, &u, 8);
    CHECK(bits(order_value(order_key(d))) == u);
  }
  std::uniform_real_distribution<double> mag(-300.0, 300.0), sgn(-1.0, 1.0);
  for (int t = 0; t < 100000; ++t) {
    const double x = sgn(rng) * std::pow(10.0, mag(rng)), y = sgn(rng) * std::pow(10.0, mag(rng));
    CHECK((x < y) == (order_key(x) < order_key(y)));
  }
}

// numpy's leaf written out: pairwise_sum of numpy/core/src/umath/loops_utils.h.src
static double leaf(const double* a, int n) {
  if (n < 8) {
    double s = 0.0;
    for (int i = 0; i < n; ++i) s += a[i];
    return s;
  }
  double r0 = a[0], r1 = a[1], r2 = a[2], r3 = a[3], r4 = a[4], r5 = a[5], r6 = a[6], r7 = a[7];
  int i = 8;
  for (; i < n - (n % 8); i += 8) {
    r0 += a[i + 0];
    r1 += a[i + 1];
    r2 += a[i + 2];
    r3 += a[i + 3];
    r4 += a[i + 4];
    r5 += a[i + 5];
    r6 += a[i + 6];
    r7 += a[i + 7];
  }
  double s = ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7));
  for (; i < n; ++i) s += a[i];
  return s;
}

static void test_pairwise() {
  std::mt19937_64 rng(5);
  std::uniform_real_distribution<double> mag(-20.0, 20.0), sgn(-1.0, 1.0);
  double a[128];
  for (int trial = 0; trial < 50; ++trial) {
    for (double& v : a) v = sgn(rng) * std::exp2(mag(rng));  // sums that round at every step
    for (int n = 0; n <= 128; ++n)
      CHECK(bits(np_pairwise_sum(a, n)) == bits(np_pairwise_block(a, n)));
    for (int n : {0, 1, 7, 8, 9, 15, 16, 127, 128})
      CHECK(bits(np_pairwise_block(a, n)) == bits(leaf(a, n)));
  }
}

int main() {
  test_order_key();
  test_pairwise();
  if (fails) {
    printf("%d checks failed\n", fails);
    return 1;
  }
  printf("all ok\n");
  return 0;
}
