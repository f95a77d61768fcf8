// Host test of the wide row-pass load maps (csrc/bsgp_lanesplit.hpp): 64
// simulated lanes, the half-wave swap (v_permlane32_swap) modelled on arrays.
//  1. split_col / split_lane are inverse permutations; per-lane partials moved
//     back through split_lane reduce (sum and max, today's butterfly xor 32,
//     16, 8, 4, 2, 1) to the bits the narrow scheme gives, and so does the
//     reordered butterfly (xor 16, 8, 4, 2, 1, 32) on the unmoved partials.
//  2. For W in {64, 70, 130, 256} and even and odd H: every pixel of every row
//     pair is loaded by an in-bounds, pair-aligned access, lands after the
//     swap in lane split_col^-1(column) with row r in `first` and row r + 1 in
//     `second`, and is consumed exactly once, in the narrow scheme's order
//     per accumulator, by the lane that (as before) stores column j of rows
//     r and r + 1.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "bsgp_lanesplit.hpp"

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

// v_permlane32_swap: lanes 32..63 of a <-> lanes 0..31 of b
template <class T>
static void half_swap(T (&a)[64], T (&b)[64]) {
  for (int i = 0; i < 32; ++i) {
    const T t = a[32 + i];
    a[32 + i] = b[i];
    b[i] = t;
  }
}

template <class OP>
static void butterfly(double (&v)[64], const int (&order)[6], OP op) {
  for (int o : order) {
    double n[64];
    for (int l = 0; l < 64; ++l) n[l] = op(v[l], v[l ^ o]);
    memcpy(v, n, sizeof(n));
  }
}

static void test_reductions() {
  bool seen[64] = {};
  for (int l = 0; l < 64; ++l) {
    CHECK(split_lane(split_col(l)) == l);
    CHECK(split_col(split_lane(l)) == l);
    CHECK(split_col(l) == split_pair(l) + split_half(l));
    seen[split_col(l)] = true;
  }
  for (int l = 0; l < 64; ++l) CHECK(seen[l]);
  const int today[6] = {32, 16, 8, 4, 2, 1}, reordered[6] = {16, 8, 4, 2, 1, 32};
  auto add = [](double a, double b) { return a + b; };
  auto mx = [](double a, double b) { return (b > a || b != b) ? b : a; };
  std::mt19937_64 rng(7);
  std::uniform_real_distribution<double> mag(-30.0, 30.0), sgn(-1.0, 1.0);
  for (int trial = 0; trial < 200; ++trial) {
    double narrow[64], wide[64], back[64];
    for (int L = 0; L < 64; ++L) narrow[L] = sgn(rng) * std::exp2(mag(rng));
    for (int l = 0; l < 64; ++l) wide[l] = narrow[split_col(l)];  // the same accumulator, moved
    for (int L = 0; L < 64; ++L) back[L] = wide[split_lane(L)];   // split_undo
    for (int L = 0; L < 64; ++L) CHECK(bits(back[L]) == bits(narrow[L]));
    double a[64], b[64], c[64];
    memcpy(a, narrow, sizeof(a));
    memcpy(b, back, sizeof(b));
    memcpy(c, wide, sizeof(c));
    butterfly(a, today, add);
    butterfly(b, today, add);
    butterfly(c, reordered, add);
    for (int l = 0; l < 64; ++l) {
      CHECK(bits(a[l]) == bits(b[l]));
      CHECK(bits(a[0]) == bits(c[l]));  // every lane holds the total
    }
    memcpy(a, narrow, sizeof(a));
    memcpy(c, wide, sizeof(c));
    butterfly(a, today, mx);
    butterfly(c, today, mx);  // max in any order
    CHECK(bits(a[0]) == bits(c[0]));
  }
}

struct Px {
  int row, col;
};

static void test_maps(int H, int W) {
  const int N = H * W;
  std::vector<double> in(N);
  std::vector<int> consumed(N, 0);
  for (int i = 0; i < N; ++i) in[i] = 1000.0 + i;
  // consumption order per accumulator: narrow lane L against wide lane split_lane(L)
  std::vector<Px> seq_narrow[64], seq_wide[64];
  for (int r = 0; r < H; r += 2) {
    const bool two = r + 1 < H;
    for (int j0 = 0; j0 < W; j0 += 64) {
      for (int L = 0; L < 64; ++L) {  // today's scheme
        const int j = j0 + L;
        if (j < W) {
          seq_narrow[L].push_back({r, j});
          if (two) seq_narrow[L].push_back({r + 1, j});
        }
      }
      double first[64], second[64];
      for (int l = 0; l < 64; ++l) {  // one access per lane
        const int rr = (two && split_half(l)) ? r + 1 : r;
        const int jp = split_pair_clamped(j0, l, W);
        CHECK(jp >= 0 && jp + 1 < W && rr < H);
        CHECK(((rr * W + jp) & 1) == 0);  // aligned to the pair
        first[l] = in[rr * W + jp];
        second[l] = in[rr * W + jp + 1];
      }
      half_swap(first, second);
      for (int l = 0; l < 64; ++l) {
        const int j = j0 + split_col(l);
        if (j < W) {
          CHECK(first[l] == in[r * W + j]);
          ++consumed[r * W + j];
          seq_wide[l].push_back({r, j});
          if (two) {
            CHECK(second[l] == in[(r + 1) * W + j]);
            ++consumed[(r + 1) * W + j];
            seq_wide[l].push_back({r + 1, j});
          }
        }
      }
    }
  }
  for (int i = 0; i < N; ++i) {
    CHECK(consumed[i] == 1);
  }
  for (int L = 0; L < 64; ++L) {
    const std::vector<Px>&a = seq_narrow[L], &b = seq_wide[split_lane(L)];
    CHECK(a.size() == b.size());
    for (size_t k = 0; k < a.size() && k < b.size(); ++k)
      CHECK(a[k].row == b[k].row && a[k].col == b[k].col);
  }
}

int main() {
  test_reductions();
  for (int W : {64, 70, 130, 256})
    for (int H : {1, 6, 7}) test_maps(H, W);
  test_maps(4, 2);  // the smallest even width: every pair clamps to (0, 1)
  if (fails) {
    printf("%d checks failed\n", fails);
    return 1;
  }
  printf("all ok\n");
  return 0;
}
