// Host side of tests/test_validate.py: the leaf plan of numpy's pairwise sum
// (csrc/bsgp_validate.hpp) behind a C interface, built as a shared library and
// called through ctypes, so that the sums can be held against np.sum itself.
#include "bsgp_validate.hpp"

using namespace bsgp;

extern "C" {

// the leaves of n values; returns their number
int vp_leaves(int n, int* off, int* len, int max_leaves) {
  return np_sum_leaves(n, off, len, max_leaves);
}

// np.sum(a[0 .. n)) leaf by leaf, then the fold: the kernel's order
double vp_sum(const double* a, int n) { return np_sum_planned(a, n); }

// the recursion alone (bsgp_prims.hpp): np.sum up to one buffer of 8192 values
double vp_sum_recursive(const double* a, int n) { return np_pairwise_sum(a, n); }

// For every n in 1 .. nmax: the leaves tile [0, n) in order, each holds 1 to
// 128 values (n itself when n <= 128).  Returns the largest number of leaves,
// or -n for the first n that fails.
int vp_check_upto(int nmax) {
  static int off[4096], len[4096];
  int most = 0;
  for (int n = 1; n <= nmax; ++n) {
    const int nl = np_sum_leaves(n, off, len, 4096);
    if (nl < 1 || nl > 4096) return -n;
    int at = 0;
    for (int i = 0; i < nl; ++i) {
      if (off[i] != at || len[i] < 1 || len[i] > 128) return -n;
      at += len[i];
    }
    if (at != n) return -n;
    most = nl > most ? nl : most;
  }
  return most;
}

int vp_max_leaves(void) { return kValidateMaxLeaves; }

}  // extern "C"
