// bsgp_validate.hpp — the leaf plan of numpy's sum of n contiguous doubles, as
// the source validation (bsgp_validate.hip) evaluates it in
// parallel.  np.sum hands the values to its add loop in buffers of 8192
// (numpy's default buffer size) and chains the buffers' sums left to right;
// inside a buffer the sum is pairwise: a recursion that halves a range (the
// left half a multiple of 8 long) until it holds at most 128 values, sums such
// a leaf with 8 accumulators (np_pairwise_block, bsgp_prims.hpp) and adds the
// halves left before right.  Up to 8192 values this is np_pairwise_sum of
// bsgp_prims.hpp.  The leaves depend on n alone, so they can be summed
// independently, one per lane, and folded afterwards in numpy's order.
// Everything here is a pure function of n and compiles on the host
// (tests/cpp/validate_plan.cpp holds it against np.sum).
#pragma once

#include "bsgp_prims.hpp"

namespace bsgp {

constexpr int kPairwiseDepth = 32;  // levels of the recursion for any int n
constexpr int kNpBufSize = 8192;    // values of one buffer of numpy's reduction
// leaves of a window of at most BSGP_VALIDATE_MAX = 16384 values: one per thread
// (tests/cpp/validate_plan.cpp counts them for every such n)
constexpr int kValidateMaxLeaves = 256;

// the recursion's explicit stack; the caller owns it (LDS on the device: a
// private array indexed by the depth would live in scratch)
struct PairwiseStack {
  int off[kPairwiseDepth], len[kPairwiseDepth], stage[kPairwiseDepth];
  double left[kPairwiseDepth];
};

// One walk over the pairwise recursion of the n values from `base`; *li counts
// the leaves met, over the calls.  lsum == nullptr: the leaves, left to right,
// go to loff / llen (entries below max_leaves are written).  lsum != nullptr:
// leaf i's sum is lsum[i] and the return value is the range's sum, folded as
// numpy folds it.
BSGP_HD double np_pairwise_walk(int base, int n, PairwiseStack* st, int* loff, int* llen,
                                int max_leaves, const double* lsum, int* li) {
  int sp = 0;
  st->off[0] = base;
  st->len[0] = n;
  st->stage[0] = 0;
  for (;;) {
    if (st->len[sp] > 128 && st->stage[sp] == 0 && sp + 1 < kPairwiseDepth) {  // the left half
      int n2 = st->len[sp] / 2;
      n2 -= n2 % 8;
      st->stage[sp] = 1;
      st->off[sp + 1] = st->off[sp];
      st->len[sp + 1] = n2;
      st->stage[sp + 1] = 0;
      ++sp;
      continue;
    }
    double ret = 0.0;
    if (lsum)
      ret = lsum[*li];
    else if (*li < max_leaves)
      loff[*li] = st->off[sp], llen[*li] = st->len[sp];
    ++*li;
    for (;;) {  // hand `ret` up the stack
      if (sp == 0) return ret;
      --sp;
      if (st->stage[sp] == 1) {  // left half done: the right half
        st->left[sp] = ret;
        st->stage[sp] = 2;
        int n2 = st->len[sp] / 2;
        n2 -= n2 % 8;
        st->off[sp + 1] = st->off[sp] + n2;
        st->len[sp + 1] = st->len[sp] - n2;
        st->stage[sp + 1] = 0;
        ++sp;
        break;
      }
      ret = st->left[sp] + ret;
    }
  }
}

// np.sum's order over n values: buffer after buffer.  lsum == nullptr: fills
// the leaf table and returns the number of leaves; else returns the sum.
BSGP_HD double np_sum_walk(int n, PairwiseStack* st, int* loff, int* llen, int max_leaves,
                           const double* lsum) {
  int li = 0;
  double tot = 0.0;
  for (int c = 0; c == 0 || c < n; c += kNpBufSize) {
    const int len = n - c < kNpBufSize ? n - c : kNpBufSize;
    const double r = np_pairwise_walk(c, len, st, loff, llen, max_leaves, lsum, &li);
    tot = c == 0 ? r : tot + r;
  }
  return lsum ? tot : (double)li;
}

// host: the leaf table of n values; returns the number of leaves (which may
// exceed max_leaves: then only the first max_leaves are written)
inline int np_sum_leaves(int n, int* loff, int* llen, int max_leaves) {
  PairwiseStack st;
  return (int)np_sum_walk(n, &st, loff, llen, max_leaves, nullptr);
}

// host: np.sum(a[0 .. n)) through the plan -- every leaf summed on its own,
// then the fold; what the kernel computes with one leaf per lane.  n must have
// at most kValidateMaxLeaves leaves (n <= 16384 has), else NaN.
inline double np_sum_planned(const double* a, int n) {
  int loff[kValidateMaxLeaves], llen[kValidateMaxLeaves];
  double lsum[kValidateMaxLeaves];
  PairwiseStack st;
  const int nl = np_sum_leaves(n, loff, llen, kValidateMaxLeaves);
  if (nl > kValidateMaxLeaves) return order_value(0xfff8000000000000ULL);
  for (int i = 0; i < nl; ++i) lsum[i] = np_pairwise_block(a + loff[i], llen[i]);
  return np_sum_walk(n, &st, nullptr, nullptr, 0, lsum);
}

}  // namespace bsgp
