// bsgp_lanesplit.hpp — index maps of the wide (two pixels per lane) operand
// loads of the per-wave row passes (row_fwd2 / row_inv2, bsgp_device.hpp).
// Plain integer functions shared by the device code and the host unit test
// (tests/cpp/lane_split_test.cpp).
//
// A row pair (r, r+1) of an even-width image is moved 64 columns at a time.
// Half-wave h = lane >> 5 loads row r + h; lane i = lane & 31 of it loads
// the adjacent columns j0 + 2i and j0 + 2i + 1 in one access (`first`,
// `second`).  One swap of the upper 32 lanes of `first` with the lower 32
// lanes of `second` (v_permlane32_swap) then leaves in every lane ONE column
// of BOTH rows: `first` = row r, `second` = row r + 1, at column
// j0 + split_col(lane).  The narrow scheme's lane L (column j0 + L of both
// rows) is lane split_lane(L) here, with the same pixels in the same order,
// so per-lane partial sums are bitwise the narrow scheme's after one
// lane permutation, and every lane stores its own pixels as before.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define BSGP_SPLIT_HD __host__ __device__
#else
#define BSGP_SPLIT_HD
#endif

namespace bsgp {

// row (0: r, 1: r + 1) a lane loads
BSGP_SPLIT_HD constexpr int split_half(int lane) { return lane >> 5; }
// first column of the lane's pair, relative to the chunk start
BSGP_SPLIT_HD constexpr int split_pair(int lane) { return 2 * (lane & 31); }
// A pair past the row end is clamped as a whole to the last pair (ncols is
// even and >= 2): the access stays in bounds and aligned, the values unused.
BSGP_SPLIT_HD constexpr int split_pair_clamped(int j0, int lane, int ncols) {
  return (j0 + split_pair(lane) < ncols - 2) ? j0 + split_pair(lane) : ncols - 2;
}
// column (relative to the chunk start) whose pixels of both rows a lane
// holds after the swap
BSGP_SPLIT_HD constexpr int split_col(int lane) { return 2 * (lane & 31) + (lane >> 5); }
// the lane that holds column L of the chunk: the inverse of split_col
BSGP_SPLIT_HD constexpr int split_lane(int L) { return (L >> 1) | ((L & 1) << 5); }

}  // namespace bsgp
