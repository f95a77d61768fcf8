// bsgp_layout.hpp — the part of the host layer that needs no device and no HIP
// header: the error string, the environment knobs, the plan layout and numpy's
// float32 reduction program.  bsgp_host.hpp includes it for the library;
// tests/cpp/plan_layout_test.cpp includes it alone and builds with plain g++.
#pragma once

#include <algorithm>
#include <cerrno>
#include <cstddef>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../include/bsgp.h"
#include "bsgp_fft.hpp"

namespace bsgp {

// The message bsgp_last_error returns: one thread-local string for the whole
// library (an inline variable, so every unit that fails writes the same one).
inline thread_local std::string g_err;

inline int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

inline size_t round_up(size_t v, size_t m) { return (v + m - 1) / m * m; }

// A/B override knobs (environment variables, the default is the literal at the
// call): a value that is not a whole decimal number in [lo, hi] is ignored and
// the default used, so a typo cannot turn into a zero (a spin limit of 0 fails
// every persistent solve with a timeout).
inline long long env_knob(const char* name, long long def, long long lo, long long hi) {
  const char* e = getenv(name);
  if (!e || !*e) return def;
  char* end = nullptr;
  errno = 0;
  const long long v = strtoll(e, &end, 10);
  if (errno != 0 || end == e || *end != '\0' || v < lo || v > hi) return def;
  return v;
}

// The kernels' constants the layout depends on (bsgp_device.hpp kWaves of the
// 256-thread build, kMaxRed, kSharedBytes; bsgp_internal.hpp kCoopBlock,
// kCoopGroups).  The device headers cannot be included here; bsgp_plan.hip
// static_asserts that these equal them.
namespace layout {
constexpr int kWaves = 4, kMaxRed = 24, kSharedBytes = 512, kCoopBlock = 512, kCoopGroups = 4;
constexpr size_t kLdsPerCu = 160 * 1024;
}  // namespace layout

// The plan-time overrides, read from the environment when a plan is created.
struct PlanKnobs {
  int perwave_min_wg;  // BSGP_PERWAVE_MIN_WG: fewest workgroups per CU a per-wave plan may take
  int perwave_tw;      // BSGP_PERWAVE_TW: 1: such a plan's twiddle tables must fit the LDS too
  int coop_elems;      // BSGP_COOP_ELEMS: elements per thread of a cooperative thread group
  static PlanKnobs from_env() {
    return {(int)env_knob("BSGP_PERWAVE_MIN_WG", 2, 2, 4), (int)env_knob("BSGP_PERWAVE_TW", 1, 0, 1),
            (int)env_knob("BSGP_COOP_ELEMS", 8, 4, 8)};
  }
};

// Everything plan creation decides without a device.  The Geo fields that do
// not point at memory (fp.tw / fq.tw stay nullptr here), the LDS sizes and the
// slot layout.  For the flagship plan (256 x 256, 25 x 25 PSF, linear, float64)
// these are SGeo256's constants (bsgp_device.hpp), which restate the formulas
// below at compile time: the static-geometry path runs only while the two
// agree (static_geo_plan), and tests/test_plan_layout.py pins both.
struct PlanLayout {
  int H, W, P, Q, Qh, sld, lpad, nfw, nfc, coop, tw2, twmix;
  FftPlan fp, fq;        // lengths P (columns) and Q (rows): radices and LDS twiddle offsets
  size_t lds_fft_bytes;  // the transform buffers
  size_t lds_bytes;      // dynamic LDS of every kernel of the plan
  int wg_per_cu;         // workgroups per CU the LDS budget was taken for
  size_t vec_stride;     // doubles per image vector
  size_t spec_off;       // doubles from a slot's start to its spectrum
  size_t slot_stride;    // doubles per slot
};

// Cooperative 2048-point transforms (fft_wide's static plan): their twiddles
// as a two-level table (bsgp_fft.hpp Tw2, 1.5 KiB) at the start of every
// kernel's LDS -- the full 32 KiB table does not fit beside the buffers, and
// from global memory every Stockham stage waited on an L2 round trip --
// and, after them, the 2048-point column transforms' stage tables
// (bsgp_fft.hpp TwMixL: 9 KiB, the global table's entries for the second and
// third Stockham stages; loaded by every kernel with the two-level tables).
// Other cooperative transforms read the global table.
inline void place_coop_tables(PlanLayout* l) {
  PlanLayout& g = *l;
  const size_t tw2b = (64 + 2048 / 64) * sizeof(cd);
  size_t off = 0;
  if (g.P == 2048) {
    g.fp.lds_tw2 = 0;
    off += tw2b;
  }
  if (g.Q == 2048) {
    if (g.P == 2048) {
      g.fq.lds_tw2 = 0;
    } else {
      g.fq.lds_tw2 = (int)off;
      off += tw2b;
    }
  }
  if (g.P == 2048) {
    g.twmix = (int)off;
    off += (64 + 512) * sizeof(cd);
  }
  g.tw2 = (int)round_up(off, 16);
  g.lds_bytes += g.tw2;
}

inline int plan_layout(int H, int W, int kh, int kw, int conv_mode, int storage,
                       const PlanKnobs& knobs, PlanLayout* out) {
  // (local names: the library's units see the kernels' own constants too)
  constexpr int kWaves = layout::kWaves, kMaxRed = layout::kMaxRed,
                kSharedBytes = layout::kSharedBytes, kCoopBlock = layout::kCoopBlock,
                kCoopGroups = layout::kCoopGroups;
  constexpr size_t kLdsPerCu = layout::kLdsPerCu;
  PlanLayout g{};
  g.H = H;
  g.W = W;
  if (conv_mode == BSGP_CONV_CIRCULAR) {
    g.P = H;
    g.Q = W;
  } else {
    // zero-fill linear convolution on a P x Q circular grid without
    // wrap-around for either kernel (A: kh x kw, AT: kw x kh)
    const int km = kh > kw ? kh : kw;
    int pmin = H + km / 2, qmin = W + km / 2;
    if (pmin < km) pmin = km;
    if (qmin < km) qmin = km;
    g.P = next_fast_len(pmin);
    g.Q = next_fast_len(qmin);
  }
  g.Qh = g.Q / 2 + 1;
  // stored half spectrum: column k at k * sld (even, so row pairs stay 32-B aligned)
  g.sld = H + ((H & 1) ? 1 : 0);
  g.fp.n = g.P;
  g.fq.n = g.Q;
  if (!plan_radices(g.P, g.fp.radix, &g.fp.ns) || !plan_radices(g.Q, g.fq.radix, &g.fq.ns))
    return fail(BSGP_ERR_UNSUPPORTED, "FFT length has too many factors");
  const int maxlen = g.P > g.Q ? g.P : g.Q;
  // one FFT buffer also stages a row pair's stored spectrum (2*Qh, row_inv2); odd spreads banks
  g.lpad = (maxlen + 1 > 2 * g.Qh ? maxlen + 1 : 2 * g.Qh) | 1;
  // LDS: nfw workers x 2 buffers, + reduction scratch
  size_t red_bytes = (size_t)kWaves * kMaxRed * sizeof(double) + kSharedBytes;
  auto need = [&](int n) { return (size_t)n * 2 * g.lpad * sizeof(cd) + red_bytes; };
  auto budget_at = [](int wg) { return kLdsPerCu / wg - 256; };
  // Per-wave transforms (a wave each, kWaves side by side) at four workgroups
  // per CU when the buffers fit that budget (the flagship's 270-point grid, the
  // 31^2 stamps).  Longer ones take three or two workgroups per CU (12 or 8
  // waves) before the cooperative build's 512-thread workgroups, if the twiddle
  // tables fit beside the buffers too: a wave that reads its twiddles from
  // global memory waits on them in every stage (400-point transforms without
  // LDS twiddles took 3.5x the cycles per point of the 270-point ones, phase
  // profile).  With the defaults both application tiles end at two per CU with
  // their twiddles in LDS: 375^2 on the 400-point grid (59264 B of 81664; at
  // three it misses 54357 by the 6400 B table) and 450^2 on the 480-point grid
  // (70784 B).  BSGP_PERWAVE_TW=0 drops the twiddle condition (375^2 then runs
  // three per CU, twiddles from global memory); BSGP_PERWAVE_MIN_WG raises the
  // floor.  Per-wave over cooperative (A/B): 375^2 tiles, 1024 per launch,
  // 68.6 k -> 87.5 k image-it/s; 450^2 48.3 -> 59.7 k.
  size_t budget = budget_at(4);
  g.wg_per_cu = 4;
  const size_t twb = (size_t)(g.P == g.Q ? g.P : g.P + g.Q) * sizeof(cd);
  const size_t tw_need = knobs.perwave_tw ? twb : 0;
  for (int wg = 3; wg >= 2 && wg >= knobs.perwave_min_wg; --wg)
    if (need(kWaves) > budget && need(kWaves) + tw_need <= budget_at(wg)) {
      budget = budget_at(wg);
      g.wg_per_cu = wg;
      break;
    }
  int nfw = kWaves;
  if (need(kWaves) > budget) {
    // transforms too long for a wave each: the whole workgroup runs one
    // transform at a time (cooperative passes)
    g.coop = 1;
    budget = budget_at(1);
    // wave partials of the cooperative build's workgroups (kCoopBlock threads)
    red_bytes = (size_t)(kCoopBlock / 64) * kMaxRed * sizeof(double) + kSharedBytes;
    if (need(1) > budget)
      return fail(BSGP_ERR_UNSUPPORTED, "FFT length too large for one workgroup's LDS");
    // thread groups (bsgp_device.hpp, cooperative passes): as many as the LDS
    // holds, each at least two waves and covering its transform in one load
    // batch (4 elements per thread).  A transform too long for that (C4's 2048
    // points) takes two groups of 256 threads with two load batches
    // (BSGP_COOP_ELEMS, 8 per thread) when the LDS holds both: each workgroup
    // then runs two row pairs through the same stages and barriers, and its
    // radix-8 stages use all 512 lanes instead of 256: C4 k_ls 180 -> 157 us,
    // k_bb 72 -> 68 us, 2114 -> 2221 it/s (float32 storage; f64 1868 -> 1971),
    // the column kernel staying on one group (nfc below).
    auto groups = [&](int el) {
      for (int n = kCoopGroups; n > 1; n /= 2)
        if (need(n) <= budget && kCoopBlock / n >= 128 && maxlen <= el * (kCoopBlock / n))
          return n;
      return 1;
    };
    nfw = groups(4);
    if (nfw == 1 && knobs.coop_elems > 4) nfw = groups(knobs.coop_elems);
    g.wg_per_cu = (int)(budget / need(nfw));
    if (g.wg_per_cu > 4) g.wg_per_cu = 4;
    budget = budget_at(g.wg_per_cu);
  }
  g.nfw = nfw;
  // the column kernel of a cooperative plan keeps one load batch per thread: a
  // 2048-point column per 256-thread group doubled C4's k_col, 42 -> 75 us,
  // while the row passes gained
  int nfc = nfw;
  while (g.coop && nfc > 1 && maxlen > 4 * (kCoopBlock / nfc)) nfc /= 2;
  g.nfc = nfc;
  g.lds_fft_bytes = (size_t)nfw * 2 * g.lpad * sizeof(cd);
  g.lds_bytes = g.lds_fft_bytes + red_bytes;
  g.fp.lds_tw = g.fq.lds_tw = -1;
  g.fp.lds_tw2 = g.fq.lds_tw2 = -1;
  g.tw2 = 0;
  g.twmix = -1;
  if (g.coop) {
    place_coop_tables(&g);
  } else if (g.lds_bytes + twb <= budget) {
    // the per-wave transforms' twiddle tables live in LDS after the reduction
    // scratch when they fit the same budget (one table when P == Q), else the
    // transforms read the global table
    g.fp.lds_tw = (int)g.lds_bytes;
    g.fq.lds_tw = g.P == g.Q ? g.fp.lds_tw : (int)(g.lds_bytes + (size_t)g.P * sizeof(cd));
    g.lds_bytes += twb;
  }
  // slot: gn and bkg in float64 (vec_stride each), the seven iteration vectors
  // in the storage type, then the half spectrum (complex float64), and, last,
  // the second x_tf / pw pair (ImgState::par_tf; slot_bufs finds it from the
  // slot's end)
  g.vec_stride = round_up((size_t)H * W, 32);
  const size_t vbytes = storage == BSGP_STORAGE_F32 ? sizeof(float) : sizeof(double);
  g.spec_off = 2 * g.vec_stride + 7 * g.vec_stride * vbytes / sizeof(double);
  g.slot_stride = g.spec_off + round_up((size_t)g.sld * g.Qh * 2, 32) + 2 * g.vec_stride;
  *out = g;
  return BSGP_OK;
}

// The argument checks bsgp_plan_create and bsgp_plan_layout share.
inline int check_plan_shape(int H, int W, int kh, int kw, int conv_mode, int storage) {
  if (storage != BSGP_STORAGE_F64 && storage != BSGP_STORAGE_F32)
    return fail(BSGP_ERR_ARG, "bad storage");
  if (H < 1 || W < 1 || kh < 1 || kw < 1) return fail(BSGP_ERR_ARG, "bad shape or psf");
  if (conv_mode != BSGP_CONV_CIRCULAR && conv_mode != BSGP_CONV_LINEAR_FILL)
    return fail(BSGP_ERR_ARG, "bad conv_mode");
  if (conv_mode == BSGP_CONV_CIRCULAR && (kh != H || kw != W))
    return fail(BSGP_ERR_ARG,
                "circular A (use_original_SGP_Afunction=True) needs psf.shape == gn.shape");
  return BSGP_OK;
}

// numpy's float32 np.sum over n contiguous elements (numpy 1.26 and 2.x,
// checked against np.sum in tests/test_oracle.py::test_numpy_f32_sum_model):
// the reduction runs over chunks of 8192 (the ufunc buffer), folding
// res = res + pairwise(chunk) from res = 0; pairwise(n) is a leaf for n <= 128
// (8 strided accumulators, or a plain loop below 8) and otherwise
// pairwise(n2) + pairwise(n - n2) with n2 = n/2 - (n/2) % 8.  The program
// lists the leaves (start, length) in order, the inner nodes (value indices
// of the two operands; values 0..L-1 are the leaves, L+k is node k) grouped
// by height so that a level can be added in parallel, and each chunk's root.
struct PwBuild {
  std::vector<int> leaves, nodes_tmp, heights, roots;
  // returns a temporary id: >= 0 leaf, < 0 node -(k+1); *h = height
  int rec(int start, int n, int* h) {
    if (n <= 128) {
      leaves.push_back(start);
      leaves.push_back(n);
      *h = 0;
      return (int)leaves.size() / 2 - 1;
    }
    int n2 = n / 2;
    n2 -= n2 % 8;
    int ha, hb;
    const int a = rec(start, n2, &ha);
    const int b = rec(start + n2, n - n2, &hb);
    nodes_tmp.push_back(a);
    nodes_tmp.push_back(b);
    *h = (ha > hb ? ha : hb) + 1;
    heights.push_back(*h);
    return -(int)(nodes_tmp.size() / 2);
  }
};

// counts = {nleaf, nnode, nlev, nchunk} (PwProg's fields, bsgp_internal.hpp)
inline std::vector<int> pairwise_program(long n, int counts[4]) {
  PwBuild b;
  std::vector<int> root_tmp;
  for (long c0 = 0; c0 < n; c0 += 8192) {
    int h;
    root_tmp.push_back(b.rec((int)c0, (int)std::min<long>(8192, n - c0), &h));
  }
  const int L = (int)b.leaves.size() / 2, M = (int)b.heights.size();
  int maxh = 0;
  for (int v : b.heights) maxh = std::max(maxh, v);
  // order the nodes by height (stable), then renumber the operands
  std::vector<int> order, newid(M), lev_off(maxh + 1, 0);
  for (int h = 1; h <= maxh; ++h) {
    lev_off[h - 1] = (int)order.size();
    for (int k = 0; k < M; ++k)
      if (b.heights[k] == h) order.push_back(k);
  }
  lev_off[maxh] = (int)order.size();
  for (int i = 0; i < M; ++i) newid[order[i]] = L + i;
  auto val = [&](int t) { return t >= 0 ? t : newid[-t - 1]; };
  std::vector<int> prog(b.leaves);
  for (int i = 0; i < M; ++i) {
    prog.push_back(val(b.nodes_tmp[2 * order[i]]));
    prog.push_back(val(b.nodes_tmp[2 * order[i] + 1]));
  }
  for (int v : lev_off) prog.push_back(v);
  for (int t : root_tmp) prog.push_back(val(t));
  counts[0] = L;
  counts[1] = M;
  counts[2] = maxh;
  counts[3] = (int)root_tmp.size();
  return prog;
}

}  // namespace bsgp
