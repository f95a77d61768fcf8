// Host-side unit test of the plan layout and numpy's float32 reduction program
// (beta-sgp_amd/csrc/bsgp_layout.hpp), which need no device.  Sweeps image
// sizes through every regime (per-wave at 4, 3 and 2 workgroups per CU,
// cooperative with 4, 2 and 1 thread groups, the LDS limit) and checks the
// layout's invariants; checks the flagship plan against SGeo256's constants;
// evaluates the reduction program of several lengths on integers.
// Build+run: g++ -O2 -std=c++17 -I beta-sgp_amd/csrc tests/cpp/plan_layout_test.cpp && ./a.out
#include <cstdio>
#include <cstring>
#include <vector>

#include "bsgp_layout.hpp"
using namespace bsgp;

static int bad = 0;
#define CHECK(cond, ...)                     \
  do {                                       \
    if (!(cond)) {                           \
      printf("FAIL %s: ", #cond);            \
      printf(__VA_ARGS__);                   \
      printf("\n");                          \
      bad++;                                 \
    }                                        \
  } while (0)

static void check_layout(int H, int W, int kh, int kw, int mode, int storage, const PlanKnobs& k,
                         int* regimes) {
  PlanLayout l;
  const int rc = plan_layout(H, W, kh, kw, mode, storage, k, &l);
  if (rc != BSGP_OK) {
    CHECK(rc == BSGP_ERR_UNSUPPORTED && !g_err.empty(), "H=%d W=%d rc=%d", H, W, rc);
    regimes[0]++;
    return;
  }
  regimes[l.coop ? 4 + l.nfw : l.wg_per_cu]++;
  CHECK(l.lds_bytes <= layout::kLdsPerCu / l.wg_per_cu - 256, "H=%d W=%d lds=%zu wg=%d", H, W,
        l.lds_bytes, l.wg_per_cu);
  CHECK(l.wg_per_cu >= 1 && l.wg_per_cu <= 4, "H=%d wg=%d", H, l.wg_per_cu);
  CHECK(l.nfc >= 1 && l.nfc <= l.nfw, "H=%d nfc=%d nfw=%d", H, l.nfc, l.nfw);
  CHECK(l.coop || (l.nfw == 4 && l.nfc == 4), "H=%d nfw=%d", H, l.nfw);
  CHECK(l.sld % 2 == 0 && l.sld >= H && l.sld <= H + 1, "H=%d sld=%d", H, l.sld);
  CHECK(l.P >= H && l.Q >= W && l.Qh == l.Q / 2 + 1, "H=%d P=%d Q=%d", H, l.P, l.Q);
  CHECK(l.lpad % 2 == 1 && l.lpad > l.P && l.lpad > l.Q && l.lpad >= 2 * l.Qh, "H=%d lpad=%d", H,
        l.lpad);
  CHECK(l.lds_fft_bytes == (size_t)l.nfw * 2 * l.lpad * 16 && l.lds_fft_bytes < l.lds_bytes,
        "H=%d fft=%zu", H, l.lds_fft_bytes);
  // (seven float32 vectors are 3.5 float64 ones: a multiple of 16 doubles)
  const size_t al = storage == BSGP_STORAGE_F32 ? 16 : 32;
  CHECK(l.slot_stride % al == 0 && l.vec_stride % 32 == 0 && l.spec_off % al == 0 &&
            l.vec_stride >= (size_t)H * W,
        "H=%d slot=%zu", H, l.slot_stride);
  CHECK(l.slot_stride >= l.spec_off + (size_t)l.sld * l.Qh * 2 + 2 * l.vec_stride, "H=%d", H);
  // LDS twiddles: inside the allocation, after the buffers, never for cooperative plans
  for (const FftPlan* f : {&l.fp, &l.fq}) {
    long prod = 1;
    for (int i = 0; i < f->ns; ++i) prod *= f->radix[i];
    CHECK(prod == f->n && f->tw == nullptr, "H=%d n=%d", H, f->n);
    CHECK(f->lds_tw == -1 || (!l.coop && (size_t)f->lds_tw >= l.lds_fft_bytes &&
                              (size_t)f->lds_tw + (size_t)f->n * 16 <= l.lds_bytes),
          "H=%d lds_tw=%d", H, f->lds_tw);
    CHECK(f->lds_tw2 == -1 || (l.coop && f->n == 2048 && f->lds_tw2 + 96 * 16 <= l.tw2),
          "H=%d lds_tw2=%d", H, f->lds_tw2);
  }
  CHECK(l.twmix == -1 || (l.P == 2048 && l.twmix + 576 * 16 <= l.tw2), "H=%d twmix=%d", H, l.twmix);
}

// the program's sum of 1, 2, ..., n in integers: every element exactly once
static void check_pairwise(long n) {
  int c[4];
  const std::vector<int> prog = pairwise_program(n, c);
  const int L = c[0], M = c[1], nlev = c[2], nchunk = c[3];
  CHECK((long)prog.size() == 2L * L + 2L * M + nlev + 1 + nchunk, "n=%ld size=%zu", n, prog.size());
  CHECK(nchunk == (n + 8191) / 8192, "n=%ld nchunk=%d", n, nchunk);
  std::vector<long long> val(L + M, 0);
  long next = 0;
  for (int i = 0; i < L; ++i) {
    const int start = prog[2 * i], len = prog[2 * i + 1];
    CHECK(start == next && len >= 1 && len <= 128, "n=%ld leaf %d", n, i);
    next = start + len;
    for (int k = 0; k < len; ++k) val[i] += start + k + 1;
  }
  CHECK(next == n, "n=%ld leaves end at %ld", n, next);
  const int* nd = prog.data() + 2 * L;
  const int* off = nd + 2 * M;
  CHECK(off[0] == 0 && off[nlev] == M, "n=%ld levels", n);
  for (int lev = 0; lev < nlev; ++lev)
    for (int k = off[lev]; k < off[lev + 1]; ++k) {
      // a level's operands are leaves or nodes of lower levels
      CHECK(nd[2 * k] < L + off[lev] && nd[2 * k + 1] < L + off[lev], "n=%ld node %d", n, k);
      val[L + k] = val[nd[2 * k]] + val[nd[2 * k + 1]];
    }
  long long total = 0;
  const int* root = off + nlev + 1;
  for (int i = 0; i < nchunk; ++i) total += val[root[i]];
  CHECK(total == (long long)n * (n + 1) / 2, "n=%ld total=%lld", n, total);
}

int main() {
  const PlanKnobs def{2, 1, 8};
  int regimes[9] = {};
  const int big[] = {500, 600, 800, 1000, 1012, 1013, 1100, 1500, 2000, 2014, 2030, 2036, 2037,
                     2100, 3000, 4000, 4300, 5000};
  for (int storage : {BSGP_STORAGE_F64, BSGP_STORAGE_F32}) {
    for (int H = 16; H <= 480; ++H) check_layout(H, H, 25, 25, BSGP_CONV_LINEAR_FILL, storage, def, regimes);
    for (int H : big) {
      check_layout(H, H, 25, 25, BSGP_CONV_LINEAR_FILL, storage, def, regimes);
      check_layout(H, 300, 25, 25, BSGP_CONV_LINEAR_FILL, storage, def, regimes);
      check_layout(300, H, 25, 25, BSGP_CONV_LINEAR_FILL, storage, def, regimes);
    }
    for (int H : {16, 31, 64, 256, 270, 512, 2048})
      check_layout(H, H, H, H, BSGP_CONV_CIRCULAR, storage, def, regimes);
  }
  // every regime was met: unsupported, per-wave at 2 and 4 per CU, cooperative
  // with 1 and 2 groups (three per CU and four groups need the knobs, below)
  for (int r : {0, 2, 4, 5, 6}) CHECK(regimes[r] > 0, "regime %d never met", r);
  int knob_regimes[9] = {};
  for (int H = 16; H <= 2100; H += 7) {
    check_layout(H, H, 25, 25, BSGP_CONV_LINEAR_FILL, 0, PlanKnobs{2, 0, 8}, knob_regimes);
    check_layout(H, H, 25, 25, BSGP_CONV_LINEAR_FILL, 0, PlanKnobs{4, 1, 4}, knob_regimes);
    check_layout(H, H, 25, 25, BSGP_CONV_LINEAR_FILL, 0, PlanKnobs{3, 1, 8}, knob_regimes);
  }
  CHECK(knob_regimes[3] > 0 && knob_regimes[8] > 0, "three per CU / four groups never met");

  // the flagship plan is SGeo256 (bsgp_device.hpp): its constants, as literals
  PlanLayout l;
  CHECK(plan_layout(256, 256, 25, 25, BSGP_CONV_LINEAR_FILL, BSGP_STORAGE_F64, def, &l) == BSGP_OK,
        "flagship");
  CHECK(l.P == 270 && l.Q == 270 && l.Qh == 136 && l.sld == 256 && l.lpad == 273 && l.nfw == 4 &&
            l.nfc == 4 && l.coop == 0 && l.tw2 == 0 && l.twmix == -1 &&
            l.lds_fft_bytes == 34944 && l.fp.lds_tw == 36224 && l.fq.lds_tw == 36224 &&
            l.lds_bytes == 40544 && l.wg_per_cu == 4,
        "flagship layout");
  CHECK(plan_layout(5000, 5000, 25, 25, BSGP_CONV_LINEAR_FILL, 0, def, &l) == BSGP_ERR_UNSUPPORTED &&
            g_err == "FFT length too large for one workgroup's LDS",
        "LDS limit: %s", g_err.c_str());

  for (long n : {1L, 7L, 8L, 128L, 129L, 961L, 8192L, 8193L, 65536L, 140625L, 202500L})
    check_pairwise(n);

  if (bad) {
    printf("%d checks failed\n", bad);
    return 1;
  }
  printf("all ok\n");
  return 0;
}
