// bsgp_internal.hpp — what the solver's kernel units (bsgp_solver*.hip,
// bsgp_persist*.hip, bsgp_state.hip) share with the C-ABI host layer
// (bsgp_plan.hip, bsgp_solve.hip, bsgp_apps.hip): the per-image state, the
// solve's argument block and launchers, the state records, and the projection
// and divergence launchers of bsgp_solver.hip.  The application stages' blocks
// are bsgp_apps.hpp's.  Not part of the public interface.
#pragma once

#include <hip/hip_runtime.h>

#include <vector>

#include "../../include/bsgp.h"
#include "bsgp_device.hpp"

namespace bsgp {

// Per-image solver state carried between the phase kernels (device memory).
struct ImgState {
  int par, Xones, stop, iter, epoch;
  int bar_base;  // team barriers completed before the next kernel (T > 1)
  int64_t E_p, E_ls, ls_passes, status, ls_series;
  int64_t proj_passes, proj_list;  // projection passes over the image / list entries read
  double sc, flux, bks_scalar, lo, hi, Dcoeff, tol, t0;
  double fv, alpha, tau, lr, init_lr, beta, lam_p, gd, lam;
  // projection history for the first pass's split bracket (cached_projection):
  // the last multiplier over the step length it was found at, and the last
  // search's first secant point over its root (0: none yet)
  double lam_ratio, kappa;
  double konst;  // lambda-independent objective sum at `beta` (sum s*gn^b / sum gn)
  // compact observed image (params.gn_compact): 0 = gn_s stored in f64; 1 = the
  // raw counts stored in f32, gn_s = raw (scale_data 0/2); 2 = gn_s = raw / sc.
  // gfill is the null-pixel value vmin*eps^2 (sgp.py:202-204).
  int g32;
  // which of the two x_tf / pw buffer pairs is current (slot_bufs): a line
  // search that accepts its speculative fused pass (ls_phase) flips it.  It
  // fills the padding before gfill.
  int par_tf;
  // this iteration's line search accepted its speculative pass: w's spectrum is
  // the speculation buffer's (SolveArgs::spec2), not the slot's.  ls_phase
  // writes it every iteration, bb_phase reads it; nothing carries it across an
  // iteration boundary (dir_phase always writes the slot's spectrum).
  int par_spec;
  double gfill;
  double Valpha[32];
  double Fold[32];
};

// Everything a phase kernel needs (passed by value: kernel-argument loads are
// scalar, so plan geometry and pointers stay in SGPRs).
// One-workgroup images run AT's column pass at the end of k_ls instead of as
// a k_col launch (SolveArgs::fuse_col; measured on C3, A/B: +4.5 %).  A's
// column pass stays a k_col launch: fused into k_dir it cost 25 % (252 VGPRs +
// scratch: the projection state stays live), at the start of k_ls 1 % (spills
// at 168 VGPRs).  Teams launch k_col for both.

// numpy float32 reduction program of a plan's N (bsgp_layout.hpp pairwise_program):
// [nleaf][2] leaves (start, len), [nnode][2] node operands (value indices),
// [nlev + 1] level offsets into the nodes, [nchunk] root value of each chunk.
struct PwProg {
  const int* prog;
  int nleaf, nnode, nlev, nchunk;
};

struct SolveArgs {
  Geo g;
  bsgp_params prm;
  bsgp_inputs in;
  bsgp_outputs out;
  int B;
  int img0, nimg;      // this launch's sub-batch [img0, img0 + nimg)
  ImgState* st;        // [B]
  int* active;         // images not yet stopped: B at the start (the host sets it); the setup
                       // and k_bb count each stopping image down
  int* done_host;      // host-mapped word: the solve's `seq` once `active` reaches 0 (the
                       // host's lookahead polling of data-dependent stop rules), or nullptr
  int seq;             // this solve's sequence number (done_host)
  double* ws;          // per-image slots
  size_t slot_stride;  // doubles per slot
  size_t vec_stride;   // doubles per image vector (N rounded up to 32)
  size_t lds_fft_bytes;
  // teams (T workgroups per image; T = 1: one workgroup, none of these used)
  int T;
  int Tc;               // workgroups per image of k_col (no reductions there: not a team)
  int fuse_col;         // bit 1: AT's column pass runs at the end of k_ls (T == 1: 2, teams: 0)
  int static_geo;       // persistent solver: the plan is SGeo256's and the kernel carries the
                        // compile-time-geometry phases, which run (persist_static_geo; the
                        // word fills the padding before tpart: no offset moves)
  double* tpart;        // [B][kPartBufs][T][kMaxRed] reduction partials
  unsigned int* tctr;   // [B][kTeamWords] barrier words, then the timeout word; zeroed per solve
  int* tfail;           // set by a timed-out barrier spin
  // projection pixel lists (proj_cache): per image two arrays (y, X) of
  // lcap * T * kBlock doubles; entry k of global thread gt at k*T*kBlock + gt
  double* plist;
  size_t plist_stride;  // doubles per image (both arrays)
  int lcap;             // list capacity per thread (pixels one thread streams)
  int list_lds;         // list entries per thread kept in the transform buffers' LDS (teams and
                        // one-workgroup images of per-wave plans; BSGP_LIST_LDS caps the latter)
  PwProg pw;            // numpy float32 sum order over N (params.gn_f32)
  int storage;          // BSGP_STORAGE_F64 / F32 (iteration vectors, Bufs<V>)
  size_t spec_off;      // doubles from a slot's start to its spectrum
  int ls_cap;           // line-search trial cap: lam = beta^(k-1) < 1e-12 ends the search
                        // (sgp.py:336) by trial ceil(log 1e-12 / log beta) + 1 for 0 < beta < 1
  unsigned spin_limit;  // persistent solver: s_sleep polls before a hand-off wait gives up
                        // (status bit 4); 2^26 unless BSGP_SPIN_LIMIT says otherwise (tests)
  int fold_setup;       // persistent solver, slot order: every image's setup is the first
                        // task of its chain inside k_persist (no k_setup launch)
  int ls_predict;       // persistent solver's line search: pass 1 does only what the predicted
                        // outcome needs (ls_phase).  0: never; 1 (default): an accept after an
                        // accepted lam = 1; 2 / 3: always an accept / a stagnation (tests);
                        // 4: as 1, and a stagnation after a tiny step; 5: stagnations only
                        // (both measured slower than 1 on C3).  BSGP_LS_PREDICT
  // second half spectrum per image for the speculative fused pass (ls_phase:
  // it reads A(d)'s rows from the slot's spectrum and writes w's rows here, so
  // a missed speculation finds A(d) intact).  The plan allocates it for solves
  // that can speculate (persistent, per-wave float64, fixed general beta with
  // the series, ls_predict != 0); nullptr otherwise: no speculation.
  cd* spec2;
  size_t spec2_stride;  // complex values per image
};

hipError_t launch_setup(const SolveArgs& a, size_t lds, hipStream_t s);
// ev: NULL, or 6 events recorded around the kernels of one iteration (profiled solves)
hipError_t launch_iteration(const SolveArgs& a, int K, size_t lds, hipStream_t s,
                            hipEvent_t* ev = nullptr);
hipError_t launch_track(const SolveArgs& a, int it, hipStream_t s);
hipError_t launch_build_tf(const Geo& g, const double* kc, cd* spec, cd* tf, double scale,
                           int conj, size_t lds, hipStream_t s);
hipError_t launch_build_tfs(const Geo& g, int n, const double* kc, size_t kc_stride, cd* spec,
                            size_t spec_stride, cd* tf, size_t tf_stride, double scale, int conj,
                            size_t lds, hipStream_t s);
hipError_t launch_place_psfs(const Geo& g, int n, const double* psfs, int kh, int kw, int circ,
                             double* kc, double* sums, hipStream_t s);
hipError_t launch_apply_op(const Geo& g, int B, int transpose, const double* x, double* out,
                           cd* specws, size_t spec_stride, int grid, size_t lds, hipStream_t s);
hipError_t launch_apply_op_split(const Geo& g, int B, int transpose, const double* x,
                                 double* out, cd* specws, size_t spec_stride, int per, size_t lds,
                                 hipStream_t s);
hipError_t launch_project_df(int n, double b, const double* c, const double* dia, ProjClip clip,
                             double lam0, double dlam0, double tol_lam, int biter, int siter,
                             int max_projs, double* x, double* info, hipStream_t s);
hipError_t launch_beta_div(int n, const double* y, const double* x, double beta, double* out,
                           hipStream_t s);
hipError_t launch_beta_div_deriv(int64_t n, const double* y, const double* x, double beta,
                                 double* out, hipStream_t s);
hipError_t launch_grad_parts(int64_t n, const double* den, const double* gn, double beta,
                             double* pow1, double* w, hipStream_t s);
hipError_t set_solver_lds_limit(size_t bytes);
// workgroups of every team kernel of a build (coop, storage) one CU holds at once
hipError_t team_resident_per_cu(bool coop, int storage, size_t lds, int* per_cu);
hipError_t phase_prof(unsigned long long* out, int n, int reset);
// persistent task-queue solver (bsgp_persist.hip): one launch runs every
// iteration of every image; queue = dequeue counter, done[B] = iterations
// published per image (both zeroed per solve)
hipError_t launch_persist(const SolveArgs& a, int K, size_t lds, hipStream_t s, unsigned* queue,
                          unsigned* done, int grid);
hipError_t persist_resident_per_cu(const SolveArgs& a, int K, size_t lds, int* per_cu);
// whether the persistent kernel this solve launches has static-geometry phases
// for the plan's geometry (SolveArgs::static_geo may then be set)
bool persist_static_geo(const SolveArgs& a, int K);
// whether a persistent solve can take the speculative fused pass (needs SolveArgs::spec2)
bool persist_speculates(const SolveArgs& a);
hipError_t persist_phase_prof(unsigned long long* out, int n, int reset);
void persist_kernels_all(std::vector<const void*>& f);

// ---- solver state records (bsgp_state.hip; layout in include/bsgp.h) -------
static_assert(sizeof(bsgp_state_header) <= BSGP_STATE_HEADER_BYTES, "state header overflows");

// Byte offsets of a record's sections (bsgp_state_layout's offs[]).
struct StateLayout {
  size_t bytes, discr, crit, times, flags, x, g, xtf, pw, gn, bkg;
};
inline size_t state_pad16(size_t v) { return (v + 15) / 16 * 16; }
inline StateLayout state_layout(size_t N, int storage, bool bmap, int hist_cap) {
  const size_t vb = storage == BSGP_STORAGE_F32 ? 4 : 8;
  StateLayout L{};
  size_t o = BSGP_STATE_HEADER_BYTES;
  auto take = [&](size_t n) {
    const size_t at = o;
    o += state_pad16(n);
    return at;
  };
  L.discr = take((size_t)hist_cap * 8);
  L.crit = take((size_t)hist_cap * 8);
  L.times = take((size_t)hist_cap * 8);
  L.flags = take((size_t)hist_cap * 4);
  L.x = take(N * vb);
  L.g = take(N * vb);
  L.xtf = take(N * vb);
  L.pw = take(N * vb);
  L.gn = take(N * 8);
  L.bkg = bmap ? take(N * 8) : 0;
  L.bytes = o;
  return L;
}

// Arguments of k_state_save / k_state_load (by value: scalar loads).
struct StateArgs {
  unsigned char* rec;   // [B or n_state] records
  size_t rec_bytes;     // bytes per record
  const int* index;     // load: record of image i (nullptr: record i)
  StateLayout L;
  double* ws;           // the plan's slots (SolveArgs::ws / slot_stride / vec_stride)
  size_t slot_stride, vec_stride;
  ImgState* st;
  int N, storage, bmap, hist_cap, T, conv_mode, H, W, beta0_given;
  int M1;               // rows of the out arrays (MAXIT + 1 of the solve they belong to)
  bsgp_outputs out;     // save: the finished solve's outputs; load: the resumed solve's
  bsgp_params prm;      // save: the finished solve's parameters
  int* active;          // load: counts the images that go on
};
hipError_t launch_state_save(const StateArgs& a, int B, hipStream_t s);
hipError_t launch_state_load(const StateArgs& a, int B, hipStream_t s);
// after k_state_load: seeds the persistent solver's slot order at iteration
// `done_it` (queue == nullptr: no seeding) and, when no image goes on, tells the
// host's lookahead poll so (done_host = seq)
hipError_t launch_state_post(const StateArgs& a, int B, unsigned* queue, unsigned* done,
                             int done_it, int* done_host, int seq, hipStream_t s);

// Cooperative plans (Geo::coop) run the phase kernels of bsgp_solver_c512.hip:
// the same kernels with 512-thread workgroups (two waves per SIMD per
// workgroup where a long transform's LDS allows one or two workgroups per CU).
// At most this many thread groups per workgroup run a cooperative plan's
// transforms side by side (bsgp_device.hpp coop passes).
constexpr int kCoopGroups = 4;
constexpr int kCoopBlock = 512;
// threads per workgroup of a plan's phase kernels
__host__ __device__ inline int plan_block(const Geo& g) { return g.coop ? kCoopBlock : kBlock; }
// plans whose persistent solve runs the application-size build (bsgp_persist_app.hip):
// per-wave, float64 storage, a 400- or 480-point row or column transform
inline bool app_static_plan(const Geo& g, int storage) {
  const bool app_n = g.fp.n == 400 || g.fp.n == 480 || g.fq.n == 400 || g.fq.n == 480;
  return !g.coop && storage == BSGP_STORAGE_F64 && app_n;
}

}  // namespace bsgp

// bsgp_solver_c512.hip (C linkage: its types live in namespace bsgp_c512; the
// argument block is this header's SolveArgs, same layout)
extern "C" {
size_t bsgp_c512_args_size(void);
int bsgp_c512_block(void);
int bsgp_c512_waves(void);
hipError_t bsgp_c512_launch_setup(const void* a, size_t lds, hipStream_t s);
hipError_t bsgp_c512_launch_iteration(const void* a, int K, size_t lds, hipStream_t s,
                                      hipEvent_t* ev);
hipError_t bsgp_c512_team_resident(int storage, size_t lds, int* per_cu);
hipError_t bsgp_c512_set_lds_limit(size_t bytes);
// the cooperative plans' persistent solver (bsgp_persist_c512.hip)
hipError_t bsgp_c512_launch_persist(const void* a, int K, size_t lds, hipStream_t s,
                                    unsigned* queue, unsigned* done, int grid);
hipError_t bsgp_c512_persist_resident(const void* a, int K, size_t lds, int* per_cu);
hipError_t bsgp_c512_persist_set_lds_limit(size_t bytes);
// the application-size persistent build (bsgp_persist_app.hip): per-wave plans
// of float64 storage whose row or column transform has 400 or 480 points
size_t bsgp_app_args_size(void);
hipError_t bsgp_app_launch_persist(const void* a, int K, size_t lds, hipStream_t s,
                                   unsigned* queue, unsigned* done, int grid);
hipError_t bsgp_app_persist_resident(const void* a, int K, size_t lds, int* per_cu);
hipError_t bsgp_app_persist_set_lds_limit(size_t bytes);
hipError_t bsgp_app_phase_prof(unsigned long long* out, int n, int reset);
hipError_t bsgp_c512_phase_prof(unsigned long long* out, int n, int reset);
}
