// bsgp_state.hip — solver-state records: gather the state a finished solve left
// in the plan's slots and ImgState into compact per-image records
// (k_state_save), and scatter records back into the slots of a plan so the
// iteration loop can go on without the setup (k_state_load).  Record layout:
// include/bsgp.h (bsgp_state_header, bsgp_state_layout); DESIGN §3.6.
//
// Both kernels are data movement: the vectors go as 16-byte chunks over a grid
// of (chunk range, image) workgroups, kStU chunks in flight per thread; the
// header, the scalars and the history rows go through the first workgroup of
// each image.  The slot layout is slot_bufs' (bsgp_kernels.hpp): gn and the
// background map in float64 at 0 and vec_stride, then x0, x1, g0, g1, x_tf,
// d_tf, pw in the storage type; after the spectrum the second x_tf / pw pair
// (a record holds the current pair, a load fills the first).
#include <hip/hip_runtime.h>

#include "bsgp_internal.hpp"

namespace bsgp {

namespace {

constexpr int kStBlock = 256;
constexpr int kStU = 4;  // 16-byte chunks in flight per thread
// k_persist's slot order marks a stopped image in done[] with this bit
// (kDoneStop, bsgp_kernels.hpp)
constexpr unsigned kSeedDoneStop = 0x40000000u;

__device__ __forceinline__ double st_now() {
  return (double)__builtin_amdgcn_s_memrealtime() * 1e-8;  // realtime_s of the phase kernels
}

// Vector sections of a record, in chunk order: 0 x, 1 g, 2 x_tf, 3 pw (nV
// chunks each), 4 gn, 5 bkg (nD chunks each).
__device__ __forceinline__ void st_locate(unsigned c, unsigned nV, unsigned nD, int& s,
                                          unsigned& k) {
  if (c < 4 * nV) {
    s = (int)(c / nV);
    k = c - (unsigned)s * nV;
  } else {
    c -= 4 * nV;
    s = c >= nD ? 5 : 4;
    k = s == 5 ? c - nD : c;
  }
}
__device__ __forceinline__ size_t st_rec_off(const StateLayout& L, int s) {
  return s == 0 ? L.x : s == 1 ? L.g : s == 2 ? L.xtf : s == 3 ? L.pw : s == 4 ? L.gn : L.bkg;
}
// byte offset of a section's vector inside a slot; buf picks x0/g0 or x1/g1,
// ptf the first x_tf / pw pair or the second (ImgState::par_tf: the slot's
// last two vectors)
__device__ __forceinline__ size_t st_slot_off(const StateArgs& S, int s, int buf, int ptf = 0) {
  const size_t v = S.vec_stride, vb = S.storage == BSGP_STORAGE_F32 ? 4 : 8;
  const size_t base = 2 * v * 8;
  const size_t spare = (S.slot_stride - 2 * v) * 8;
  return s == 0   ? base + (size_t)buf * v * vb
         : s == 1 ? base + (size_t)(2 + buf) * v * vb
         : s == 2 ? (ptf ? spare : base + 4 * v * vb)
         : s == 3 ? (ptf ? spare + v * vb : base + 6 * v * vb)
         : s == 4 ? 0
                  : v * 8;
}
// bytes of a section's N elements
__device__ __forceinline__ unsigned st_sec_bytes(const StateArgs& S, int s) {
  return (unsigned)S.N * (s < 4 && S.storage == BSGP_STORAGE_F32 ? 4u : 8u);
}
// chunk k of a section of nb bytes: the words past the section's end are 0
__device__ __forceinline__ uint4 st_mask(uint4 w, unsigned nb, unsigned k) {
  const unsigned valid = nb - 16u * k;  // >= 4, a multiple of 4
  if (valid < 16u) w.w = 0u;
  if (valid < 12u) w.z = 0u;
  if (valid < 8u) w.y = 0u;
  return w;
}

// Why an image of a finished solve is stopped: 0 it ran out of MAXIT only (it
// goes on when resumed), 1 a stop rule fired (bb_phase's rules, re-evaluated
// from the state they were evaluated from: bb_phase changes neither fv nor
// Fold) or a hand-off timed out, 8 the setup stopped it.
__device__ __forceinline__ int st_final(const StateArgs& S, int img, const ImgState& st) {
  if (!st.stop) return 0;
  if (st.status & 8) return 8;
  if (st.status & 4) return 1;
  const bsgp_params& P = S.prm;
  if (st.iter <= P.MAXIT) return 1;
  bool loop = true;
  if (P.stop_criterion == 2) {
    const double crit = S.out.crit[(size_t)img * S.M1 + st.iter - 1];  // (the host requires crit)
    loop = crit > st.tol;
  } else if (P.stop_criterion == 3) {
    const double crit = (st.Fold[P.M - 1] - st.fv) / st.fv;
    loop = crit > st.tol && crit >= 0;
  } else if (P.stop_criterion == 4) {
    loop = st.Dcoeff * st.fv > st.tol;
  }
  return loop ? 0 : 1;
}

}  // namespace

// ------------------------------------------------------------ kernel: save
// Grid (chunk ranges, B).  The iterate after the last completed iteration: an
// image that stopped for MAXIT alone wrote it to xb / gb and left `par` as it
// was (bb_phase); an image a stop rule stopped returns xa (sgp.py:424-438).
__global__ void __launch_bounds__(kStBlock) k_state_save(StateArgs S) {
  const int img = (int)blockIdx.y;
  const int tid = (int)threadIdx.x;
  const ImgState& st = S.st[img];
  unsigned char* rec = S.rec + (size_t)img * S.rec_bytes;
  const unsigned char* slot =
      reinterpret_cast<const unsigned char*>(S.ws + (size_t)img * S.slot_stride);
  const int fin = st_final(S, img, st);
  const int buf = (st.stop && fin == 0) ? (st.par ^ 1) : st.par;
  const unsigned vb = S.storage == BSGP_STORAGE_F32 ? 4u : 8u;
  const unsigned nV = ((unsigned)S.N * vb + 15u) / 16u, nD = ((unsigned)S.N * 8u + 15u) / 16u;
  const unsigned total = 4u * nV + (S.bmap ? 2u : 1u) * nD;
  const bool no_pw = S.prm.variant != BSGP_VARIANT_BETA;  // KL never writes pw
  for (unsigned c0 = blockIdx.x * (unsigned)(kStBlock * kStU) + (unsigned)tid; c0 < total;
       c0 += gridDim.x * (unsigned)(kStBlock * kStU)) {
    uint4 w[kStU];
#pragma unroll
    for (int u = 0; u < kStU; ++u) {
      const unsigned c = c0 + (unsigned)(u * kStBlock);
      int s;
      unsigned k;
      st_locate(c < total ? c : total - 1u, nV, nD, s, k);
      w[u] = *reinterpret_cast<const uint4*>(slot + st_slot_off(S, s, buf, st.par_tf) + (size_t)k * 16);
    }
#pragma unroll
    for (int u = 0; u < kStU; ++u) {
      const unsigned c = c0 + (unsigned)(u * kStBlock);
      if (c >= total) continue;
      int s;
      unsigned k;
      st_locate(c, nV, nD, s, k);
      uint4 v = st_mask(w[u], st_sec_bytes(S, s), k);
      if (s == 3 && no_pw) v = uint4{0u, 0u, 0u, 0u};
      *reinterpret_cast<uint4*>(rec + st_rec_off(S.L, s) + (size_t)k * 16) = v;
    }
  }
  if (blockIdx.x != 0) return;
  // header, scalars and history: the image's first workgroup
  bsgp_state_header* h = reinterpret_cast<bsgp_state_header*>(rec);
  const int done = st.iter - 1;
  const size_t row = (size_t)img * S.M1;
  double* hd = reinterpret_cast<double*>(rec + S.L.discr);
  double* hc = reinterpret_cast<double*>(rec + S.L.crit);
  double* ht = reinterpret_cast<double*>(rec + S.L.times);
  int* hf = reinterpret_cast<int*>(rec + S.L.flags);
  const int cap2 = (S.hist_cap + 1) & ~1;  // the sections' zero padding (16 bytes: 2 rows)
  for (int k = tid; k < cap2; k += kStBlock) {
    const bool in = k <= done && k < S.M1 && k < S.hist_cap;
    hd[k] = in ? S.out.discr[row + k] : 0.0;
    hc[k] = (in && S.out.crit) ? S.out.crit[row + k] : 0.0;
    ht[k] = (in && S.out.times) ? S.out.times[row + k] : 0.0;
  }
  const int cap4 = (S.hist_cap + 3) & ~3;
  for (int k = tid; k < cap4; k += kStBlock)
    hf[k] = (k <= done && k < S.M1 && k < S.hist_cap && S.out.flags) ? S.out.flags[row + k] : 0;
  if (tid < 32) {
    h->Valpha[tid] = tid < S.prm.M_alpha ? st.Valpha[tid] : 0.0;
    h->Fold[tid] = tid < S.prm.M ? st.Fold[tid] : 0.0;
  }
  // zero padding of the header block
  for (int i = (int)sizeof(bsgp_state_header) / 4 + tid; i < BSGP_STATE_HEADER_BYTES / 4;
       i += kStBlock)
    reinterpret_cast<unsigned*>(rec)[i] = 0u;
  if (tid == 0) {
    h->magic = BSGP_STATE_MAGIC;
    h->version = BSGP_STATE_VERSION;
    h->H = S.H;
    h->W = S.W;
    h->storage = S.storage;
    h->conv_mode = S.conv_mode;
    h->hist_cap = S.hist_cap;
    h->T = S.T;
    h->iters_done = done;
    h->stopped = fin;
    // (an image that stopped for MAXIT alone completed an iteration: bb_phase
    // clears Xones only when it goes on, so the running form clears it here)
    h->Xones = (st.stop && fin == 0) ? 0 : st.Xones;
    h->epoch = st.epoch;
    h->g32 = st.g32;
    h->beta0_given = S.beta0_given;
    h->record_bytes = (int64_t)S.rec_bytes;
    h->counters[0] = st.E_p;
    h->counters[1] = st.E_ls;
    h->counters[2] = st.ls_passes;
    h->counters[3] = st.status;
    h->counters[4] = st.ls_series;
    h->counters[5] = st.proj_passes;
    h->counters[6] = st.proj_list;
    h->scaling = st.sc;
    h->flux = st.flux;
    h->bkg_scalar = st.bks_scalar;
    h->x_low = st.lo;
    h->x_upp = st.hi;
    h->Dcoeff = st.Dcoeff;
    h->tol = st.tol;
    h->elapsed = (S.out.times && done < S.M1) ? S.out.times[row + done] : 0.0;
    h->fv = st.fv;
    h->alpha = st.alpha;
    h->tau = st.tau;
    h->lr = st.lr;
    h->init_lr = st.init_lr;
    h->beta = st.beta;
    h->lam_p = st.lam_p;
    h->lam_ratio = st.lam_ratio;
    h->kappa = st.kappa;
    h->konst = st.konst;
    h->gfill = st.gfill;
    h->prm = S.prm;
  }
}

// ------------------------------------------------------------ kernel: load
// Grid (chunk ranges, B): image i of the resumed batch takes record index[i].
// Every image enters in "running" form, as after a continuing iteration: the
// iterate in x0 / g0 with par = 0, stop = 0 unless the record is stopped; the
// pad elements of odd N as the setup leaves them (setup_phase).  Stopped
// records also get their outputs here: nothing else will write them.
__global__ void __launch_bounds__(kStBlock) k_state_load(StateArgs S) {
  const int img = (int)blockIdx.y;
  const int tid = (int)threadIdx.x;
  const int r = S.index ? S.index[img] : img;
  const unsigned char* rec = S.rec + (size_t)r * S.rec_bytes;
  unsigned char* slot = reinterpret_cast<unsigned char*>(S.ws + (size_t)img * S.slot_stride);
  const unsigned vb = S.storage == BSGP_STORAGE_F32 ? 4u : 8u;
  const unsigned nV = ((unsigned)S.N * vb + 15u) / 16u, nD = ((unsigned)S.N * 8u + 15u) / 16u;
  const unsigned total = 4u * nV + (S.bmap ? 2u : 1u) * nD;
  const bool odd = (S.N & 1) != 0;
  for (unsigned c0 = blockIdx.x * (unsigned)(kStBlock * kStU) + (unsigned)tid; c0 < total;
       c0 += gridDim.x * (unsigned)(kStBlock * kStU)) {
    uint4 w[kStU];
#pragma unroll
    for (int u = 0; u < kStU; ++u) {
      const unsigned c = c0 + (unsigned)(u * kStBlock);
      int s;
      unsigned k;
      st_locate(c < total ? c : total - 1u, nV, nD, s, k);
      w[u] = *reinterpret_cast<const uint4*>(rec + st_rec_off(S.L, s) + (size_t)k * 16);
    }
#pragma unroll
    for (int u = 0; u < kStU; ++u) {
      const unsigned c = c0 + (unsigned)(u * kStBlock);
      if (c >= total) continue;
      int s;
      unsigned k;
      st_locate(c, nV, nD, s, k);
      uint4 v = st_mask(w[u], st_sec_bytes(S, s), k);
      if (s == 4 && odd && k == nD - 1u) {  // gns[N] = 1.0: the pair streams' pad element
        v.z = 0u;
        v.w = 0x3ff00000u;
      }
      *reinterpret_cast<uint4*>(slot + st_slot_off(S, s, 0) + (size_t)k * 16) = v;
    }
  }
  if (blockIdx.x != 0) return;
  const bsgp_state_header* h = reinterpret_cast<const bsgp_state_header*>(rec);
  ImgState& st = S.st[img];
  const int done = h->iters_done;
  const int fin = h->stopped;
  const size_t row = (size_t)img * S.M1;
  const double* hd = reinterpret_cast<const double*>(rec + S.L.discr);
  const double* hc = reinterpret_cast<const double*>(rec + S.L.crit);
  const double* ht = reinterpret_cast<const double*>(rec + S.L.times);
  const int* hf = reinterpret_cast<const int*>(rec + S.L.flags);
  for (int k = tid; k <= done && k < S.M1 && k < S.hist_cap; k += kStBlock) {
    S.out.discr[row + k] = hd[k];
    if (S.out.crit) S.out.crit[row + k] = hc[k];
    if (S.out.times) S.out.times[row + k] = ht[k];
    if (S.out.flags) S.out.flags[row + k] = hf[k];
  }
  if (fin == 1) {  // the result a stop rule returned: x * scaling (bb_phase)
    double* xo = S.out.x + (size_t)img * S.N;
    const double sc = h->scaling;
    if (S.storage == BSGP_STORAGE_F32) {
      const float* x = reinterpret_cast<const float*>(rec + S.L.x);
      for (int i = tid; i < S.N; i += kStBlock) xo[i] = x[i] * sc;
    } else {
      const double* x = reinterpret_cast<const double*>(rec + S.L.x);
      for (int i = tid; i < S.N; i += kStBlock) xo[i] = x[i] * sc;
    }
  }
  if (tid < 32) {
    st.Valpha[tid] = h->Valpha[tid];
    st.Fold[tid] = h->Fold[tid];
  }
  if (tid != 0) return;
  if (odd) {  // pad elements of the other buffers (x1, g1, d_tf), as the setup sets them
    const size_t n = (size_t)S.N * vb;
    for (int b = 0; b < 3; ++b) {
      unsigned char* p = slot + (b == 0   ? st_slot_off(S, 0, 1)
                                 : b == 1 ? st_slot_off(S, 1, 1)
                                          : 2 * S.vec_stride * 8 + 5 * S.vec_stride * vb) + n;
      if (vb == 4)
        *reinterpret_cast<float*>(p) = 0.0f;
      else
        *reinterpret_cast<double*>(p) = 0.0;
    }
  }
  st.par = 0;
  st.par_tf = 0;  // the record's x_tf / pw went to the first pair
  st.par_spec = 0;
  st.Xones = h->Xones;
  st.stop = fin != 0;
  st.iter = done + 1;
  st.epoch = h->epoch;
  st.bar_base = 0;  // the team barrier words are zeroed per solve
  st.E_p = h->counters[0];
  st.E_ls = h->counters[1];
  st.ls_passes = h->counters[2];
  st.status = h->counters[3];
  st.ls_series = h->counters[4];
  st.proj_passes = h->counters[5];
  st.proj_list = h->counters[6];
  st.sc = h->scaling;
  st.flux = h->flux;
  st.bks_scalar = h->bkg_scalar;
  st.lo = h->x_low;
  st.hi = h->x_upp;
  st.Dcoeff = h->Dcoeff;
  st.tol = h->tol;
  st.t0 = st_now() - h->elapsed;  // times go on from the record's last entry
  st.fv = h->fv;
  st.alpha = h->alpha;
  st.tau = h->tau;
  st.lr = h->lr;
  st.init_lr = h->init_lr;
  st.beta = h->beta;
  st.lam_p = h->lam_p;
  st.gd = 0.0;   // direction scalars of an iteration: written by k_dir / k_ls
  st.lam = 0.0;  // before they are read
  st.lam_ratio = h->lam_ratio;
  st.kappa = h->kappa;
  st.konst = h->konst;
  st.g32 = h->g32;
  st.gfill = h->gfill;
  if (fin) {
    S.out.iters[img] = done;
    if (S.out.beta_final) S.out.beta_final[img] = h->beta;
    if (S.out.counters) {  // write_counters of the phase kernels
      int64_t* c = S.out.counters + (size_t)img * 8;
      c[0] = h->counters[0];
      c[1] = h->counters[1];
      c[2] = h->counters[2];
      c[3] = h->counters[3];
      c[4] = h->counters[4];
      c[5] = S.T;
      c[6] = h->counters[5];
      c[7] = h->counters[6];
    }
  } else {
    atomicAdd(S.active, 1);
  }
}

// After k_state_load on the same stream.  queue != nullptr: the persistent
// solver's slot order starts at iteration done_it + 1 (task t = done_it * nimg
// is the first dequeued; done[i] = done_it, with the stopped bit for images
// that stay stopped, so task t / nimg lines up with the absolute iteration).
// No image left to run: the host's lookahead poll learns it at once.
__global__ void __launch_bounds__(kStBlock) k_state_post(const ImgState* st, int nimg,
                                                         unsigned* queue, unsigned* done,
                                                         unsigned done_it, const int* active,
                                                         int* done_host, int seq) {
  const int i = (int)(blockIdx.x * (unsigned)kStBlock + threadIdx.x);
  if (queue) {
    if (i == 0) queue[0] = done_it * (unsigned)nimg;
    if (i < nimg) done[i] = st[i].stop ? (kSeedDoneStop | done_it) : done_it;
  }
  if (i == 0 && done_host && *active == 0)
    __hip_atomic_store(done_host, seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

static dim3 state_grid(const StateArgs& a, int B) {
  const size_t vb = a.storage == BSGP_STORAGE_F32 ? 4 : 8;
  const size_t total = 4 * (((size_t)a.N * vb + 15) / 16) +
                       (a.bmap ? 2 : 1) * (((size_t)a.N * 8 + 15) / 16);
  const size_t per = (size_t)kStBlock * kStU;
  size_t gx = (total + per - 1) / per;
  if (gx > 4096) gx = 4096;  // (the kernels stride over the chunk ranges)
  return dim3((unsigned)gx, (unsigned)B);
}

hipError_t launch_state_save(const StateArgs& a, int B, hipStream_t s) {
  hipLaunchKernelGGL(k_state_save, state_grid(a, B), dim3(kStBlock), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_state_load(const StateArgs& a, int B, hipStream_t s) {
  hipLaunchKernelGGL(k_state_load, state_grid(a, B), dim3(kStBlock), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_state_post(const StateArgs& a, int B, unsigned* queue, unsigned* done,
                             int done_it, int* done_host, int seq, hipStream_t s) {
  hipLaunchKernelGGL(k_state_post, dim3((B + kStBlock - 1) / kStBlock), dim3(kStBlock), 0, s,
                     a.st, B, queue, done, (unsigned)done_it, a.active, done_host, seq);
  return hipGetLastError();
}

}  // namespace bsgp
