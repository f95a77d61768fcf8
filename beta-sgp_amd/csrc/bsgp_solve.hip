// bsgp_solve.hip — the solves of the C-ABI host layer (declared in
// include/bsgp.h): parameter checks, the team size, the solve launcher
// (solve_impl) with its device, profiled and host entry points, and state save
// and resume (kernels in bsgp_state.hip).  Plans are in bsgp_plan.hip.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "bsgp_host.hpp"

using namespace bsgp;

namespace {

int check_params(const bsgp_params* q) {
  if (!q) return fail(BSGP_ERR_ARG, "params is NULL");
  if (q->variant != BSGP_VARIANT_KL && q->variant != BSGP_VARIANT_BETA)
    return fail(BSGP_ERR_ARG, "bad variant");
  if (q->MAXIT < 1) return fail(BSGP_ERR_ARG, "MAXIT must be >= 1");
  if (q->M_alpha < 1 || q->M_alpha > 32) return fail(BSGP_ERR_ARG, "M_alpha must be in [1, 32]");
  if (q->M < 1 || q->M > 32) return fail(BSGP_ERR_ARG, "M must be in [1, 32]");
  if (q->ls_spec < 1 || q->ls_spec > 8) return fail(BSGP_ERR_ARG, "ls_spec must be in [1, 8]");
  if (q->init_recon < 0 || q->init_recon > 3) return fail(BSGP_ERR_ARG, "bad init_recon");
  if (q->proj_type != 0 && q->proj_type != 1) return fail(BSGP_ERR_ARG, "bad proj_type");
  if (q->scale_data < 0 || q->scale_data > 2) return fail(BSGP_ERR_ARG, "bad scale_data");
  if (q->flux_f32 && !(q->gn_f32 && q->scale_data != 2))
    return fail(BSGP_ERR_ARG, "flux_f32 needs gn_f32 with scale_data 0 or 1");
  return BSGP_OK;
}

// The solve-time A/B knobs, read from the environment once per solve (tests
// flip them between solves of one process).
struct SolveKnobs {
  unsigned spin_limit;  // BSGP_SPIN_LIMIT
  int ls_predict;       // BSGP_LS_PREDICT
  size_t list_lds;      // BSGP_LIST_LDS
  int static_geo;       // BSGP_STATIC_GEO
  int fold_setup;       // BSGP_FOLD_SETUP
  static SolveKnobs from_env() {
    return {(unsigned)env_knob("BSGP_SPIN_LIMIT", 1ll << 26, 0, 0xffffffffll),
            (int)env_knob("BSGP_LS_PREDICT", 1, 0, 5),
            (size_t)env_knob("BSGP_LIST_LDS", 1 << 20, 0, 1 << 20),
            (int)env_knob("BSGP_STATIC_GEO", 1, 0, 1), (int)env_knob("BSGP_FOLD_SETUP", 1, 0, 1)};
  }
};

// Every solve entry point holds one for the call: the choice of
// bsgp_plan_set_static_geo (plan::static_geo_next, which solve_impl reads)
// belongs to this call whatever becomes of it, also when it fails before
// anything runs, and until a solve runs the plan reports no static path.
struct StaticGeoCall {
  bsgp_plan p;
  explicit StaticGeoCall(bsgp_plan q) : p(q) { p->last_static_geo = 0; }
  ~StaticGeoCall() { p->static_geo_next = -1; }
};

// Capacity of one thread's projection list: the pixels it streams in one pass
// (stream2 in bsgp_solver.hip: T == 1 strides pixel pairs over the block; T > 1
// strides row chunks of cp = nfw*W pairs over the members).
int proj_list_cap(const Geo& g, int T) {
  const long npair = ((long)g.H * g.W + 1) / 2;
  const int nb = plan_block(g);
  if (T == 1) return (int)(2 * ((npair + nb - 1) / nb));
  const long cp = (long)g.nfw * g.W;
  const long nch = (npair + cp - 1) / cp;
  return (int)(2 * ((nch + T - 1) / T) * ((cp + nb - 1) / nb));
}

size_t spec2_stride(const bsgp_plan_s* p) {
  return round_up((size_t)p->g.sld * p->g.Qh, 16);  // the slot spectrum's size
}

// Solve sequence numbers for the lookahead poll's host-mapped word: one
// process-wide counter, so no plan (nor a reused pinned block) ever sees a
// value another solve wrote.
std::atomic<int> g_solve_seq{0};

// Workgroups per image.  Every member of every team must be resident at once
// (the team barriers spin): B*T never exceeds the CUs times the workgroups per
// CU the runtime reports for every team kernel of the plan's build
// (p->resident_per_cu, hipOccupancyMaxActiveBlocksPerMultiprocessor).  Each
// member keeps at least one row pair and one column per FFT wave.
int choose_team(const bsgp_plan_s* p, int B, int req) {
  if (req == 1) return 1;
  const Geo& g = p->g;
  const int rows2 = (g.H + 1) / 2;
  int tgeo = rows2 / g.nfw;
  if (g.Qh / g.nfw < tgeo) tgeo = g.Qh / g.nfw;
  const int res = p->ncu * p->resident_per_cu / B;  // resident members per image
  // auto: one workgroup per CU (cooperative plans would fit two per CU, but
  // one per CU measured faster on C4: 1262 vs 1180 it/s)
  int T = std::min(p->ncu / B, tgeo);
  if (req > 1) T = std::min(req, tgeo);
  T = std::min(T, res);
  // the barrier words and the group leaders' polls cover at most kMaxTeam
  // members (bsgp_device.hpp)
  T = std::min(T, kMaxTeam);
  return T < 1 ? 1 : T;
}

// Profiled solves: events around every kernel class of every iteration.
struct SolveProf {
  std::vector<hipEvent_t> ev;  // [MAXIT][6] + setup pair
  double* kernel_ms;
  int64_t* launches;
};

// A resumed solve (bsgp_solve_resume): k_state_load takes the place of the
// setup, and the iteration loop goes on where the records stopped.
struct ResumeCtx {
  StateArgs sa;     // the records (rec, rec_bytes, index, L, hist_cap); solve_impl adds the plan's part
  int T;            // the records' team size
  int it0;          // first iteration to launch: the fewest iterations done + 1
  bool uniform;     // every image that goes on has done `done_it` iterations
  int done_it;
  int beta0_given;  // the records' solve had per-image betas (picks the line-search build)
};

// How a solve runs, decided once (solve_path).
struct SolvePath {
  bool data_stop;  // stop rules 2 to 4: the data decide when an image stops
  bool track;      // per-iteration error / iterate snapshots (errflag, save): one small
                   // kernel after setup and after every iteration, off the hot kernels
  bool persist;    // one k_persist launch runs every iteration
  int K;           // line-search trials per pass of the kernels launched
  int S;           // sub-batches, each on its own stream
};

int validate_solve(bsgp_plan p, int32_t B, const bsgp_params* prm, const bsgp_inputs* in,
                   const bsgp_outputs* out, bool resumed) {
  if (!p) return fail(BSGP_ERR_ARG, "plan is NULL");
  if (int rc = check_params(prm)) return rc;
  if (B < 1) return fail(BSGP_ERR_ARG, "B must be >= 1");
  if (!resumed) {
    if (!in || !in->gn || !in->bkg) return fail(BSGP_ERR_ARG, "inputs gn/bkg missing");
    if ((prm->init_recon == 1 || prm->scale_data == 2) && !in->x0)
      return fail(BSGP_ERR_ARG, "init_recon=1 and scale_data=2 need x0");
  }
  if (!out || !out->x || !out->iters || !out->discr) return fail(BSGP_ERR_ARG, "outputs missing");
  if (out->err && (!in || !in->obj)) return fail(BSGP_ERR_ARG, "err needs the ground truth obj");
  if (p->n_tf > 1 && B != p->n_tf)
    return fail(BSGP_ERR_ARG, "the plan holds one PSF per image: B must equal its PSF count");
  return BSGP_OK;
}

// The kernels' argument block from the plan, the parameters and the team
// size; grows the plan's workspaces, team buffers and projection lists.
int solve_args(bsgp_plan p, int B, int T, const bsgp_params* prm, const bsgp_inputs* in,
               const bsgp_outputs* out, const ResumeCtx* rs, const SolveKnobs& knobs,
               SolveArgs* args) {
  HIP_TRY(p->ws.reserve((size_t)B * p->slot_stride));
  HIP_TRY(p->st.reserve((size_t)B));
  if (T > 1) HIP_TRY(p->tpart.reserve((size_t)B * kPartBufs * (size_t)(T + 8) * kMaxRed));
  HIP_TRY(p->tctr.reserve(round_up(((size_t)B * kTeamWords + kTeamLine) * sizeof(unsigned int), 128) /
                          sizeof(unsigned int)));
  SolveArgs& a = *args;
  a.g = p->g;
  a.prm = *prm;
  if (rs) {
    // no inputs: the records hold what the iterations read.  The kernels read
    // in.beta0 in the setup only; the launchers ask whether it was given
    // (ls_mode), so a resumed solve of per-image betas points it at the state.
    a.in = bsgp_inputs{};
    if (rs->beta0_given) a.in.beta0 = reinterpret_cast<const double*>(p->st.p);
  } else {
    a.in = *in;
  }
  a.out = *out;
  a.B = B;
  a.img0 = 0;
  a.nimg = B;
  a.st = p->st;
  a.active = p->active;
  a.ws = p->ws;
  a.slot_stride = p->slot_stride;
  a.vec_stride = p->vec_stride;
  a.lds_fft_bytes = p->lds_fft_bytes;
  a.T = T;
  // k_col has no team reduction, so a team image may spread its columns over
  // more workgroups than the team has (C4: 1025 columns, 256-member team)
  a.Tc = T;
  if (T > 1) {
    // (one-group cooperative columns pair column 0 with the Nyquist column)
    const int ncol = (p->g.coop && p->g.nfc == 1 && p->g.Q % 2 == 0) ? p->g.Qh - 1 : p->g.Qh;
    const int nc = (ncol + p->g.nfc - 1) / p->g.nfc;
    const int want = 4 * p->ncu / B;
    a.Tc = std::max(T, std::min(nc, want));
  }
  // one-workgroup images run AT's column pass at the end of k_ls (bit 1);
  // teams launch k_col for it
  a.fuse_col = T == 1 ? 2 : 0;
  a.static_geo = 0;
  a.fold_setup = 0;
  a.tpart = T > 1 ? p->tpart.p : nullptr;
  a.tctr = p->tctr;
  a.tfail = reinterpret_cast<int*>(p->tctr + (size_t)B * kTeamWords);
  a.plist = nullptr;
  a.plist_stride = 0;
  a.lcap = 0;
  a.list_lds = 0;
  a.pw = p->pw;
  a.storage = p->storage;
  a.spec_off = p->spec_off;
  a.spec2 = nullptr;
  a.spec2_stride = 0;
  a.spin_limit = knobs.spin_limit;
  a.ls_predict = knobs.ls_predict;
  a.ls_cap = (prm->beta > 0.0 && prm->beta < 1.0)
                 ? (int)std::ceil(std::log(1e-12) / std::log(prm->beta)) + 2
                 : 4096;
  a.done_host = p->done_d;
  if (prm->proj_cache && prm->proj_type == 1) {
    a.lcap = proj_list_cap(p->g, T);
    const size_t half = round_up((size_t)a.lcap * T * plan_block(p->g), 32);
    a.plist_stride = 2 * half;
    HIP_TRY(p->plist.reserve((size_t)B * a.plist_stride));
    a.plist = p->plist;
    // the projection lists stay in the transform buffers' LDS as far as they
    // fit: teams, and one-workgroup images of per-wave plans (there
    // BSGP_LIST_LDS caps the entries per thread; 0: every entry in global memory)
    const size_t fit = p->lds_fft_bytes / ((size_t)plan_block(p->g) * 2 * sizeof(double));
    if (T > 1)
      a.list_lds = (int)std::min<size_t>((size_t)a.lcap, fit);
    else if (!p->g.coop)
      a.list_lds = (int)std::min<size_t>(std::min<size_t>((size_t)a.lcap, fit), knobs.list_lds);
  }
  return BSGP_OK;
}

// Which kernels run the solve.  Sets the argument block's spec2, static_geo
// and fold_setup, and the plan's last_static_geo.
int solve_path(bsgp_plan p, int B, const ResumeCtx* rs, const SolveKnobs& knobs, SolveArgs* args,
               SolvePath* path) {
  SolveArgs& a = *args;
  const bsgp_params& prm = a.prm;
  SolvePath& w = *path;
  w.data_stop = prm.stop_criterion >= 2 && prm.stop_criterion <= 4;
  w.track = a.out.err != nullptr || a.out.x_iter != nullptr;
  w.K = (prm.adapt_beta && prm.variant == BSGP_VARIANT_BETA)
            ? 1
            : (prm.ls_spec <= 1 ? 1 : prm.ls_spec <= 2 ? 2 : prm.ls_spec <= 4 ? 4 : 8);
  // Sub-batches on their own streams (fork/join with the caller's stream):
  // while one sub-batch runs the compute-bound line search the other can
  // stream its memory-bound phases.
  w.S = std::min(std::min(std::max(prm.streams, 1), (int)bsgp_plan_s::kMaxStreams), B);
  // persistent solver (one launch for every iteration, k_persist): one-workgroup
  // images, with per-wave transforms or (cooperative plans: the application's
  // 375^2 / 450^2 subdivisions) the 512-thread build's thread-group transforms
  // (bsgp_persist_c512.hip); it overlaps the phases of different images itself,
  // so it runs the whole batch as one sub-batch
  // (a resumed slot-order solve needs every image at the same iteration; records
  // that are not take the phase kernels, which are bit-identical)
  w.persist = prm.persistent && a.T == 1 && !w.track && (!rs || w.data_stop || rs->uniform);
  if (w.persist) w.S = 1;
  // the speculative fused pass of the persistent line search writes w's rows
  // to a second spectrum per image; without one the kernel never speculates
  if (w.persist && persist_speculates(a)) {
    HIP_TRY(p->spec2.reserve((size_t)B * spec2_stride(p)));
    a.spec2 = p->spec2;
    a.spec2_stride = spec2_stride(p);
  }
  // the flagship plan's compile-time-geometry phases (k_persist): this solve's
  // choice (bsgp_plan_set_static_geo, else BSGP_STATIC_GEO, default on), taken
  // only when the kernel launched carries them and every plan value they fold
  // equals the plan's own
  const int want = p->static_geo_next >= 0 ? p->static_geo_next : knobs.static_geo;
  a.static_geo = (want && w.persist && persist_static_geo(a, w.K)) ? 1 : 0;
  p->last_static_geo = a.static_geo;
  // fixed-length persistent solves run every image's setup as the first task
  // of its chain inside k_persist: the setups of the last images overlap the
  // first iterations of the others, with no k_setup launch and no boundary
  // (BSGP_FOLD_SETUP=0: k_setup first, for A/B)
  a.fold_setup = (w.persist && !w.data_stop && !rs && knobs.fold_setup) ? 1 : 0;
  return BSGP_OK;
}

// sub-batch 0 runs on the caller's stream itself, sub-batches 1..S-1 on the
// plan's streams: S streams in all, so S = 4 fits the 4 hardware queues HIP
// opens per process (GPU_MAX_HW_QUEUES)
int ensure_streams(bsgp_plan p, int S) {
  if (S <= 1 || p->nsub >= S) return BSGP_OK;
  if (!p->ev_fork) HIP_TRY(hipEventCreateWithFlags(&p->ev_fork, hipEventDisableTiming));
  for (int i = (p->nsub > 1 ? p->nsub : 1); i < S; ++i) {
    HIP_TRY(hipStreamCreateWithFlags(&p->sub[i], hipStreamNonBlocking));
    HIP_TRY(hipEventCreateWithFlags(&p->ev_join[i], hipEventDisableTiming));
  }
  p->nsub = S;
  return BSGP_OK;
}

// The per-solve counters, and the plan's record of this solve (bsgp_state_save).
int reset_counters(bsgp_plan p, SolveArgs* a, bool resumed, hipStream_t s) {
  const int B = a->B, T = a->T;
  // device counter of images not yet stopped: B, counted down by every image
  // the setup or k_bb stops (count_stopped); the last one writes this solve's
  // seq to the host-mapped word
  // (resumed: 0, counted up by k_state_load for every image that goes on)
  HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)p->active.p, resumed ? 0 : B, 1, s));
  a->seq = g_solve_seq.fetch_add(1, std::memory_order_relaxed) + 1;
  p->seq = a->seq;
  // team barrier counters and the timeout word restart at 0 every solve
  HIP_TRY(hipMemsetAsync(p->tctr, 0, p->tctr.bytes(), s));
  // flag barriers: every partial slot starts empty
  if (T > 1 && (T <= kTeamFlags || T >= 8))
    HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)p->tpart.p, kPartEmptyWord,
                              B * kPartBufs * (size_t)(T + 8) * kMaxRed * 2, s));
  p->last_valid = true;
  p->last_prm = a->prm;
  p->last_out = a->out;
  p->last_B = B;
  p->last_T = T;
  p->last_beta0 = a->in.beta0 != nullptr;
  return BSGP_OK;
}

// Resumed solves: load the records into the slots.  Returns the load's
// arguments, which run_persistent needs to seed the slot order.
int resume_preload(bsgp_plan p, const SolveArgs& a, const SolvePath& w, const ResumeCtx& rs,
                   hipStream_t s, StateArgs* ld) {
  *ld = rs.sa;
  ld->ws = p->ws;
  ld->slot_stride = p->slot_stride;
  ld->vec_stride = p->vec_stride;
  ld->st = p->st;
  ld->T = a.T;
  ld->M1 = a.prm.MAXIT + 1;
  ld->out = a.out;
  ld->prm = a.prm;
  ld->active = p->active;
  HIP_TRY(launch_state_load(*ld, a.B, s));
  if (!(w.persist && !w.data_stop))
    HIP_TRY(launch_state_post(*ld, a.B, nullptr, nullptr, 0, p->done_d, a.seq, s));
  return BSGP_OK;
}

// The sub-batches' streams and argument blocks: fork from the caller's
// stream, then every sub-batch's setup (unless folded or resumed) and the
// first snapshot.
int launch_setups(bsgp_plan p, const SolveArgs& a, const SolvePath& w, bool resumed, hipStream_t s,
                  SolveProf* prof, hipStream_t* ss, SolveArgs* sa) {
  if (w.S > 1) HIP_TRY(hipEventRecord(p->ev_fork, s));
  for (int j = 0; j < w.S; ++j) {
    ss[j] = j > 0 ? p->sub[j] : s;
    if (j > 0) HIP_TRY(hipStreamWaitEvent(ss[j], p->ev_fork, 0));
    sa[j] = a;
    sa[j].img0 = (int)((int64_t)a.B * j / w.S);
    sa[j].nimg = (int)((int64_t)a.B * (j + 1) / w.S) - sa[j].img0;
    if (prof) HIP_TRY(hipEventRecord(prof->ev[0], ss[j]));
    if (!a.fold_setup && !resumed) HIP_TRY(launch_setup(sa[j], p->lds_bytes, ss[j]));
    if (prof) HIP_TRY(hipEventRecord(prof->ev[1], ss[j]));
    if (w.track) HIP_TRY(launch_track(sa[j], 0, ss[j]));
  }
  return BSGP_OK;
}

// One k_persist launch for every iteration of every image.  ld: the resume
// preload's arguments, or nullptr.
int run_persistent(bsgp_plan p, const SolveArgs& a, const SolvePath& w, const ResumeCtx* rs,
                   const StateArgs* ld, hipStream_t s, SolveProf* prof) {
  const int B = a.B;
  const size_t need = (size_t)2 * B + 4;  // head, tail, pad, ready ring[B] (64-bit entries)
  HIP_TRY(p->pq.reserve(need));
  HIP_TRY(hipMemsetAsync(p->pq, 0, need * sizeof(unsigned), s));
  if (rs && !w.data_stop)  // slot order: the queue starts at the records' iteration
    HIP_TRY(launch_state_post(*ld, B, p->pq, p->pq + 1, rs->done_it, p->done_d, a.seq, s));
  int per_cu = 0;
  HIP_TRY(persist_resident_per_cu(a, w.K, p->lds_bytes, &per_cu));
  if (per_cu < 1) return fail(BSGP_ERR_HIP, "persistent solver does not fit a CU");
  // every workgroup resident at once (a dequeued task's predecessor is always
  // running or done); no more workgroups than images
  const int grid = (int)std::min<long>(B, (long)p->ncu * per_cu);
  if (prof) HIP_TRY(hipEventRecord(prof->ev[2], s));
  HIP_TRY(launch_persist(a, w.K, p->lds_bytes, s, p->pq, p->pq + 1, grid));
  if (prof) HIP_TRY(hipEventRecord(prof->ev[3], s));
  return BSGP_OK;
}

// The phase kernels, iteration by iteration; *it_run: the last one launched.
// Fixed-length runs (stop_criterion 0/1) are launched back to back with no
// host synchronisation.  Data-dependent stop rules are polled with
// lookahead: the host keeps at most kLook iterations queued ahead of the
// device (it waits for the event after iteration it - kLook, never for the
// stream to drain) and stops enqueueing once the host-mapped word carries
// this solve's seq, i.e. every image has stopped; the iterations queued
// past the last stop find every image stopped and return at once.  (Draining
// the stream after every iteration, as round 4 did, is one host round trip
// per iteration on the latency-bound single-image solves: measured and
// removed.)
int run_phased(bsgp_plan p, const SolvePath& w, int it0, int MAXIT, int seq, const hipStream_t* ss,
               const SolveArgs* sa, SolveProf* prof, int* it_run) {
  constexpr int kLook = 2;
  constexpr int kRing = bsgp_plan_s::kPollRing;
  if (w.data_stop)
    for (int i = 0; i < kRing; ++i)
      if (!p->ev_it[i]) HIP_TRY(hipEventCreateWithFlags(&p->ev_it[i], hipEventDisableTiming));
  for (int it = it0; it <= MAXIT; ++it) {
    *it_run = it;
    for (int j = 0; j < w.S; ++j) {
      HIP_TRY(launch_iteration(sa[j], w.K, p->lds_bytes, ss[j],
                               prof ? &prof->ev[2 + 6 * (size_t)(it - 1)] : nullptr));
      if (w.track) HIP_TRY(launch_track(sa[j], it, ss[j]));
    }
    if (w.data_stop && it < MAXIT) {
      HIP_TRY(hipEventRecord(p->ev_it[it % kRing], ss[0]));
      if (it - it0 >= kLook) {
        HIP_TRY(hipEventSynchronize(p->ev_it[(it - kLook) % kRing]));
        if (__atomic_load_n(p->done_h.p, __ATOMIC_ACQUIRE) == seq) break;
      }
    }
  }
  for (int j = 1; j < w.S; ++j) {
    HIP_TRY(hipEventRecord(p->ev_join[j], ss[j]));
    HIP_TRY(hipStreamWaitEvent(ss[0], p->ev_join[j], 0));
  }
  return BSGP_OK;
}

// A profiled solve's times and launch counts per kernel class: 0 setup, 1 dir,
// 2 col (A and AT launches), 3 ls, 4 bb, 5 k_persist.
int read_profile(SolveProf* prof, const SolveArgs& a, bool persist, int it_run, hipStream_t s) {
  HIP_TRY(hipStreamSynchronize(s));
  for (int k = 0; k < 6; ++k) {
    prof->kernel_ms[k] = 0.0;
    prof->launches[k] = 0;
  }
  float ms = 0.f;
  HIP_TRY(hipEventElapsedTime(&ms, prof->ev[0], prof->ev[1]));
  // (a folded setup runs inside k_persist: no k_setup launch)
  prof->kernel_ms[0] = a.fold_setup ? 0.0 : ms;
  prof->launches[0] = a.fold_setup ? 0 : 1;
  if (persist) {
    HIP_TRY(hipEventElapsedTime(&ms, prof->ev[2], prof->ev[3]));
    prof->kernel_ms[5] = ms;
    prof->launches[5] = 1;
    return BSGP_OK;
  }
  const int cls[5] = {1, 2, 3, 2, 4};
  const bool launched[5] = {true, true, true, !(a.fuse_col & 2), true};
  for (int it = 0; it < it_run; ++it) {
    hipEvent_t* e = &prof->ev[2 + 6 * (size_t)it];
    for (int k = 0; k < 5; ++k) {
      HIP_TRY(hipEventElapsedTime(&ms, e[k], e[k + 1]));
      prof->kernel_ms[cls[k]] += ms;
      if (launched[k]) prof->launches[cls[k]] += 1;
    }
  }
  return BSGP_OK;
}

// What in a record's header does not match the plan and the parameters of the
// resume (the first mismatch's name), or nullptr.
const char* record_mismatch(const bsgp_plan_s* p, const bsgp_state_header& h,
                            const bsgp_params* prm, int64_t bytes_per_image) {
  const bsgp_params& q = h.prm;
  const size_t N = (size_t)p->g.H * p->g.W;
  const char* bad = nullptr;
  auto same = [](const void* a, const void* b, size_t n) { return memcmp(a, b, n) == 0; };
#define BSGP_SAME(f) \
  if (!bad && !same(&q.f, &prm->f, sizeof q.f)) bad = #f
  if (h.magic != BSGP_STATE_MAGIC) bad = "magic";
  if (!bad && h.version != BSGP_STATE_VERSION) bad = "version";
  if (!bad && (h.H != p->g.H || h.W != p->g.W)) bad = "shape (H, W)";
  if (!bad && h.storage != p->storage) bad = "storage";
  if (!bad && h.conv_mode != p->conv_mode) bad = "conv_mode";
  BSGP_SAME(variant);
  BSGP_SAME(init_recon);
  BSGP_SAME(proj_type);
  BSGP_SAME(stop_criterion);
  BSGP_SAME(M_alpha);
  BSGP_SAME(M);
  BSGP_SAME(max_projs);
  BSGP_SAME(gamma);
  BSGP_SAME(beta);
  BSGP_SAME(alpha);
  BSGP_SAME(alpha_min);
  BSGP_SAME(alpha_max);
  BSGP_SAME(tau);
  BSGP_SAME(ccd_sat_level);
  BSGP_SAME(betaParam);
  BSGP_SAME(lr);
  BSGP_SAME(lr_exp_param);
  BSGP_SAME(tol_convergence);
  BSGP_SAME(prescaled_scaling);
  BSGP_SAME(prescaled_tol4);
  BSGP_SAME(has_sat);
  BSGP_SAME(scale_data);
  BSGP_SAME(verbose);
  BSGP_SAME(adapt_beta);
  BSGP_SAME(schedule_lr);
  BSGP_SAME(bkg_is_map);
  BSGP_SAME(ls_series);
  BSGP_SAME(gn_compact);
  BSGP_SAME(gn_f32);
  BSGP_SAME(beta0_general);
  BSGP_SAME(flux_f32);
#undef BSGP_SAME
  if (!bad && (h.hist_cap < 1 || h.iters_done < 0 || h.iters_done >= h.hist_cap ||
               h.record_bytes != bytes_per_image ||
               (int64_t)state_layout(N, p->storage, q.bkg_is_map != 0, h.hist_cap).bytes !=
                   bytes_per_image))
    bad = "record_bytes / hist_cap";
  return bad;
}

// Every solve: the caller holds a StaticGeoCall.
int solve_impl(bsgp_plan p, int32_t B, const bsgp_params* prm, const bsgp_inputs* in,
               const bsgp_outputs* out, void* stream, SolveProf* prof,
               const ResumeCtx* rs = nullptr) {
  if (int rc = validate_solve(p, B, prm, in, out, rs != nullptr)) return rc;
  DEVICE_SCOPE(p->device);
  const SolveKnobs knobs = SolveKnobs::from_env();
  hipStream_t s = (hipStream_t)stream;
  const int T = rs ? rs->T : choose_team(p, B, prm->team);
  SolveArgs a;
  if (int rc = solve_args(p, B, T, prm, in, out, rs, knobs, &a)) return rc;
  SolvePath w;
  if (int rc = solve_path(p, B, rs, knobs, &a, &w)) return rc;
  if (int rc = ensure_streams(p, w.S)) return rc;
  if (int rc = reset_counters(p, &a, rs != nullptr, s)) return rc;
  StateArgs ld{};
  if (rs)
    if (int rc = resume_preload(p, a, w, *rs, s, &ld)) return rc;
  hipStream_t ss[bsgp_plan_s::kMaxStreams];
  SolveArgs sa[bsgp_plan_s::kMaxStreams];
  if (int rc = launch_setups(p, a, w, rs != nullptr, s, prof, ss, sa)) return rc;
  int it_run = 0;
  if (int rc = w.persist ? run_persistent(p, sa[0], w, rs, &ld, s, prof)
                         : run_phased(p, w, rs ? rs->it0 : 1, prm->MAXIT, a.seq, ss, sa, prof,
                                      &it_run))
    return rc;
  return prof ? read_profile(prof, sa[0], w.persist, it_run, s) : BSGP_OK;
}

}  // namespace

extern "C" {

// Diagnostics (not in include/bsgp.h): per-phase shader cycles of a build
// with -DBSGP_PHASE_PROF; returns BSGP_ERR_UNSUPPORTED otherwise.
int bsgp_phase_prof(uint64_t* out, int32_t n, int32_t reset) {
  hipError_t e = phase_prof(reinterpret_cast<unsigned long long*>(out), n, reset);
  if (e == hipErrorNotSupported) return fail(BSGP_ERR_UNSUPPORTED, "built without BSGP_PHASE_PROF");
  if (e != hipSuccess) return fail(BSGP_ERR_HIP, hipGetErrorString(e));
  return BSGP_OK;
}

int bsgp_device_synchronize(void) {
  HIP_TRY(hipDeviceSynchronize());
  return BSGP_OK;
}

int bsgp_solve_device(bsgp_plan p, int32_t B, const bsgp_params* prm, const bsgp_inputs* in,
                      const bsgp_outputs* out, void* stream) {
  if (!p) return fail(BSGP_ERR_ARG, "plan is NULL");
  StaticGeoCall sgc(p);
  return solve_impl(p, B, prm, in, out, stream, nullptr);
}

int bsgp_solve_profiled(bsgp_plan p, int32_t B, const bsgp_params* prm, const bsgp_inputs* in,
                        const bsgp_outputs* out, void* stream, double* kernel_ms,
                        int64_t* launches) {
  if (!kernel_ms || !launches) return fail(BSGP_ERR_ARG, "kernel_ms / launches missing");
  if (!prm) return fail(BSGP_ERR_ARG, "params is NULL");
  if (!p) return fail(BSGP_ERR_ARG, "plan is NULL");
  StaticGeoCall sgc(p);
  DEVICE_SCOPE(p->device);
  SolveProf prof;
  prof.kernel_ms = kernel_ms;
  prof.launches = launches;
  const size_t nev = 6 * (size_t)(prm->MAXIT > 0 ? prm->MAXIT : 0) + 2;
  prof.ev.resize(nev, nullptr);
  int rc = BSGP_OK;
  for (size_t i = 0; i < nev && rc == BSGP_OK; ++i)
    if (hipEventCreate(&prof.ev[i]) != hipSuccess) rc = fail(BSGP_ERR_HIP, "event create failed");
  if (rc == BSGP_OK) {
    bsgp_params q = *prm;
    q.streams = 1;  // one stream: kernel spans do not overlap
    rc = solve_impl(p, B, &q, in, out, stream, &prof);
  }
  for (hipEvent_t e : prof.ev)
    if (e) (void)hipEventDestroy(e);
  return rc;
}

int bsgp_solve_host(bsgp_plan p, int32_t B, const bsgp_params* prm, const bsgp_inputs* in,
                    const bsgp_outputs* out) {
  if (!p) return fail(BSGP_ERR_ARG, "plan is NULL");
  int rc = check_params(prm);
  if (rc) return rc;
  if (B < 1 || !in || !in->gn || !in->bkg || !out || !out->x || !out->iters || !out->discr)
    return fail(BSGP_ERR_ARG, "bad arguments");
  DEVICE_SCOPE(p->device);
  const size_t N = (size_t)p->g.H * p->g.W, M1 = (size_t)prm->MAXIT + 1;
  // device copies of the arrays the caller gave: at most 16, freed on return
  DevBuf<unsigned char> bufs[16];
  int nbuf = 0;
  bool ok = true;
  auto dalloc = [&](const void* host, size_t bytes) -> void* {
    if (!host) return nullptr;
    DevBuf<unsigned char>& b = bufs[nbuf++];
    ok = b.reserve(bytes ? bytes : 8) == hipSuccess && ok;
    return b.p;
  };
  bsgp_inputs di{};
  bsgp_outputs dout{};
  const size_t nb = prm->bkg_is_map ? B * N : (size_t)B;
  di.gn = (const double*)dalloc(in->gn, B * N * 8);
  di.bkg = (const double*)dalloc(in->bkg, nb * 8);
  di.flux = (const double*)dalloc(in->flux, B * 8);
  di.x0 = (const double*)dalloc(in->x0, B * N * 8);
  di.beta0 = (const double*)dalloc(in->beta0, B * 8);
  di.obj = (const double*)dalloc(in->obj, B * N * 8);
  dout.x = (double*)dalloc(out->x, B * N * 8);
  dout.iters = (int32_t*)dalloc(out->iters, B * 4);
  dout.discr = (double*)dalloc(out->discr, B * M1 * 8);
  dout.times = (double*)dalloc(out->times, B * M1 * 8);
  dout.crit = (double*)dalloc(out->crit, B * M1 * 8);
  dout.flags = (int32_t*)dalloc(out->flags, B * M1 * 4);
  dout.beta_final = (double*)dalloc(out->beta_final, B * 8);
  dout.counters = (int64_t*)dalloc(out->counters, B * 8 * 8);
  dout.err = (double*)dalloc(out->err, B * M1 * 8);
  dout.x_iter = (double*)dalloc(out->x_iter, B * (M1 - 1) * N * 8);
  if (!ok) return fail(BSGP_ERR_HIP, "device allocation failed");
  auto h2d = [&](const void* d, const void* h, size_t bytes) {
    return !h || hipMemcpy(const_cast<void*>(d), h, bytes, hipMemcpyHostToDevice) == hipSuccess;
  };
  ok = h2d(di.gn, in->gn, B * N * 8) && h2d(di.bkg, in->bkg, nb * 8) &&
       h2d(di.flux, in->flux, B * 8) && h2d(di.x0, in->x0, B * N * 8) &&
       h2d(di.beta0, in->beta0, B * 8) && h2d(di.obj, in->obj, B * N * 8);
  if (!ok) return fail(BSGP_ERR_HIP, "host to device copy failed");
  rc = bsgp_solve_device(p, B, prm, &di, &dout, nullptr);
  if (rc) return rc;
  auto d2h = [&](void* h, const void* d, size_t bytes) {
    return !h || hipMemcpy(h, d, bytes, hipMemcpyDeviceToHost) == hipSuccess;
  };
  ok = hipDeviceSynchronize() == hipSuccess && d2h(out->x, dout.x, B * N * 8) &&
       d2h(out->iters, dout.iters, B * 4) && d2h(out->discr, dout.discr, B * M1 * 8) &&
       d2h(out->times, dout.times, B * M1 * 8) && d2h(out->crit, dout.crit, B * M1 * 8) &&
       d2h(out->flags, dout.flags, B * M1 * 4) && d2h(out->beta_final, dout.beta_final, B * 8) &&
       d2h(out->counters, dout.counters, B * 64) && d2h(out->err, dout.err, B * M1 * 8) &&
       d2h(out->x_iter, dout.x_iter, B * (M1 - 1) * N * 8);
  if (!ok) return fail(BSGP_ERR_HIP, "solve or device to host copy failed");
  return BSGP_OK;
}

// ---- solver state: save / resume (kernels in bsgp_state.hip) ---------------

int bsgp_state_layout(int32_t H, int32_t W, int32_t storage, int32_t bkg_is_map,
                      int32_t hist_cap, int64_t* offs) {
  if (!offs) return fail(BSGP_ERR_ARG, "offs is NULL");
  if (H < 1 || W < 1 || hist_cap < 1) return fail(BSGP_ERR_ARG, "bad shape or hist_cap");
  if (storage != BSGP_STORAGE_F64 && storage != BSGP_STORAGE_F32)
    return fail(BSGP_ERR_ARG, "bad storage");
  const StateLayout L = state_layout((size_t)H * W, storage, bkg_is_map != 0, hist_cap);
  const size_t v[11] = {L.bytes, L.discr, L.crit, L.times, L.flags, L.x,
                        L.g,     L.xtf,   L.pw,   L.gn,    L.bkg};
  for (int i = 0; i < 11; ++i) offs[i] = (int64_t)v[i];
  return BSGP_OK;
}

int bsgp_state_bytes(bsgp_plan p, int32_t bkg_is_map, int32_t MAXIT_done_max,
                     int64_t* bytes_per_image) {
  if (!p) return fail(BSGP_ERR_ARG, "plan is NULL");
  if (!bytes_per_image || MAXIT_done_max < 0) return fail(BSGP_ERR_ARG, "bad arguments");
  *bytes_per_image = (int64_t)state_layout((size_t)p->g.H * p->g.W, p->storage, bkg_is_map != 0,
                                           MAXIT_done_max + 1)
                         .bytes;
  return BSGP_OK;
}

int bsgp_state_save(bsgp_plan p, int32_t B, void* state_dev, int64_t bytes_per_image,
                    void* stream) {
  if (!p) return fail(BSGP_ERR_ARG, "plan is NULL");
  if (!state_dev) return fail(BSGP_ERR_ARG, "state_dev is NULL");
  if (!p->last_valid) return fail(BSGP_ERR_ARG, "no solve has run on this plan");
  if (B != p->last_B || B > 65535)
    return fail(BSGP_ERR_ARG, "B must be the last solve's batch size (at most 65535)");
  const bsgp_params& q = p->last_prm;
  if (q.stop_criterion == 2 && !p->last_out.crit)
    return fail(BSGP_ERR_ARG, "saving a stop_criterion 2 solve needs its out->crit");
  StateArgs a{};
  a.N = p->g.H * p->g.W;
  a.H = p->g.H;
  a.W = p->g.W;
  a.storage = p->storage;
  a.conv_mode = p->conv_mode;
  a.bmap = q.bkg_is_map != 0;
  a.hist_cap = q.MAXIT + 1;
  a.L = state_layout((size_t)a.N, a.storage, a.bmap != 0, a.hist_cap);
  if ((int64_t)a.L.bytes != bytes_per_image)
    return fail(BSGP_ERR_ARG, "bytes_per_image is not bsgp_state_bytes(plan, bkg_is_map, MAXIT)");
  a.rec = static_cast<unsigned char*>(state_dev);
  a.rec_bytes = a.L.bytes;
  a.ws = p->ws;
  a.slot_stride = p->slot_stride;
  a.vec_stride = p->vec_stride;
  a.st = p->st;
  a.T = p->last_T;
  a.beta0_given = p->last_beta0;
  a.M1 = q.MAXIT + 1;
  a.out = p->last_out;
  a.prm = q;
  DEVICE_SCOPE(p->device);
  HIP_TRY(launch_state_save(a, B, (hipStream_t)stream));
  return BSGP_OK;
}

int bsgp_solve_resume(bsgp_plan p, int32_t B, const bsgp_params* prm, const void* state_dev,
                      int32_t n_state, int64_t bytes_per_image, const int32_t* index,
                      const bsgp_outputs* out, void* stream) {
  if (!p) return fail(BSGP_ERR_ARG, "plan is NULL");
  StaticGeoCall sgc(p);
  int rc = check_params(prm);
  if (rc) return rc;
  if (!state_dev || n_state < 1) return fail(BSGP_ERR_ARG, "state_dev missing");
  if (B < 1 || B > 65535 || (!index && B > n_state))
    return fail(BSGP_ERR_ARG, "B must be in [1, 65535] and, without an index, at most n_state");
  if (!out || !out->x || !out->iters || !out->discr) return fail(BSGP_ERR_ARG, "outputs missing");
  if (out->err || out->x_iter)
    return fail(BSGP_ERR_UNSUPPORTED, "err / x_iter are not available on a resumed solve");
  if (p->n_tf > 1 && B != p->n_tf)
    return fail(BSGP_ERR_ARG, "the plan holds one PSF per image: B must equal its PSF count");
  if (bytes_per_image < BSGP_STATE_HEADER_BYTES || bytes_per_image % 16)
    return fail(BSGP_ERR_ARG, "bad bytes_per_image");
  DEVICE_SCOPE(p->device);
  hipStream_t s = (hipStream_t)stream;
  // the headers (and the index) on the host, for validation
  std::vector<bsgp_state_header> hs((size_t)n_state);
  std::vector<int32_t> idx((size_t)B);
  HIP_TRY(hipMemcpy2DAsync(hs.data(), sizeof(bsgp_state_header), state_dev,
                           (size_t)bytes_per_image, sizeof(bsgp_state_header), (size_t)n_state,
                           hipMemcpyDeviceToHost, s));
  if (index)
    HIP_TRY(hipMemcpyAsync(idx.data(), index, (size_t)B * sizeof(int32_t), hipMemcpyDeviceToHost,
                           s));
  HIP_TRY(hipStreamSynchronize(s));
  if (!index)
    for (int i = 0; i < B; ++i) idx[i] = i;
  const size_t N = (size_t)p->g.H * p->g.W;
  ResumeCtx rs{};
  int min_done = -1, max_done = -1;
  char msg[200];
  for (int i = 0; i < B; ++i) {
    if (idx[i] < 0 || idx[i] >= n_state) {
      snprintf(msg, sizeof msg, "index[%d] = %d is outside the %d records", i, idx[i], n_state);
      return fail(BSGP_ERR_ARG, msg);
    }
    const bsgp_state_header& h = hs[(size_t)idx[i]];
    const char* bad = record_mismatch(p, h, prm, bytes_per_image);
    if (!bad && i > 0 && (h.hist_cap != rs.sa.hist_cap || h.T != rs.T ||
                          h.beta0_given != rs.beta0_given))
      bad = "hist_cap / T / beta0_given (records of different solves)";
    if (!bad && h.T < 1) bad = "T";
    if (bad) {
      snprintf(msg, sizeof msg, "state record %d does not match the plan / parameters: %s",
               idx[i], bad);
      return fail(BSGP_ERR_ARG, msg);
    }
    if (prm->MAXIT <= h.iters_done) {
      snprintf(msg, sizeof msg, "MAXIT = %d must exceed the %d iterations record %d has done",
               prm->MAXIT, h.iters_done, idx[i]);
      return fail(BSGP_ERR_ARG, msg);
    }
    if (i == 0) {
      rs.sa.hist_cap = h.hist_cap;
      rs.T = h.T;
      rs.beta0_given = h.beta0_given;
    }
    if (!h.stopped) {
      min_done = min_done < 0 ? h.iters_done : std::min(min_done, h.iters_done);
      max_done = std::max(max_done, h.iters_done);
    }
  }
  // the team size decides the order of every sum: it must be the records'
  const int Tres = choose_team(p, B, prm->team == 0 ? rs.T : prm->team);
  if (Tres != rs.T) {
    snprintf(msg, sizeof msg,
             "team: the records were solved with %d workgroups per image, this resume would "
             "run %d",
             rs.T, Tres);
    return fail(BSGP_ERR_ARG, msg);
  }
  if (min_done < 0) min_done = max_done = prm->MAXIT;  // every record is stopped: nothing runs
  rs.it0 = min_done + 1;
  rs.uniform = min_done == max_done;
  rs.done_it = min_done;
  StateArgs& a = rs.sa;
  a.rec = static_cast<unsigned char*>(const_cast<void*>(state_dev));
  a.rec_bytes = (size_t)bytes_per_image;
  a.index = index;
  a.N = (int)N;
  a.H = p->g.H;
  a.W = p->g.W;
  a.storage = p->storage;
  a.conv_mode = p->conv_mode;
  a.bmap = prm->bkg_is_map != 0;
  a.L = state_layout(N, p->storage, a.bmap != 0, a.hist_cap);
  a.beta0_given = rs.beta0_given;
  return solve_impl(p, B, prm, nullptr, out, stream, nullptr, &rs);
}

}  // extern "C"
