// bsgp_persist.hip — the float64-storage build of the persistent task-queue
// solver (k_persist, bsgp_kernels.hpp) and the dispatch of both storage
// builds (bsgp_persist_f32.hip holds the float32 one).  Own translation units:
// every k_persist instantiation inlines a whole SGP iteration.
//
// Reference hot path: restoration/sgp.py:748-882 (one iteration of the main
// loop of sgp_betaDiv; :302-425 for sgp), run for every image of a batch.
#include <hip/hip_runtime.h>

#include <vector>

// pass 1 of the line search also sums the second trial, as in the per-wave
// float64 phase kernels (bsgp_solver.hip): the two stay bitwise equal
// (bsgp_kernels.hpp; the float32 and application-size builds leave it off)
#ifndef BSGP_LS1_K2
#define BSGP_LS1_K2 1
#endif
// stream policy of this build's phases (bsgp_device.hpp, "cache policy"):
// O16 | W | SC = the wide operand loads, the operand stores and the column
// pass's spectrum accesses are non-temporal (C3 +2.3 % against plain, same
// box; DESIGN §8 has every mask).  The row-side spectrum (SR) must stay plain:
// its 32-byte pieces of a line are merged across waves in the caches, -36 %
// with nt.  The other persistent units keep the header's 0.
#ifndef BSGP_STREAM_NT
#define BSGP_STREAM_NT 21
#endif
// this unit's eligible kernels carry the compile-time-geometry phases of the
// flagship plan (bsgp_kernels.hpp, BSGP_STATIC_GEO)
#ifndef BSGP_STATIC_GEO
#define BSGP_STATIC_GEO 1
#endif
// one-workgroup images keep their projection lists in the transform buffers'
// LDS as far as they fit (cached_projection, SolveArgs::list_lds)
#ifndef BSGP_PERSIST_LL
#define BSGP_PERSIST_LL 1
#endif
#include "bsgp_kernels.hpp"

namespace bsgp {

hipError_t launch_persist_f32(const SolveArgs& a, int K, size_t lds, hipStream_t s,
                              unsigned* queue, unsigned* done, int grid);
const void* persist_kernel_f32(int K, int mode, bool adapt, bool scalar_bkg);
void persist_kernels_f32(std::vector<const void*>& f);

hipError_t launch_persist(const SolveArgs& a, int K, size_t lds, hipStream_t s, unsigned* queue,
                          unsigned* done, int grid) {
  if (a.g.coop) return bsgp_c512_launch_persist(&a, K, lds, s, queue, done, grid);
  if (app_static_plan(a.g, a.storage))
    return bsgp_app_launch_persist(&a, K, lds, s, queue, done, grid);
  if (a.storage == BSGP_STORAGE_F32) return launch_persist_f32(a, K, lds, s, queue, done, grid);
  return launch_persist_t<double>(a, K, lds, s, queue, done, grid);
}

// The solve takes this unit's float64 kernels (the routing of launch_persist),
// the kernel it takes has the static phases, and the plan is SGeo256's.
bool persist_static_geo(const SolveArgs& a, int K) {
  if (a.g.coop || app_static_plan(a.g, a.storage) || a.storage != BSGP_STORAGE_F64) return false;
  bool adapt = false;
  const int mode = ls_mode(a, &adapt);
  return static_geo_kernel<double, (BSGP_STATIC_GEO != 0)>(false, K >= 2 ? 2 : K, mode, adapt) &&
         static_geo_plan(a);
}

// The kernel the solve takes carries the line search's outcome prediction and
// the solve's parameters let it speculate (ls_phase's kPredBuild and `pred`):
// such a solve needs the second spectrum (SolveArgs::spec2).
bool persist_speculates(const SolveArgs& a) {
  if (a.g.coop || app_static_plan(a.g, a.storage) || a.storage != BSGP_STORAGE_F64) return false;
  bool adapt = false;
  const int mode = ls_mode(a, &adapt);
  return (BSGP_LS1_K2) != 0 && !adapt && (mode == 3 || mode == 4) && a.prm.ls_series != 0 &&
         a.T == 1 && a.ls_predict != 0;
}

// Workgroups of the persistent kernel a solve would launch that one CU holds.
hipError_t persist_resident_per_cu(const SolveArgs& a, int K, size_t lds, int* per_cu) {
  if (a.g.coop) return bsgp_c512_persist_resident(&a, K, lds, per_cu);
  if (app_static_plan(a.g, a.storage)) return bsgp_app_persist_resident(&a, K, lds, per_cu);
  bool adapt = false;
  const int mode = ls_mode(a, &adapt);
  const bool sb = !a.prm.bkg_is_map;
  const void* f = a.storage == BSGP_STORAGE_F32 ? persist_kernel_f32(K, mode, adapt, sb)
                                                : persist_kernel<double>(K, mode, adapt, sb);
  return hipOccupancyMaxActiveBlocksPerMultiprocessor(per_cu, f, kBlock, lds);
}

// phase-profile counters of this translation unit's kernels (-DBSGP_PHASE_PROF;
// phase_prof in bsgp_solver.hip adds them)
hipError_t persist_phase_prof_f32(unsigned long long* out, int n, int reset);
hipError_t persist_phase_prof(unsigned long long* out, int n, int reset) {
#ifdef BSGP_PHASE_PROF
  hipError_t e = hipMemcpyFromSymbol(out, HIP_SYMBOL(g_phase), n * sizeof(unsigned long long));
  if (e == hipSuccess && reset) {
    unsigned long long z[kPhaseSlots] = {};
    e = hipMemcpyToSymbol(HIP_SYMBOL(g_phase), z, sizeof z);
  }
  if (e == hipSuccess) {
    unsigned long long c[kPhaseSlots] = {};
    e = persist_phase_prof_f32(c, n, reset);
    for (int i = 0; i < n; ++i) out[i] += c[i];
  }
  if (e == hipSuccess) {
    unsigned long long c[kPhaseSlots] = {};
    e = bsgp_app_phase_prof(c, n, reset);
    for (int i = 0; i < n; ++i) out[i] += c[i];
  }
  return e;
#else
  for (int i = 0; i < n; ++i) out[i] = 0;
  (void)reset;
  return hipSuccess;
#endif
}

void persist_kernels_all(std::vector<const void*>& f) {
  persist_kernels<double>(f);
  persist_kernels_f32(f);
}

}  // namespace bsgp
