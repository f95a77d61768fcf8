// bsgp_solver_f32.hip — the float32-storage build (BSGP_STORAGE_F32, SURVEY
// config C4) of the batched beta-SGP phase kernels of bsgp_kernels.hpp with
// per-wave transforms: the seven iteration vectors in float32, every reduction
// and scalar in float64.  (Cooperative plans: bsgp_solver_c512.hip.)
#include <hip/hip_runtime.h>

#include <vector>

#include "bsgp_kernels.hpp"

namespace bsgp {

hipError_t launch_setup_f32(const SolveArgs& a, size_t lds, hipStream_t s) {
  return launch_setup_t<false, float>(a, lds, s);
}
hipError_t launch_iteration_f32(const SolveArgs& a, int K, size_t lds, hipStream_t s,
                                hipEvent_t* ev) {
  return launch_iteration_t<false, float>(a, K, lds, s, ev);
}
hipError_t launch_track_f32(const SolveArgs& a, int it, hipStream_t s) {
  return launch_track_t<float>(a, it, s);
}
void solver_kernels_f32(std::vector<const void*>& f) { solver_kernels<false, float>(f); }

}  // namespace bsgp
