// teb_fleet_inst.hip — ONE fleet instantiation of teb_optimize_kernel per translation unit (teb_fleet.hpp):
//   hipcc -c -DTEB_AMD_FLEET -DTEB_AMD_SOLVE_CSR -DTEB_INST_SOLVER=<0|1|2> -DTEB_INST_SCENE=<0|1> teb_fleet_inst.hip
// Closed-form Jacobians, the non-folded kinds SCENE_POINTS / SCENE_GENERIC only.
#include <hip/hip_runtime.h>

#if !defined(TEB_AMD_FLEET) || !defined(TEB_AMD_SOLVE_CSR)
#error "teb_fleet_inst.hip needs -DTEB_AMD_FLEET and -DTEB_AMD_SOLVE_CSR"
#endif
#if !defined(TEB_INST_SOLVER) || !defined(TEB_INST_SCENE)
#error "teb_fleet_inst.hip needs -DTEB_INST_SOLVER and -DTEB_INST_SCENE"
#endif
#if TEB_INST_SCENE != 0 && TEB_INST_SCENE != 1
#error "fleet units exist for SCENE_POINTS (0) and SCENE_GENERIC (1)"
#endif
#if TEB_INST_SOLVER == 2 && !defined(TEB_AMD_POSE_ITER)
#define TEB_AMD_POSE_ITER 4   // band in HBM: up to four poses per lane (teb_device.hpp: kPoseIterBandHbm)
#endif
#include "teb_fleet.hpp"
#include "teb_kernel.hpp"

static_assert(tebamd::SOLVER_BAND == 0 && tebamd::SOLVER_CR == 1 && tebamd::SOLVER_BANDG == 2, "teb_fleet.hpp numbers the layouts");
static_assert(tebamd::SCENE_POINTS == 0 && tebamd::SCENE_GENERIC == 1, "teb_fleet.hpp numbers the scene kinds");
static_assert(TEB_INST_SOLVER != 2 || tebamd::kMaxPoseIter == tebamd::kPoseIterBandHbm, "the host sizes band-in-HBM handles for kPoseIterBandHbm poses per lane");

__attribute__((visibility("hidden"))) const void* TEB_FLEET_KERNEL_FN(TEB_INST_SOLVER, TEB_INST_SCENE)() {
  return reinterpret_cast<const void*>(&tebamd::teb_optimize_kernel<TEB_INST_SOLVER, TEB_AMD_JACOBIAN_ANALYTIC, TEB_INST_SCENE>);
}
