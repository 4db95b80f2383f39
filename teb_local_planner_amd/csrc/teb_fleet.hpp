// teb_fleet.hpp — fleet batches: the bands of MANY scenes in one launch of teb_optimize_kernel (include/teb_amd.h: teb_amd_set_scenes).
//
// A fleet unit is teb_optimize_kernel compiled with -DTEB_AMD_FLEET (teb_fleet_inst.hip): it takes a FleetDev instead of the
// configuration and one SceneDev, and the table of robot classes (teb_amd_set_scene_configs) as two trailing read-only parameters. The
// workgroup of band b starts with `const SceneDev sc = fl.scenes[fl.scene_of[b]]` and
// `const teb_amd_config_t& c = cfgs[class_of_scene[fl.scene_of[b]]]`. Everything below these lines is the single-scene kernel, so a
// band ends with the bits it has in a single-scene handle that holds only its scene under its class's configuration and launches the
// same kind. A fleet without a class map is launched with a table of one class, the handle's configuration, and a class array of zeros:
// one path. Every SceneDev of the array points at its own segment of the concatenated obstacle rows, with list indices local to it.
//
// Built: the non-folded kinds SCENE_POINTS (0) and SCENE_GENERIC (1) in the three layouts, closed-form Jacobians - six units,
// fleet_<layout>_0_<kind>.o, on the plain calling convention of the solve (-DTEB_AMD_SOLVE_CSR; build.py: FLEET_UNIT_FLAGS). They are not
// part of the opt_<layout>_<jmode>_<kind> table of teb_opt_launch.hpp: the host reaches them through the hidden accessors declared here.
// No helper workgroups, no run-time compilation, no debug_linearize in a fleet launch.
#pragma once
#include "teb_device.hpp"

namespace tebamd {

struct FleetDev {
  const SceneDev* scenes;   // [n_scenes]
  const int* scene_of;      // [B]: scene of band b, < n_scenes (checked by the host before every launch)
};

// selectBestTeb per scene (select_best_kernel's rule - src/homotopy_class_planner.cpp:564-667 - over the bands of ONE scene): one
// workgroup per scene, the lanes stride over the B bands and keep those of scene blockIdx.x. Hysteresis on last_best[s], the
// initial-plan preference on initial_plan[s] (band indices, -1 = none), strict '<', lowest band index on ties. out_idx[s] = -1 (and
// out_cost[s] = numeric_limits<double>::max()) for a scene without bands. selection_cost_hysteresis and selection_prefer_initial_plan
// are those of the scene's class (the table of a fleet launch).
#ifdef TEB_AMD_MAIN_TU
__global__ void __launch_bounds__(kThreads) select_best_per_scene_kernel(const double* cost, const int* scene_of, int B, const int* last_best,
                                                                         const int* initial_plan, const teb_amd_config_t* __restrict__ cfgs,
                                                                         const int* __restrict__ class_of_scene, double* out_cost, int* out_idx) {
  __shared__ double sv[kThreads];
  __shared__ int si[kThreads];
  const int s = blockIdx.x;
  const double hyst = cfgs[class_of_scene[s]].selection_cost_hysteresis, prefer = cfgs[class_of_scene[s]].selection_prefer_initial_plan;
  const int lb = last_best ? last_best[s] : -1, ip = initial_plan ? initial_plan[s] : -1;
  double best = 1.7976931348623157e308;
  int bi = -1;
  for (int i = threadIdx.x; i < B; i += kThreads) {
    if (scene_of[i] != s) continue;
    double cst = cost[i];
    if (i == lb) cst = cst * hyst;
    else if (i == ip) cst = cst * prefer;
    if (cst < best) { best = cst; bi = i; }
  }
  sv[threadIdx.x] = best; si[threadIdx.x] = bi;
  __syncthreads();
  for (int w = kThreads / 2; w > 0; w >>= 1) {
    if (threadIdx.x < w) {
      const double ov = sv[threadIdx.x + w]; const int oi = si[threadIdx.x + w];
      const double mv = sv[threadIdx.x]; const int mi = si[threadIdx.x];
      const bool take = (oi >= 0) && (mi < 0 || ov < mv || (ov == mv && oi < mi));
      if (take) { sv[threadIdx.x] = ov; si[threadIdx.x] = oi; }
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) { out_cost[s] = sv[0]; out_idx[s] = si[0]; }
}
#endif

}  // namespace tebamd

// The fleet units and how the host reaches them: layout 0 SOLVER_BAND, 1 SOLVER_CR, 2 SOLVER_BANDG; kind 0 SCENE_POINTS, 1 SCENE_GENERIC.
#define TEB_FLEET_CAT_(a, b, c) a##_##b##_##c
#define TEB_FLEET_CAT(a, b, c) TEB_FLEET_CAT_(a, b, c)
#define TEB_FLEET_KERNEL_FN(S, P) TEB_FLEET_CAT(teb_fleet_kernel, S, P)
#define TEB_FLEET_DECLARE(S, P) __attribute__((visibility("hidden"))) const void* TEB_FLEET_KERNEL_FN(S, P)();
#define TEB_FLEET_FOR_ALL(X) X(0, 0) X(1, 0) X(2, 0) X(0, 1) X(1, 1) X(2, 1)
