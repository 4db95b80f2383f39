// teb_fleet_host.hpp — the host rules of a fleet with robot classes (include/teb_amd.h: teb_amd_set_scene_configs), each stated once
// as a pure function over the class list, free of HIP, in the manner of teb_launch_host.hpp: which fields the classes of one map must
// agree on, the one distance path of the launch, whether a launch may change the pose counts, which configuration fields a tick reads
// for a scene (the _per_class calls), the feasibility specs of a fleet. A fleet without a map is the list of
// one class, the handle's configuration; so is the single scene of a handle. teb_amd.hip calls these and decides nothing itself;
// tests/host/fleet_config_host_check.cpp and tests/host/fleet_class_tick_host_check.cpp hold them to hand-written answers.
#pragma once

#include <vector>

#include "teb_launch_host.hpp"

namespace tebamd {

// ---- what the classes of one map must agree on -----------------------------------------------------------------------------------------
// A decision the host takes once per launch cannot follow a field that differs between the classes:
//   jacobian_mode              fleet units exist for closed-form Jacobians only, so every class is TEB_AMD_JACOBIAN_ANALYTIC;
//   include_dynamic_obstacles  the 2-D / 3-D kind of the per-scene signature calls is one per launch (as a truth value).
// cls < 0: the classes agree. Else the first offending class and the field, for the error text.
struct ClassRefusal {
  int cls = -1;
  const char* field = nullptr;
  const char* why = nullptr;
  bool ok() const { return cls < 0; }
};
inline ClassRefusal fleet_classes_agree(const teb_amd_config_t* cfgs, int n_classes) {
  for (int k = 0; k < n_classes; ++k) {
    if (cfgs[k].jacobian_mode != TEB_AMD_JACOBIAN_ANALYTIC)
      return ClassRefusal{k, "jacobian_mode", "fleet kernels exist for TEB_AMD_JACOBIAN_ANALYTIC only"};
    if ((cfgs[k].include_dynamic_obstacles != 0) != (cfgs[0].include_dynamic_obstacles != 0))
      return ClassRefusal{k, "include_dynamic_obstacles", "differs from class 0: the kind of the per-scene signatures is one per launch"};
  }
  return ClassRefusal{};
}
// every scene has a class of the list; -1, or the first scene that has not
inline int first_scene_without_class(const int* class_of_scene, int n_scenes, int n_classes) {
  for (int s = 0; s < n_scenes; ++s)
    if (class_of_scene[s] < 0 || class_of_scene[s] >= n_classes) return s;
  return -1;
}

// ---- the distance path of the launch ---------------------------------------------------------------------------------------------------
inline bool footprint_pointlike(int footprint_type) {
  return footprint_type == TEB_AMD_FOOTPRINT_POINT || footprint_type == TEB_AMD_FOOTPRINT_CIRCULAR;
}
// EVERY class, used by a scene or not (the map says which robots MAY come; the path does not move with the assignment)
inline bool fleet_footprints_pointlike(const teb_amd_config_t* cfgs, int n_classes) {
  for (int k = 0; k < n_classes; ++k)
    if (!footprint_pointlike(cfgs[k].footprint_type)) return false;
  return true;
}
// layout_per_table (teb_launch_host.hpp) over the class list: the point-like path iff the rows of every table AND the footprint of every
// class are point-like and the cache of the widest table (M entries) fits; the generic one otherwise - one path for the whole launch.
template <class PlanBytes>
TableLayout fleet_layout_per_table(bool pointlike_rows, const teb_amd_config_t* cfgs, int n_classes, bool generic_distance_path, int created,
                                   int pin, int M, int stride, size_t lds_limit, PlanBytes bytes) {
  const int footprint = fleet_footprints_pointlike(cfgs, n_classes) ? TEB_AMD_FOOTPRINT_POINT : TEB_AMD_FOOTPRINT_POLYGON;
  return layout_per_table(pointlike_rows, footprint, generic_distance_path, created, pin, M, stride, lds_limit, bytes);
}

// ---- what a launch may do to the pose counts -------------------------------------------------------------------------------------------
// autoResize runs in the bands of every class that has teb_autosize: after an unchecked launch the host's bound on the pose counts is
// void as soon as ANY class resizes.
inline bool fleet_any_autosize(const teb_amd_config_t* cfgs, int n_classes) {
  for (int k = 0; k < n_classes; ++k)
    if (cfgs[k].teb_autosize) return true;
  return false;
}

// ---- what a tick reads from the class of a scene ---------------------------------------------------------------------------------------
// The _per_class calls (include/teb_amd.h) are their _per_scene siblings without the arguments that stand for a configuration field.
// This block is the ONLY place that says which field feeds which argument:
//   dist_to_obst           obstacles.min_obstacle_dist, as the reference passes it (src/homotopy_class_planner.cpp:115): the graph's
//                          vertices on the host and GraphArgs::min_dist of the edge kernel
//   max_vel_x .. min_samples  the three initialisers and updateAndPruneTEB
//   weight_viapoint        the via-point rule after a tick (updateReferenceTrajectoryViaPoints)
//   obst_cost_scale ..     selection_obst_cost_scale, selection_viapoint_cost_scale, selection_alternative_time_cost (computeCurrentCost)
// class_of_scene null: class 0 for every scene (a fleet without a map is the table of one class, the handle's configuration).
struct SceneTickParams {
  double dist_to_obst, max_vel_x, max_vel_theta, acc_lim_x;
  int min_samples;
  double weight_viapoint, obst_cost_scale, viapoint_cost_scale;
  int alternative_time_cost;
};
inline SceneTickParams scene_tick_params(const teb_amd_config_t* cfgs, int n_classes, const int* class_of_scene, int s) {
  const int k = class_of_scene ? class_of_scene[s] : 0;
  const teb_amd_config_t& c = cfgs[k >= 0 && k < n_classes ? k : 0];   // (a map is checked at its install: first_scene_without_class)
  return SceneTickParams{c.min_obstacle_dist, c.max_vel_x, c.max_vel_theta, c.acc_lim_x, c.min_samples, c.weight_viapoint,
                         c.selection_obst_cost_scale, c.selection_viapoint_cost_scale, c.selection_alternative_time_cost};
}

// ---- the feasibility specs of teb_amd_is_trajectory_feasible_per_class -----------------------------------------------------------------
// Every spec passes the checks of the single call (1 <= n_footprint <= max_footprint, both arrays given, radius and angular resolution
// > 0); spec_of_scene gives every scene a spec of the list, or is null: then scene s takes the spec of its class, which needs one spec
// per class of the map (n_classes; 1 without a map). The footprints of all specs lie in one staged array: spec k at
// offset[k] .. offset[k + 1] (x plane, then the y plane after offset[n_specs] entries). Refusal: the first offending spec (or -1) /
// scene (or -1) and the reason, for the error text.
struct SpecRefusal {
  int spec = -1, scene = -1;
  const char* why = nullptr;
  bool ok() const { return why == nullptr; }
};
// the spec of scene s: its entry of spec_of_scene, or (null) its class - class 0 without a map
inline int feasibility_spec_of(const int* spec_of_scene, const int* class_of_scene, int s) {
  return spec_of_scene ? spec_of_scene[s] : class_of_scene ? class_of_scene[s] : 0;
}
struct FeasibilitySpecs {
  SpecRefusal refusal;
  std::vector<int> offset;   // [n_specs + 1]
};
inline FeasibilitySpecs check_feasibility_specs(const teb_amd_feasibility_spec_t* specs, int n_specs, const int* spec_of_scene, int n_scenes,
                                                int n_classes, int max_footprint) {
  FeasibilitySpecs r;
  if (n_specs < 1 || !specs) { r.refusal.why = "needs at least one spec"; return r; }
  r.offset.assign(1, 0);
  for (int k = 0; k < n_specs; ++k) {
    const teb_amd_feasibility_spec_t& q = specs[k];
    const char* why = nullptr;
    if (q.n_footprint < 1 || q.n_footprint > max_footprint) why = "n_footprint outside 1 .. the footprint limit";
    else if (!q.footprint_x || !q.footprint_y) why = "null footprint";
    else if (!(q.inscribed_radius > 0) || !(q.min_resolution_collision_check_angular > 0)) why = "inscribed_radius and the angular resolution must be > 0";
    if (why) { r.refusal.spec = k; r.refusal.why = why; r.offset.clear(); return r; }
    r.offset.push_back(r.offset.back() + q.n_footprint);
  }
  if (!spec_of_scene) {
    if (n_specs != n_classes) { r.refusal.why = "spec_of_scene NULL needs one spec per class of the map (one without a map)"; r.offset.clear(); }
    return r;
  }
  for (int s = 0; s < n_scenes; ++s)
    if (spec_of_scene[s] < 0 || spec_of_scene[s] >= n_specs) {
      r.refusal.scene = s; r.refusal.why = "spec_of_scene entry is not one of the specs"; r.offset.clear();
      return r;
    }
  return r;
}

}  // namespace tebamd
