// teb_fleet_host.hpp — the host rules of a fleet with robot classes (include/teb_amd.h: teb_amd_set_scene_configs), each stated once
// as a pure function over the class list, free of HIP, in the manner of teb_launch_host.hpp: which fields the classes of one map must
// agree on, the one distance path of the launch, whether a launch may change the pose counts. A fleet without a map is the list of
// one class, the handle's configuration; so is the single scene of a handle. teb_amd.hip calls these and decides nothing itself;
// tests/host/fleet_config_host_check.cpp holds them to hand-written answers.
#pragma once

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

}  // namespace tebamd
