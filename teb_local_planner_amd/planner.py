"""Host-side mirror of the reference's optimiser interface on top of the C-ABI (libteb_amd.so).

  TebOptimalPlanner.optimizeTEB(...)         <-> reference optimal_planner.h:231-232
  HomotopyClassPlanner.optimizeAllTEBs(...)  <-> reference src/homotopy_class_planner.cpp:466-493
  HomotopyClassPlanner.selectBestTeb()       <-> reference src/homotopy_class_planner.cpp:564-667

Same names, argument meaning and error behaviour (bool returns, no exceptions for optimiser failures).
The library is loaded with ctypes; there is NO CPU fallback: constructing a solver without a gfx950 GPU
raises TebAmdError.
"""
import ctypes as C
import os

import numpy as np

from . import _abi
from .config import TebConfig, normalize_theta

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None


class TebAmdError(RuntimeError):
    def __init__(self, code, what, msg):
        super().__init__("%s failed: status %d (%s)" % (what, code, msg))
        self.code = code


class FeasibilitySpec(C.Structure):
    """teb_amd_feasibility_spec_t: what the adapter passes to isTrajectoryFeasible for one robot class"""
    _fields_ = [("n_footprint", C.c_int32), ("footprint_x", _abi.p_f64), ("footprint_y", _abi.p_f64), ("inscribed_radius", C.c_double),
                ("min_resolution_collision_check_angular", C.c_double), ("look_ahead_idx", C.c_int32),
                ("feasibility_check_lookahead_distance", C.c_double)]


def lib():
    """Loads libteb_amd.so (built in-tree by teb_local_planner_amd.build)."""
    global _LIB
    if _LIB is None:
        so = os.environ.get("TEB_AMD_LIB") or os.path.join(_HERE, "libteb_amd.so")   # TEB_AMD_LIB: kernel experiments (tools/)
        if not os.path.exists(so):
            raise TebAmdError(-1, "load", "libteb_amd.so missing: run `python -m teb_local_planner_amd.build`")
        L = C.CDLL(so)
        vp = C.c_void_p
        L.teb_amd_last_error.restype = C.c_char_p
        L.teb_amd_config_default.argtypes = [C.POINTER(_abi.Config)]
        L.teb_amd_create.argtypes = [C.POINTER(_abi.Config), C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                     C.c_int32, vp, C.POINTER(vp)]
        L.teb_amd_create_ex.argtypes = [C.POINTER(_abi.Config), C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                        C.c_int32, vp, C.POINTER(_abi.Options), C.POINTER(vp)]
        L.teb_amd_options_default.argtypes = [C.POINTER(_abi.Options)]
        L.teb_amd_options_default.restype = None
        L.teb_amd_destroy.argtypes = [vp]
        L.teb_amd_destroy.restype = None
        L.teb_amd_set_config.argtypes = [vp, C.POINTER(_abi.Config)]
        L.teb_amd_set_obstacles.argtypes = [vp, C.POINTER(_abi.Obstacles)]
        L.teb_amd_set_via_points.argtypes = [vp, C.c_int32, _abi.p_f64, _abi.p_f64]
        L.teb_amd_upload_tebs.argtypes = [vp, C.POINTER(_abi.TebBatch)]
        L.teb_amd_download_tebs.argtypes = [vp, C.POINTER(_abi.TebBatch)]
        L.teb_amd_optimize_batch.argtypes = [vp, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_double, C.c_int32]
        L.teb_amd_synchronize.argtypes = [vp]
        L.teb_amd_get_results.argtypes = [vp, C.POINTER(_abi.Results)]
        L.teb_amd_select_best.argtypes = [vp, C.c_int32, C.c_int32, _abi.p_i32, _abi.p_f64]
        if hasattr(L, "teb_amd_last_launch_info"):
            L.teb_amd_last_launch_info.argtypes = [vp, _abi.p_i32, _abi.p_i32, _abi.p_i32]
        if hasattr(L, "teb_amd_multi_cu_backoff"):
            L.teb_amd_multi_cu_backoff.argtypes = [vp, _abi.p_i32, _abi.p_i32]
        if hasattr(L, "teb_amd_set_iteration_log"):   # (absent from the older builds tools/ compares against through TEB_AMD_LIB)
            L.teb_amd_set_iteration_log.argtypes = [vp, C.c_int32]
            L.teb_amd_get_iteration_log.argtypes = [vp, C.c_int32, _abi.p_f64, C.c_int32, _abi.p_i32]
            L.teb_amd_debug_world_argmin.argtypes = [_abi.p_f64, C.c_int32, _abi.p_i32, _abi.p_f64, _abi.p_i32]
        L.teb_amd_device_state.argtypes = [vp] + [C.POINTER(vp)] * 5 + [_abi.p_i32]
        L.teb_amd_snapshot_state.argtypes = [vp]
        L.teb_amd_restore_state.argtypes = [vp]
        L.teb_amd_last_kernel_ms.argtypes = [vp, C.POINTER(C.c_float)]
        L.teb_amd_capacity.argtypes = [vp, _abi.p_i32, _abi.p_i32]
        L.teb_amd_debug_linearize.argtypes = [vp, C.c_int32, C.c_double, _abi.p_f64, _abi.p_f64, _abi.p_f64,
                                              _abi.p_i32, _abi.p_i32, C.c_int32, _abi.p_i32]
        L.teb_amd_debug_distance.argtypes = [vp, C.c_int32, _abi.p_i32, _abi.p_f64, _abi.p_f64, _abi.p_f64,
                                             _abi.p_i32, _abi.p_f64, _abi.p_f64, _abi.p_f64]
        L.teb_amd_debug_assoc_overflow.argtypes = [vp, _abi.p_i32]
        L.teb_amd_debug_stream.argtypes = [vp, C.c_int64, C.c_int32]
        L.teb_amd_debug_profile.argtypes = [vp, _abi.p_f64]
        # producers / consumers of the device-resident strips
        d, i32 = C.c_double, C.c_int32
        L.teb_amd_init_trajectory_line.argtypes = [vp, i32, _abi.p_f64, _abi.p_f64, d, d, i32, i32]
        L.teb_amd_init_trajectory_plan.argtypes = [vp, i32, i32, _abi.p_f64, _abi.p_f64, _abi.p_f64, d, d, i32, i32, i32]
        L.teb_amd_init_trajectory_path.argtypes = [vp, i32, i32, _abi.p_f64, _abi.p_f64, d, d, _abi.p_f64, _abi.p_f64, _abi.p_f64,
                                                   i32, i32]
        L.teb_amd_update_and_prune.argtypes = [vp, i32, _abi.p_f64, _abi.p_f64, i32]
        L.teb_amd_set_velocity_start.argtypes = [vp, i32, i32, _abi.p_f64]
        L.teb_amd_set_velocity_goal.argtypes = [vp, i32, i32, _abi.p_f64]
        L.teb_amd_get_pose_counts.argtypes = [vp, _abi.p_i32, _abi.p_i32]
        L.teb_amd_get_velocity_command.argtypes = [vp, i32, i32, i32, _abi.p_f64, _abi.p_f64, _abi.p_f64, _abi.p_i32]
        L.teb_amd_get_velocity_profile.argtypes = [vp, i32, _abi.p_f64, i32, _abi.p_i32]
        L.teb_amd_get_full_trajectory.argtypes = [vp, i32, _abi.p_f64, i32, _abi.p_i32]
        L.teb_amd_has_diverged.argtypes = [vp, i32, _abi.p_i32]
        L.teb_amd_get_batch_statistics.argtypes = [vp, _abi.p_i32, _abi.p_f64]
        L.teb_amd_compute_h_signatures.argtypes = [vp, d, _abi.p_f64, _abi.p_i32]
        L.teb_amd_filter_equivalence_classes.argtypes = [vp, d, i32, i32, _abi.p_i32, _abi.p_i32, _abi.p_i32]
        L.teb_amd_explore_candidates.argtypes = [vp, C.POINTER(_abi.HcpParams), _abi.p_f64, _abi.p_f64, d, _abi.p_f64, i32, i32,
                                                 _abi.p_f64, C.c_int64, _abi.p_i32, _abi.p_i32, _abi.p_i32, i32, _abi.p_f64, _abi.p_f64,
                                                 _abi.p_f64, _abi.p_i32]
        L.teb_amd_get_exploration_graph.argtypes = [vp, _abi.p_f64, _abi.p_f64, C.POINTER(C.c_ubyte), i32, _abi.p_i32]
        L.teb_amd_compact_bands.argtypes = [vp, _abi.p_i32, i32, _abi.p_i32, _abi.p_i32]
        L.teb_amd_filter_detours.argtypes = [vp, C.POINTER(_abi.HcpParams), i32, _abi.p_i32]
        L.teb_amd_set_optimized_flags.argtypes = [vp, _abi.p_i32]
        L.teb_amd_get_optimized_flags.argtypes = [vp, _abi.p_i32]
        L.teb_amd_get_band_flags.argtypes = [vp, _abi.p_i32, _abi.p_i32, _abi.p_i32]
        L.teb_amd_hcp_params_default.argtypes = [C.POINTER(_abi.HcpParams)]
        L.teb_amd_hcp_params_default.restype = None
        L.teb_amd_set_costmap.argtypes = [vp, C.c_void_p, i32, i32, d, d, d]
        L.teb_amd_is_trajectory_feasible.argtypes = [vp, i32, i32, _abi.p_f64, _abi.p_f64, d, d, i32, d, _abi.p_i32, _abi.p_i32]
        L.teb_amd_set_obstacles_from_costmap.argtypes = [vp, _abi.p_f64, d, C.POINTER(_abi.Obstacles), _abi.p_i32, _abi.p_f64, _abi.p_f64, i32]
        L.teb_amd_set_obstacles_from_costmap_polygons.argtypes = [vp, _abi.p_f64, d, i32, C.POINTER(_abi.Obstacles), _abi.p_i32,
                                                                  _abi.p_i32, _abi.p_i32, _abi.p_f64, _abi.p_f64, i32, i32]
        # multi-GPU exchange
        L.teb_amd_comm_unique_id.argtypes = [C.c_char_p]
        L.teb_amd_comm_create.argtypes = [C.c_char_p, i32, i32, i32, C.POINTER(vp)]
        L.teb_amd_comm_destroy.argtypes = [vp]
        L.teb_amd_comm_destroy.restype = None
        L.teb_amd_select_best_distributed.argtypes = [vp, vp, i32, i32, i32, _abi.p_i32, _abi.p_f64, _abi.p_i32]
        L.teb_amd_broadcast_band.argtypes = [vp, vp, i32, i32, i32, _abi.p_i32, _abi.p_f64, _abi.p_f64, _abi.p_f64, _abi.p_f64]
        if hasattr(L, "teb_amd_set_scenes"):   # fleet batches (absent from the older builds tools/ compares against through TEB_AMD_LIB)
            L.teb_amd_set_scenes.argtypes = [vp, i32, C.POINTER(_abi.Obstacles), _abi.p_i32, _abi.p_f64, _abi.p_f64]
            L.teb_amd_set_band_scenes.argtypes = [vp, _abi.p_i32, i32]
            L.teb_amd_clear_scenes.argtypes = [vp]
            L.teb_amd_get_scene_count.argtypes = [vp, _abi.p_i32]
            L.teb_amd_select_best_per_scene.argtypes = [vp, _abi.p_i32, _abi.p_i32, _abi.p_i32, _abi.p_f64]
        if hasattr(L, "teb_amd_set_scene_configs"):   # robot classes: a configuration per scene of a fleet batch
            L.teb_amd_set_scene_configs.argtypes = [vp, i32, C.POINTER(_abi.Config), i32, _abi.p_i32]
            L.teb_amd_clear_scene_configs.argtypes = [vp]
            L.teb_amd_get_scene_configs.argtypes = [vp, _abi.p_i32, _abi.p_i32, i32]
        if hasattr(L, "teb_amd_compute_h_signatures_per_scene"):   # equivalence classes per scene of a fleet batch
            L.teb_amd_compute_h_signatures_per_scene.argtypes = [vp, d, _abi.p_f64, C.c_int64, _abi.p_i32, C.POINTER(C.c_int64)]
            L.teb_amd_filter_equivalence_classes_per_scene.argtypes = [vp, d, _abi.p_i32, i32, _abi.p_i32, _abi.p_i32, _abi.p_i32]
            L.teb_amd_filter_detours_per_scene.argtypes = [vp, C.POINTER(_abi.HcpParams), _abi.p_i32, _abi.p_i32]
        if hasattr(L, "teb_amd_explore_candidates_per_scene"):   # candidate exploration per scene of a fleet batch
            L.teb_amd_explore_candidates_per_scene.argtypes = [vp, C.POINTER(_abi.HcpParams), _abi.p_f64, _abi.p_f64, d, _abi.p_f64, i32, _abi.p_i32,
                                                               _abi.p_f64, C.c_int64, _abi.p_i32, _abi.p_i32, _abi.p_i32, _abi.p_i32, _abi.p_i32,
                                                               _abi.p_f64, _abi.p_f64, _abi.p_f64, _abi.p_i32]
            L.teb_amd_get_exploration_graph_per_scene.argtypes = [vp, i32, _abi.p_f64, _abi.p_f64, C.POINTER(C.c_ubyte), i32, _abi.p_i32]
            L.teb_amd_compact_bands_per_scene.argtypes = [vp, _abi.p_i32, _abi.p_i32, _abi.p_i32, _abi.p_i32]
            L.teb_amd_get_band_scenes.argtypes = [vp, _abi.p_i32, i32, _abi.p_i32]
            L.teb_amd_debug_set_explore_quota.argtypes = [vp, i32]
        if hasattr(L, "teb_amd_set_costmaps"):   # both ends of a fleet tick per scene
            L.teb_amd_set_costmaps.argtypes = [vp, i32, C.c_void_p, _abi.p_i32, _abi.p_i32, _abi.p_f64, _abi.p_f64, _abi.p_f64]
            L.teb_amd_set_scenes_from_costmaps.argtypes = [vp, i32, _abi.p_f64, d, C.POINTER(_abi.Obstacles), _abi.p_i32, _abi.p_f64, _abi.p_f64,
                                                           _abi.p_i32, _abi.p_f64, _abi.p_f64, i32]
            L.teb_amd_is_trajectory_feasible_per_scene.argtypes = [vp, _abi.p_i32, i32, _abi.p_f64, _abi.p_f64, d, d, i32, d, _abi.p_i32, _abi.p_i32]
            L.teb_amd_update_and_prune_per_scene.argtypes = [vp, _abi.p_f64, _abi.p_f64, i32, _abi.p_f64, _abi.p_i32]
            L.teb_amd_get_velocity_commands.argtypes = [vp, i32, _abi.p_i32, i32, i32, _abi.p_f64, _abi.p_i32]
        if hasattr(L, "teb_amd_set_scenes_from_costmap_polygons"):   # the polygon route of the costmap per scene
            L.teb_amd_set_scenes_from_costmap_polygons.argtypes = [vp, i32, _abi.p_f64, d, _abi.p_i32, C.POINTER(_abi.Obstacles), _abi.p_i32,
                                                                   _abi.p_f64, _abi.p_f64, _abi.p_i32, _abi.p_i32, _abi.p_i32, _abi.p_f64,
                                                                   _abi.p_f64, i32, i32]
        if hasattr(L, "teb_amd_explore_candidates_per_class"):   # the whole tick per robot class: the _per_scene calls without the configuration fields
            L.teb_amd_explore_candidates_per_class.argtypes = [vp, C.POINTER(_abi.HcpParams), _abi.p_f64, _abi.p_f64, _abi.p_f64, i32, _abi.p_i32,
                                                               _abi.p_f64, C.c_int64, _abi.p_i32, _abi.p_i32, _abi.p_i32, _abi.p_i32, _abi.p_i32,
                                                               _abi.p_f64, _abi.p_f64, _abi.p_f64, _abi.p_i32]
            L.teb_amd_update_and_prune_per_class.argtypes = [vp, _abi.p_f64, _abi.p_f64, _abi.p_f64, _abi.p_i32]
            L.teb_amd_optimize_batch_per_class.argtypes = [vp, i32, i32, i32]
            L.teb_amd_is_trajectory_feasible_per_class.argtypes = [vp, _abi.p_i32, i32, C.POINTER(FeasibilitySpec), _abi.p_i32, _abi.p_i32, _abi.p_i32]
        if hasattr(L, "teb_amd_plan_windows"):   # local plan windows per robot from resident global plans
            L.teb_amd_plan_window_params_default.argtypes = [C.POINTER(_abi.PlanWindowParams)]
            L.teb_amd_plan_window_params_default.restype = None
            L.teb_amd_set_global_plans.argtypes = [vp, i32, _abi.p_i32, _abi.p_f64, _abi.p_f64, _abi.p_f64, _abi.p_i32]
            L.teb_amd_plan_windows.argtypes = [vp, i32, C.POINTER(_abi.PlanWindowParams), _abi.p_f64, _abi.p_f64, _abi.p_f64, _abi.p_i32, _abi.p_i32,
                                               _abi.p_i32, _abi.p_i32, _abi.p_f64, _abi.p_f64, _abi.p_i32, _abi.p_i32, _abi.p_f64, _abi.p_f64,
                                               _abi.p_f64, i32, _abi.p_i32, _abi.p_f64, _abi.p_f64, i32]
            L.teb_amd_get_plan_cursors.argtypes = [vp, _abi.p_i32]
        _LIB = L
    return _LIB


def _chk(rc, what):
    if rc != 0:
        raise TebAmdError(rc, what, lib().teb_amd_last_error().decode())


class TebBatchSolver:
    """Thin RAII wrapper of a teb_amd_handle_t (one per GPU / host thread)."""

    def __init__(self, cfg, max_tebs, max_poses, max_obstacles=0, max_obstacle_vertices=0, max_via_points=0,
                 device=0, stream=None, options=None):
        self._h = C.c_void_p(None)
        self.cfg = cfg
        c = cfg.to_c()
        _chk(lib().teb_amd_create_ex(C.byref(c), max_tebs, max_poses, max_obstacles, max_obstacle_vertices,
                                     max_via_points, device, C.c_void_p(stream) if stream else None,
                                     C.byref(options) if options is not None else None, C.byref(self._h)), "teb_amd_create_ex")
        self.max_tebs, self.max_poses, self.max_obstacles = max_tebs, max_poses, max_obstacles
        self.max_obstacle_vertices = max_obstacle_vertices
        self.count = 0
        self._plan_counts = None   # pose counts of the resident global plans (set_global_plans)

    def close(self):
        if self._h:
            lib().teb_amd_destroy(self._h)
            self._h = C.c_void_p(None)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- scene ---------------------------------------------------------------------------------------
    def set_config(self, cfg):
        self.cfg = cfg
        c = cfg.to_c()
        _chk(lib().teb_amd_set_config(self._h, C.byref(c)), "teb_amd_set_config")

    def set_obstacles(self, obst):
        _chk(lib().teb_amd_set_obstacles(self._h, C.byref(obst.freeze())), "teb_amd_set_obstacles")
        self._n_obst = len(obst)

    def set_via_points(self, via):
        vx = _abi.f64([v[0] for v in via]) if via else _abi.f64([0.0])
        vy = _abi.f64([v[1] for v in via]) if via else _abi.f64([0.0])
        _chk(lib().teb_amd_set_via_points(self._h, len(via), _abi._ptr(vx, C.c_double), _abi._ptr(vy, C.c_double)),
             "teb_amd_set_via_points")

    # -- fleet batches: a set of scenes and a band -> scene map (include/teb_amd.h) ------------------------
    def set_scenes(self, tables, vias=None):
        """Installs one scene per entry of `tables` (ObstacleTable) with its via-points ([(x, y), ...] per scene or None) and enters
        fleet mode: optimize() then runs every band against the scene set_band_scenes gave it, in one launch."""
        p = _abi.pack_scenes(tables, vias)
        _chk(lib().teb_amd_set_scenes(self._h, p.n, p.obstacles, _abi._ptr(p.via_count, C.c_int32), _abi._ptr(p.via_x, C.c_double),
                                      _abi._ptr(p.via_y, C.c_double)), "teb_amd_set_scenes")
        self._widest_scene = max(len(t) for t in tables)
        self._n_scenes = len(tables)

    def set_band_scenes(self, scene_of):
        a = _abi.i32(scene_of)
        _chk(lib().teb_amd_set_band_scenes(self._h, _abi._ptr(a, C.c_int32), len(a)), "teb_amd_set_band_scenes")

    def clear_scenes(self):
        _chk(lib().teb_amd_clear_scenes(self._h), "teb_amd_clear_scenes")
        self._n_scenes = 0

    def scene_count(self):
        n = C.c_int32(0)
        _chk(lib().teb_amd_get_scene_count(self._h, C.byref(n)), "teb_amd_get_scene_count")
        return n.value

    def set_scene_configs(self, cfgs, class_of_scene):
        """Installs the robot classes `cfgs` (TebConfig each, footprint included) and the class of every scene of the set
        (teb_amd_set_scene_configs): every band then runs under the configuration of its scene's class. Lengths are checked here,
        everything else by the library."""
        p = _abi.pack_scene_configs(cfgs, class_of_scene, getattr(self, "_n_scenes", 0))
        _chk(lib().teb_amd_set_scene_configs(self._h, p.n_classes, p.configs, p.n_scenes, _abi._ptr(p.class_of_scene, C.c_int32)),
             "teb_amd_set_scene_configs")

    def clear_scene_configs(self):
        _chk(lib().teb_amd_clear_scene_configs(self._h), "teb_amd_clear_scene_configs")

    def scene_configs(self):
        """(number of classes, class of every scene [n_scenes]) of the installed class map; (0, empty) without one."""
        n = C.c_int32(0)
        _chk(lib().teb_amd_get_scene_configs(self._h, C.byref(n), None, 0), "teb_amd_get_scene_configs")
        if n.value == 0:
            return 0, np.zeros(0, np.int32)
        of = np.zeros(max(self.max_tebs, 1), np.int32)
        _chk(lib().teb_amd_get_scene_configs(self._h, C.byref(n), _abi._ptr(of, C.c_int32), len(of)), "teb_amd_get_scene_configs")
        return n.value, of[:self.scene_count()].copy()

    def select_best_per_scene(self, last_best=None, initial_plan=None):
        """(best [n_scenes] band indices, -1 for a scene without bands; scaled costs [n_scenes]). last_best / initial_plan: band index
        per scene or -1, None = none."""
        ns = self.scene_count()
        best = np.full(max(ns, 1), -1, np.int32); cost = np.zeros(max(ns, 1))
        lb = None if last_best is None else _abi.i32(last_best)
        ip = None if initial_plan is None else _abi.i32(initial_plan)
        for a in (lb, ip):
            if a is not None and len(a) != ns:
                raise ValueError("select_best_per_scene: %d entries for %d scenes" % (len(a), ns))
        _chk(lib().teb_amd_select_best_per_scene(self._h, _abi._ptr(lb, C.c_int32), _abi._ptr(ip, C.c_int32), _abi._ptr(best, C.c_int32),
                                                 _abi._ptr(cost, C.c_double)), "teb_amd_select_best_per_scene")
        return best[:ns].copy(), cost[:ns].copy()

    def h_signatures_per_scene(self, prescaler=1.0, values=True):
        """Fleet mode: the H-signature of every band against its own scene, one launch - a list of per-band arrays, [rows of the band's
        scene] (HSignature3d, include_dynamic_obstacles) or [2] (HSignature: re, im). values=False: compute only (the signatures stay
        in the handle for filter_equivalence_classes_per_scene)."""
        self._sync_count()
        n = C.c_int64(0)
        if not values:
            _chk(lib().teb_amd_compute_h_signatures_per_scene(self._h, prescaler, None, 0, None, C.byref(n)), "teb_amd_compute_h_signatures_per_scene")
            return None
        B = max(self.count, 1)
        out = np.zeros(B * max(getattr(self, "_widest_scene", 0), 2))   # no band is wider than the widest scene
        off = np.zeros(B + 1, np.int32)
        _chk(lib().teb_amd_compute_h_signatures_per_scene(self._h, prescaler, _abi._ptr(out, C.c_double), out.size, _abi._ptr(off, C.c_int32),
                                                          C.byref(n)), "teb_amd_compute_h_signatures_per_scene")
        return [out[off[b]:off[b + 1]].copy() for b in range(self.count)]

    def _best_per_scene(self, best, what):
        if best is None:
            return None
        a = _abi.i32(best)
        if len(a) != self.scene_count():
            raise ValueError("%s: %d entries for %d scenes" % (what, len(a), self.scene_count()))
        return a

    def filter_equivalence_classes_per_scene(self, threshold=0.1, best=None, max_number_plans_in_current_class=1):
        """filter_equivalence_classes over the bands of every scene on the signatures of the last h_signatures_per_scene call:
        (keep, valid, reasonable), each [B]. best: per scene a band of that scene (visited first; its class is remembered for the
        scene) or -1, None = none."""
        self._sync_count()
        bp = self._best_per_scene(best, "filter_equivalence_classes_per_scene")
        keep = np.zeros(self.count, np.int32); valid = np.zeros(self.count, np.int32); reas = np.zeros(self.count, np.int32)
        I = lambda a: _abi._ptr(a, C.c_int32)
        _chk(lib().teb_amd_filter_equivalence_classes_per_scene(self._h, threshold, I(bp), max_number_plans_in_current_class, I(keep), I(valid),
                                                                I(reas)), "teb_amd_filter_equivalence_classes_per_scene")
        return keep, valid, reas

    def filter_detours_per_scene(self, keep, best, params=None):
        """filter_detours scene by scene (best: per scene a band of that scene or -1): returns the new keep array."""
        p = params if params is not None else self.cfg.hcp_params()
        bp = self._best_per_scene(best, "filter_detours_per_scene")
        keep = _abi.i32(keep).copy()
        _chk(lib().teb_amd_filter_detours_per_scene(self._h, C.byref(p), _abi._ptr(bp, C.c_int32), _abi._ptr(keep, C.c_int32)),
             "teb_amd_filter_detours_per_scene")
        return keep

    def band_scenes(self):
        """[B] scene of every resident band (the map of set_band_scenes as compaction and exploration moved and extended it)."""
        self._sync_count()
        a = np.zeros(max(self.count, 1), np.int32); n = C.c_int32(0)
        _chk(lib().teb_amd_get_band_scenes(self._h, _abi._ptr(a, C.c_int32), len(a), C.byref(n)), "teb_amd_get_band_scenes")
        return a[:n.value].copy()

    def _per_scene(self, what, name, a, width=None):
        """`a` as a contiguous array with one row per scene set by set_scenes, or None; ValueError before the library is entered."""
        ns = getattr(self, "_n_scenes", 0)
        if a is None:
            return None
        if len(a) != ns:
            raise ValueError("%s: %d %s for %d scenes" % (what, len(a), name, ns))
        if width is None:
            return _abi.i32(a)
        out = np.ascontiguousarray(np.asarray(a, np.float64).reshape(ns, -1))
        if out.shape[1] != width:
            raise ValueError("%s: %s have %d values per scene, not %d" % (what, name, out.shape[1], width))
        return out

    def explore_candidates_per_scene(self, starts, goals, dist_to_obst=None, start_vels=None, free_goal_vel=False, best=None,
                                     unit_samples=None, max_paths=0, params=None, initial_plans=None):
        """Fleet mode: exploreEquivalenceClassesAndInitTebs of every scene with its own start / goal / start velocity / best band /
        unit samples / initial plan ((x, y, yaw) arrays or None per scene): dict(n_total, n_bands [n_scenes], n_vertices, n_paths,
        initial_plan_teb - the position among the bands of the scene, or -1). New bands are appended to the batch."""
        dist_to_obst = self.cfg.obstacles.min_obstacle_dist if dist_to_obst is None else dist_to_obst
        return self._explore_fleet("explore_candidates_per_scene", float(dist_to_obst), starts, goals, start_vels, free_goal_vel, best,
                                   unit_samples, max_paths, params, initial_plans)

    def explore_candidates_per_class(self, starts, goals, start_vels=None, free_goal_vel=False, best=None, unit_samples=None, max_paths=0,
                                     params=None, initial_plans=None):
        """explore_candidates_per_scene where every scene reads min_obstacle_dist (the graph's dist_to_obst), max_vel_x, max_vel_theta,
        acc_lim_x, min_samples and weight_viapoint from the configuration of its robot class (set_scene_configs; without a map the
        handle's configuration). params stays one per call."""
        return self._explore_fleet("explore_candidates_per_class", None, starts, goals, start_vels, free_goal_vel, best, unit_samples,
                                   max_paths, params, initial_plans)

    def _explore_fleet(self, what, dist_to_obst, starts, goals, start_vels, free_goal_vel, best, unit_samples, max_paths, params, initial_plans):
        ns = getattr(self, "_n_scenes", 0)
        p = params if params is not None else self.cfg.hcp_params()
        if starts is None or goals is None:
            raise ValueError(what + ": starts and goals are required")
        st = self._per_scene(what, "starts", starts, 3); gl = self._per_scene(what, "goals", goals, 3)
        sv = self._per_scene(what, "start velocities", start_vels, 3)
        bp = self._per_scene(what, "best bands", best)
        us = self._per_scene(what, "unit sample rows", unit_samples, 2 * max(int(p.roadmap_graph_no_samples), 0))
        pc = px = py = pyaw = None
        if initial_plans is not None:
            if len(initial_plans) != ns:
                raise ValueError("%s: %d initial plans for %d scenes" % (what, len(initial_plans), ns))
            pc = _abi.i32([0 if q is None else len(q[0]) for q in initial_plans])
            cat = lambda j: _abi.f64(np.concatenate([np.asarray(q[j], np.float64).ravel() for q in initial_plans if q is not None] + [np.zeros(1)]))
            px, py, pyaw = cat(0), cat(1), cat(2)
        nt = C.c_int32(0)
        nb = np.zeros(max(ns, 1), np.int32); nv = nb.copy(); npth = nb.copy(); ipt = np.full(max(ns, 1), -1, np.int32)
        D = lambda a: _abi._ptr(a, C.c_double)
        I = lambda a: _abi._ptr(a, C.c_int32)
        tail = (D(sv), int(bool(free_goal_vel)), I(bp), D(us), int(max_paths), C.byref(nt), I(nb), I(nv), I(npth), I(pc), D(px), D(py), D(pyaw),
                I(ipt))
        if dist_to_obst is None:
            _chk(lib().teb_amd_explore_candidates_per_class(self._h, C.byref(p), D(st), D(gl), *tail), "teb_amd_explore_candidates_per_class")
        else:
            _chk(lib().teb_amd_explore_candidates_per_scene(self._h, C.byref(p), D(st), D(gl), dist_to_obst, *tail),
                 "teb_amd_explore_candidates_per_scene")
        self.count = nt.value
        return dict(n_total=nt.value, n_bands=nb[:ns].copy(), n_vertices=nv[:ns].copy(), n_paths=npth[:ns].copy(),
                    initial_plan_teb=ipt[:ns].copy())

    def exploration_graph_per_scene(self, s):
        """(vertices [N, 2], adjacency [N, N] uint8) of scene s in the last explore_candidates_per_scene call (N = 0: no graph)."""
        nv = C.c_int32(0)
        _chk(lib().teb_amd_get_exploration_graph_per_scene(self._h, int(s), None, None, None, 0, C.byref(nv)),
             "teb_amd_get_exploration_graph_per_scene")
        N = nv.value
        vx = np.zeros(max(N, 1)); vy = np.zeros(max(N, 1)); adj = np.zeros((max(N, 1), max(N, 1)), np.uint8)
        if N:
            _chk(lib().teb_amd_get_exploration_graph_per_scene(self._h, int(s), _abi._ptr(vx, C.c_double), _abi._ptr(vy, C.c_double),
                                                               adj.ctypes.data_as(C.POINTER(C.c_ubyte)), N, C.byref(nv)),
                 "teb_amd_get_exploration_graph_per_scene")
        return np.stack([vx[:N], vy[:N]], 1), adj[:N, :N]

    def compact_bands_per_scene(self, keep, best=None):
        """Keeps the bands with keep[b] != 0, every scene's best band first among the bands of its scene: (n_kept, new_best [n_scenes])."""
        bp = self._per_scene("compact_bands_per_scene", "best bands", best)
        keep = _abi.i32(keep)
        ns = getattr(self, "_n_scenes", 0)
        nk = C.c_int32(0); nb = np.full(max(ns, 1), -1, np.int32)
        _chk(lib().teb_amd_compact_bands_per_scene(self._h, _abi._ptr(keep, C.c_int32), _abi._ptr(bp, C.c_int32), C.byref(nk),
                                                   _abi._ptr(nb, C.c_int32)), "teb_amd_compact_bands_per_scene")
        self.count = nk.value
        return nk.value, nb[:ns].copy()

    def debug_set_explore_quota(self, q):
        _chk(lib().teb_amd_debug_set_explore_quota(self._h, int(q)), "teb_amd_debug_set_explore_quota")

    # -- both ends of a fleet tick per scene (include/teb_amd.h) ----------------------------------------------
    def set_costmaps(self, costmaps):
        """One grid per scene: a list of objects with cells (uint8 [size_y, size_x]), resolution, origin_x, origin_y (oracle.oracle_py.Costmap
        or alike); grid s belongs to scene s. An empty list drops the set. The single costmap of set_costmap is not touched."""
        cms = list(costmaps)
        n = len(cms)
        if n == 0:
            _chk(lib().teb_amd_set_costmaps(self._h, 0, None, None, None, None, None, None), "teb_amd_set_costmaps")
            return
        grids = [np.ascontiguousarray(c.cells, dtype=np.uint8) for c in cms]
        for g in grids:
            if g.ndim != 2:
                raise ValueError("set_costmaps: cells must be [size_y, size_x]")
        cells = np.concatenate([g.reshape(-1) for g in grids]) if sum(g.size for g in grids) else np.zeros(1, np.uint8)
        sx = _abi.i32([g.shape[1] for g in grids]); sy = _abi.i32([g.shape[0] for g in grids])
        res = _abi.f64([float(c.resolution) for c in cms]); ox = _abi.f64([float(c.origin_x) for c in cms]); oy = _abi.f64([float(c.origin_y) for c in cms])
        D = lambda a: _abi._ptr(a, C.c_double)
        _chk(lib().teb_amd_set_costmaps(self._h, n, cells.ctypes.data_as(C.c_void_p), _abi._ptr(sx, C.c_int32), _abi._ptr(sy, C.c_int32), D(res), D(ox),
                                        D(oy)), "teb_amd_set_costmaps")

    def set_scenes_from_costmaps(self, robot_poses, costmap_obstacles_behind_robot_dist, custom=None, vias=None):
        """set_scenes with table s = set_obstacles_from_costmap's rows of grid s (set_costmaps) and robot_poses[s] ++ the rows of custom[s]
        (ObstacleTable or None entries; None = no custom rows anywhere). Returns (n [n_scenes], [(xs, ys)] per scene): the number of cell
        obstacles of every scene and their centres in table order."""
        poses = np.ascontiguousarray(np.asarray(robot_poses, np.float64).reshape(-1, 3))
        ns = len(poses)
        tables = [t if t is not None else _abi.ObstacleTable() for t in (custom if custom is not None else [None] * ns)]
        if len(tables) != ns or (vias is not None and len(vias) != ns):
            raise ValueError("set_scenes_from_costmaps: %d robot poses, %d custom tables, %s via-point lists" % (ns, len(tables), None if vias is None else len(vias)))
        p = _abi.pack_scenes(tables, vias)
        cap = max(int(self.max_obstacles), 1)
        n = np.zeros(ns, np.int32); xs = np.zeros(cap); ys = np.zeros(cap)
        D = lambda a: _abi._ptr(a, C.c_double)
        _chk(lib().teb_amd_set_scenes_from_costmaps(self._h, ns, D(poses), float(costmap_obstacles_behind_robot_dist), p.obstacles,
                                                    _abi._ptr(p.via_count, C.c_int32), D(p.via_x), D(p.via_y), _abi._ptr(n, C.c_int32), D(xs), D(ys), cap),
             "teb_amd_set_scenes_from_costmaps")
        off = np.concatenate([[0], np.cumsum(n)])
        self._widest_scene = max(int(n[s]) + len(tables[s]) for s in range(ns))
        self._n_scenes = ns
        return n.copy(), [(xs[off[s]:off[s + 1]].copy(), ys[off[s]:off[s + 1]].copy()) for s in range(ns)]

    def set_scenes_from_costmap_polygons(self, robot_poses, costmap_obstacles_behind_robot_dist, tile_cells=8, custom=None, vias=None, return_tables=True):
        """set_scenes with table s = set_obstacles_from_costmap_polygons' rows of grid s (set_costmaps), robot_poses[s] and the scene's own
        tile size ++ the rows of custom[s] (ObstacleTable or None entries; None = no custom rows anywhere). tile_cells: an int for every
        scene or one per scene (sparse maps want 1, structured maps 8: DESIGN.md section 7). Returns the converted rows of every scene
        as a list of ObstacleTable, in table order; return_tables = False skips the out arrays and the host tables and returns the number
        of converted rows per scene (what FleetHomotopyClassPlanner.plan wants: it does not look at the rows)."""
        poses = np.ascontiguousarray(np.asarray(robot_poses, np.float64).reshape(-1, 3))
        ns = len(poses)
        tiles = _abi.i32([int(tile_cells)] * ns if np.ndim(tile_cells) == 0 else [int(t) for t in tile_cells])
        tables = [t if t is not None else _abi.ObstacleTable() for t in (custom if custom is not None else [None] * ns)]
        if len(tables) != ns or len(tiles) != ns or (vias is not None and len(vias) != ns):
            raise ValueError("set_scenes_from_costmap_polygons: %d robot poses, %d tile sizes, %d custom tables, %s via-point lists"
                             % (ns, len(tiles), len(tables), None if vias is None else len(vias)))
        p = _abi.pack_scenes(tables, vias)
        cap_o = max(int(self.max_obstacles), 1)
        cap_p = 2 * cap_o + int(self.max_obstacle_vertices)   # a successful call fits: <= 2 vertices per point / line row
        n_o = np.zeros(ns, np.int32); n_p = np.zeros(ns, np.int32)
        off = xs = ys = None
        if return_tables:
            off = np.zeros(cap_o + 1, np.int32); xs = np.zeros(cap_p); ys = np.zeros(cap_p)
        D = lambda a: _abi._ptr(a, C.c_double)
        I = lambda a: _abi._ptr(a, C.c_int32)
        _chk(lib().teb_amd_set_scenes_from_costmap_polygons(self._h, ns, D(poses), float(costmap_obstacles_behind_robot_dist), I(tiles), p.obstacles,
                                                            I(p.via_count), D(p.via_x), D(p.via_y), I(n_o), I(n_p), I(off), D(xs), D(ys), cap_o, cap_p),
             "teb_amd_set_scenes_from_costmap_polygons")
        r0 = np.concatenate([[0], np.cumsum(n_o)])
        self._widest_scene = max(int(n_o[s]) + len(tables[s]) for s in range(ns))
        self._n_scenes = ns
        if not return_tables:
            return n_o.copy()
        out = []
        for s in range(ns):
            o = off[r0[s]:r0[s + 1] + 1]
            out.append(_abi.ObstacleTable.from_polygon_list(o - o[0], xs[o[0]:o[-1]], ys[o[0]:o[-1]]))
        return out

    def is_trajectory_feasible_per_scene(self, bands, footprint, inscribed_radius, min_resolution_collision_check_angular=3.141592653589793,
                                         look_ahead_idx=-1, feasibility_check_lookahead_distance=-1.0):
        """isTrajectoryFeasible of band bands[s] (a band of scene s; negative: none) against grid s of set_costmaps, one launch:
        (feasible [n_scenes], first_infeasible [n_scenes]) as int32 - 1 / 0, and -1 in both for a scene without a band."""
        bd = self._per_scene("is_trajectory_feasible_per_scene", "bands", bands)
        if bd is None:
            raise ValueError("is_trajectory_feasible_per_scene: bands are required")
        fx = _abi.f64([p[0] for p in footprint]); fy = _abi.f64([p[1] for p in footprint])
        ok = np.zeros(max(len(bd), 1), np.int32); first = np.zeros(max(len(bd), 1), np.int32)
        _chk(lib().teb_amd_is_trajectory_feasible_per_scene(self._h, _abi._ptr(bd, C.c_int32), len(footprint), _abi._ptr(fx, C.c_double),
                                                            _abi._ptr(fy, C.c_double), float(inscribed_radius), float(min_resolution_collision_check_angular),
                                                            int(look_ahead_idx), float(feasibility_check_lookahead_distance), _abi._ptr(ok, C.c_int32),
                                                            _abi._ptr(first, C.c_int32)), "teb_amd_is_trajectory_feasible_per_scene")
        return ok[:len(bd)].copy(), first[:len(bd)].copy()

    def update_and_prune_per_scene(self, new_starts=None, new_goals=None, min_samples=3, start_vels=None, has_start_vel=None):
        """updateAndPruneTEB of every band with the start / goal of its scene ([n_scenes, 3] or None), one launch; start_vels [n_scenes, 3]:
        the bands of the scenes with has_start_vel[s] (None: all) get that fixed start velocity (set_velocity_start(v, True, b))."""
        what = "update_and_prune_per_scene"
        st = self._per_scene(what, "starts", new_starts, 3); gl = self._per_scene(what, "goals", new_goals, 3)
        sv = self._per_scene(what, "start velocities", start_vels, 3)
        hv = self._per_scene(what, "start velocity flags", has_start_vel)
        D = lambda a: _abi._ptr(a, C.c_double)
        _chk(lib().teb_amd_update_and_prune_per_scene(self._h, D(st), D(gl), int(min_samples), D(sv), _abi._ptr(hv, C.c_int32)),
             "teb_amd_update_and_prune_per_scene")

    def update_and_prune_per_class(self, new_starts=None, new_goals=None, start_vels=None, has_start_vel=None):
        """update_and_prune_per_scene where every band is pruned with min_samples of its scene's robot class."""
        what = "update_and_prune_per_class"
        st = self._per_scene(what, "starts", new_starts, 3); gl = self._per_scene(what, "goals", new_goals, 3)
        sv = self._per_scene(what, "start velocities", start_vels, 3)
        hv = self._per_scene(what, "start velocity flags", has_start_vel)
        D = lambda a: _abi._ptr(a, C.c_double)
        _chk(lib().teb_amd_update_and_prune_per_class(self._h, D(st), D(gl), D(sv), _abi._ptr(hv, C.c_int32)), "teb_amd_update_and_prune_per_class")

    def is_trajectory_feasible_per_class(self, bands, specs, spec_of_scene=None):
        """is_trajectory_feasible_per_scene with a spec per scene. specs: a list of dict(footprint=[(x, y), ...], inscribed_radius=,
        min_resolution_collision_check_angular=pi, look_ahead_idx=-1, feasibility_check_lookahead_distance=-1.0); spec_of_scene
        [n_scenes] picks one for every scene, None: the spec of the scene's robot class (one spec per class of the map, one without a
        map). (feasible [n_scenes], first_infeasible [n_scenes]) as int32."""
        what = "is_trajectory_feasible_per_class"
        bd = self._per_scene(what, "bands", bands)
        if bd is None:
            raise ValueError(what + ": bands are required")
        specs = list(specs)
        if not specs:
            raise ValueError(what + ": needs at least one spec")
        so = self._per_scene(what, "spec entries", spec_of_scene)
        if so is not None and len(so) and (so.min() < 0 or so.max() >= len(specs)):
            raise ValueError("%s: spec_of_scene does not fit the %d specs" % (what, len(specs)))
        arr = (FeasibilitySpec * len(specs))()
        keep = []   # the footprint arrays live until the call returns
        for k, q in enumerate(specs):
            fx = _abi.f64([v[0] for v in q["footprint"]]); fy = _abi.f64([v[1] for v in q["footprint"]])
            keep.append((fx, fy))
            arr[k] = FeasibilitySpec(len(q["footprint"]), _abi._ptr(fx, C.c_double), _abi._ptr(fy, C.c_double), float(q["inscribed_radius"]),
                                     float(q.get("min_resolution_collision_check_angular", 3.141592653589793)), int(q.get("look_ahead_idx", -1)),
                                     float(q.get("feasibility_check_lookahead_distance", -1.0)))
        ok = np.zeros(max(len(bd), 1), np.int32); first = np.zeros(max(len(bd), 1), np.int32)
        _chk(lib().teb_amd_is_trajectory_feasible_per_class(self._h, _abi._ptr(bd, C.c_int32), len(specs), arr, _abi._ptr(so, C.c_int32),
                                                            _abi._ptr(ok, C.c_int32), _abi._ptr(first, C.c_int32)),
             "teb_amd_is_trajectory_feasible_per_class")
        return ok[:len(bd)].copy(), first[:len(bd)].copy()

    def velocity_commands(self, bands, look_ahead_poses=1, prevent_look_ahead_poses_near_goal=0):
        """getVelocityCommand of many bands after one launch and one download: (ok [n] bool, cmd [n, 3]); a negative band: False, zeros."""
        bd = _abi.i32(bands)
        n = len(bd)
        cmd = np.zeros((max(n, 1), 3)); ok = np.zeros(max(n, 1), np.int32)
        _chk(lib().teb_amd_get_velocity_commands(self._h, n, _abi._ptr(bd, C.c_int32), int(look_ahead_poses), int(prevent_look_ahead_poses_near_goal),
                                                 _abi._ptr(cmd, C.c_double), _abi._ptr(ok, C.c_int32)), "teb_amd_get_velocity_commands")
        return ok[:n].astype(bool), cmd[:n].copy()

    # -- local plan windows per robot from resident global plans (include/teb_amd.h) ---------------------------
    def set_global_plans(self, plans, begin=None):
        """plans[r] = (x, y, yaw) arrays of robot r's global plan in the plan frame (None or empty arrays: no plan); begin [n] or None =
        zeros: the pruning cursors. An empty list drops the set."""
        plans = [(_abi.f64([]),) * 3 if p is None else tuple(_abi.f64(a).reshape(-1) for a in p) for p in plans]
        n = len(plans)
        if n == 0:
            _chk(lib().teb_amd_set_global_plans(self._h, 0, None, None, None, None, None), "teb_amd_set_global_plans")
            self._plan_counts = None
            return
        for p in plans:
            if len(p) != 3 or not (len(p[0]) == len(p[1]) == len(p[2])):
                raise ValueError("set_global_plans: a plan is three arrays (x, y, yaw) of one length")
        cnt = _abi.i32([len(p[0]) for p in plans])
        cat = lambda k: _abi.f64(np.concatenate([p[k] for p in plans])) if cnt.sum() else _abi.f64([0.0])
        x, y, yaw = cat(0), cat(1), cat(2)
        bg = None if begin is None else _abi.i32(begin)
        if bg is not None and len(bg) != n:
            raise ValueError("set_global_plans: %d cursors for %d plans" % (len(bg), n))
        D = lambda a: _abi._ptr(a, C.c_double)
        _chk(lib().teb_amd_set_global_plans(self._h, n, _abi._ptr(cnt, C.c_int32), D(x), D(y), D(yaw), _abi._ptr(bg, C.c_int32)),
             "teb_amd_set_global_plans")
        self._plan_counts = cnt.copy()

    def plan_cursors(self):
        """The pruning cursors of the resident plans [n]."""
        if self._plan_counts is None:
            raise ValueError("plan_cursors: no global plans set")
        b = np.zeros(len(self._plan_counts), np.int32)
        _chk(lib().teb_amd_get_plan_cursors(self._h, _abi._ptr(b, C.c_int32)), "teb_amd_get_plan_cursors")
        return b

    def plan_windows(self, robot_poses, dist_thresholds, params=None, plan_to_global=None, capacity_window=None, capacity_via=None):
        """teb_amd_plan_windows for the resident plans: robot_poses [n, 3] in the global frame, dist_thresholds [n] (the reference's
        0.85 * max(size_x, size_y) * resolution / 2), plan_to_global [n, 5] = (cos, sin, tx, ty, yaw_tf) or None = identity, params a
        _abi.PlanWindowParams or None = defaults. Returns a dict: window_count, goal_idx, cursor, pruned, via_count [n] int32; goal,
        global_goal [n, 3]; offset, via_offset [n + 1]; win_x, win_y, win_yaw, via_x, via_y concatenated; windows [n] = (x, y, yaw)
        per robot and vias [n] = [(x, y), ...] per robot. The capacities default to what always fits."""
        if self._plan_counts is None:
            raise ValueError("plan_windows: no global plans set")
        n = len(self._plan_counts)
        poses = np.ascontiguousarray(np.asarray(robot_poses, np.float64).reshape(-1, 3))
        thr = _abi.f64(dist_thresholds).reshape(-1)
        tf = None if plan_to_global is None else np.ascontiguousarray(np.asarray(plan_to_global, np.float64).reshape(-1, 5))
        if len(poses) != n or len(thr) != n or (tf is not None and len(tf) != n):
            raise ValueError("plan_windows: %d plans, %d poses, %d thresholds, %s transforms" % (n, len(poses), len(thr), None if tf is None else len(tf)))
        cap = int(self._plan_counts.sum()) + n
        cw = cap if capacity_window is None else int(capacity_window)
        cv = cap if capacity_via is None else int(capacity_via)
        I = lambda a: _abi._ptr(a, C.c_int32)
        D = lambda a: _abi._ptr(a, C.c_double)
        o = {k: np.zeros(n, np.int32) for k in ("window_count", "goal_idx", "cursor", "pruned", "via_count")}
        o["goal"] = np.zeros((n, 3)); o["global_goal"] = np.zeros((n, 3))
        o["offset"] = np.zeros(n + 1, np.int32); o["via_offset"] = np.zeros(n + 1, np.int32)
        for k in ("win_x", "win_y", "win_yaw"):
            o[k] = np.zeros(max(cw, 1))
        for k in ("via_x", "via_y"):
            o[k] = np.zeros(max(cv, 1))
        rc = lib().teb_amd_plan_windows(self._h, n, C.byref(params) if params is not None else None, D(poses), D(tf), D(thr), I(o["window_count"]),
                                        I(o["goal_idx"]), I(o["cursor"]), I(o["pruned"]), D(o["goal"]), D(o["global_goal"]), I(o["via_count"]),
                                        I(o["offset"]), D(o["win_x"]), D(o["win_y"]), D(o["win_yaw"]), cw, I(o["via_offset"]), D(o["via_x"]),
                                        D(o["via_y"]), cv)
        if rc == _abi.ERR_CAPACITY and (capacity_window is not None or capacity_via is not None):
            o["status"] = rc   # the caller chose the capacities: counts and per-robot values are delivered, the arrays untouched
            return o
        _chk(rc, "teb_amd_plan_windows")
        o["status"] = rc
        off, voff = o["offset"], o["via_offset"]
        for k in ("win_x", "win_y", "win_yaw"):
            o[k] = o[k][:off[n]]
        for k in ("via_x", "via_y"):
            o[k] = o[k][:voff[n]]
        o["windows"] = [(o["win_x"][off[r]:off[r + 1]].copy(), o["win_y"][off[r]:off[r + 1]].copy(), o["win_yaw"][off[r]:off[r + 1]].copy())
                        for r in range(n)]
        o["vias"] = [list(zip(o["via_x"][voff[r]:voff[r + 1]].tolist(), o["via_y"][voff[r]:voff[r + 1]].tolist())) for r in range(n)]
        return o

    # -- state ---------------------------------------------------------------------------------------
    def upload(self, batch):
        bs = batch.c_struct()
        _chk(lib().teb_amd_upload_tebs(self._h, C.byref(bs)), "teb_amd_upload_tebs")
        self.count = batch.count

    def download(self, batch):
        bs = batch.c_struct()
        _chk(lib().teb_amd_download_tebs(self._h, C.byref(bs)), "teb_amd_download_tebs")
        return batch

    def snapshot(self):
        _chk(lib().teb_amd_snapshot_state(self._h), "teb_amd_snapshot_state")

    def restore(self):
        _chk(lib().teb_amd_restore_state(self._h), "teb_amd_restore_state")

    # -- hot path --------------------------------------------------------------------------------------
    def optimize(self, inner, outer, compute_cost=False, obst_cost_scale=1.0, viapoint_cost_scale=1.0,
                 alternative_time_cost=False):
        _chk(lib().teb_amd_optimize_batch(self._h, inner, outer, int(compute_cost), float(obst_cost_scale),
                                          float(viapoint_cost_scale), int(alternative_time_cost)),
             "teb_amd_optimize_batch")

    def optimize_per_class(self, inner, outer, compute_cost=False):
        """Fleet mode: optimize where band b's cost takes selection_obst_cost_scale, selection_viapoint_cost_scale and
        selection_alternative_time_cost from the configuration of its scene's robot class."""
        _chk(lib().teb_amd_optimize_batch_per_class(self._h, int(inner), int(outer), int(bool(compute_cost))), "teb_amd_optimize_batch_per_class")

    def synchronize(self):
        _chk(lib().teb_amd_synchronize(self._h), "teb_amd_synchronize")

    def results(self):
        res = _abi.ResultsHost(self.count)
        rs = res.c_struct()
        _chk(lib().teb_amd_get_results(self._h, C.byref(rs)), "teb_amd_get_results")
        return res

    def set_iteration_log(self, enable=True):
        """Opt-in per-iteration log of the LM loop (g2o's verbose line as data, src/optimal_planner.cpp:384)."""
        _chk(lib().teb_amd_set_iteration_log(self._h, int(bool(enable))), "teb_amd_set_iteration_log")

    PHASES = ("autoresize", "graph side data", "linearize", "H backup", "solve", "update + evaluate", "accept / restore")

    def set_phase_log(self, enable=True):
        """Phase split of the product kernel (include/teb_amd_debug.h): shader cycles per phase of every band's workgroup."""
        L = lib()
        L.teb_amd_set_phase_log.argtypes = [C.c_void_p, C.c_int32]
        _chk(L.teb_amd_set_phase_log(self._h, int(bool(enable))), "teb_amd_set_phase_log")

    def phase_log(self):
        """[B, 9] shader cycles of the last optimize(): the seven PHASES, a spare slot, the whole workgroup."""
        L = lib()
        L.teb_amd_get_phase_log.argtypes = [C.c_void_p, _abi.p_f64, C.c_int32, _abi.p_i32]
        self._sync_count()
        out = np.zeros((max(self.count, 1), 9)); nb = C.c_int32(0)
        _chk(L.teb_amd_get_phase_log(self._h, _abi._ptr(out, C.c_double), self.count, C.byref(nb)), "teb_amd_get_phase_log")
        return out[:nb.value]

    def iteration_log(self, b, capacity_rows=256):
        """[iterations, 4] of band b after the last optimize(): chi2 after the iteration, lambda after it, damping trials, pose count."""
        rows = np.zeros((int(capacity_rows), 4))
        n = C.c_int32(0)
        _chk(lib().teb_amd_get_iteration_log(self._h, int(b), _abi._ptr(rows, C.c_double), int(capacity_rows), C.byref(n)),
             "teb_amd_get_iteration_log")
        return rows[:n.value].copy()

    def select_best(self, last_best=-1, initial_plan=-1):
        best = C.c_int32(-1)
        cost = C.c_double(0)
        _chk(lib().teb_amd_select_best(self._h, last_best, initial_plan, C.byref(best), C.byref(cost)),
             "teb_amd_select_best")
        return best.value, cost.value

    def select_best_distributed(self, comm, global_offset, last_best_global=-1, initial_plan_global=-1):
        """selectBestTeb over the candidates of all ranks of `comm` (parallel.RcclComm): (best_global, scaled cost, owner_rank), the
        same on every rank. One 16-byte-per-rank ncclAllGather inside libteb_amd.so."""
        best = C.c_int32(-1); cost = C.c_double(0); owner = C.c_int32(-1)
        _chk(lib().teb_amd_select_best_distributed(self._h, comm._c, int(global_offset), int(last_best_global), int(initial_plan_global),
                                                   C.byref(best), C.byref(cost), C.byref(owner)), "teb_amd_select_best_distributed")
        return best.value, cost.value, owner.value

    def broadcast_band(self, comm, owner_rank, local_index, capacity=None):
        """The winner's strip from its owner to every rank: (x, y, theta, dt) as host arrays."""
        cap = int(capacity or self.max_poses)
        n = C.c_int32(0)
        x = np.zeros(cap); y = np.zeros(cap); th = np.zeros(cap); dt = np.zeros(cap)
        P = lambda a: _abi._ptr(a, C.c_double)
        _chk(lib().teb_amd_broadcast_band(self._h, comm._c, int(owner_rank), int(local_index), cap, C.byref(n), P(x), P(y), P(th), P(dt)),
             "teb_amd_broadcast_band")
        return x[:n.value].copy(), y[:n.value].copy(), th[:n.value].copy(), dt[:max(n.value - 1, 0)].copy()

    def last_kernel_ms(self):
        ms = C.c_float(0)
        _chk(lib().teb_amd_last_kernel_ms(self._h, C.byref(ms)), "teb_amd_last_kernel_ms")
        return ms.value

    def last_shader_clock_mhz(self):
        """shader clock of the last optimise kernel (cycle counter / real-time counter of its first workgroup)"""
        L = lib()
        L.teb_amd_last_shader_clock_mhz.argtypes = [C.c_void_p, _abi.p_f64]
        v = C.c_double(0)
        _chk(L.teb_amd_last_shader_clock_mhz(self._h, C.byref(v)), "teb_amd_last_shader_clock_mhz")
        return v.value

    def last_launch_info(self):
        """(distance helpers per band of the last optimize(), solver helpers per band, repeated on one CU per band after a timeout)"""
        a = C.c_int32(0); k = C.c_int32(0); b = C.c_int32(0)
        _chk(lib().teb_amd_last_launch_info(self._h, C.byref(a), C.byref(k), C.byref(b)), "teb_amd_last_launch_info")
        return a.value, k.value, bool(b.value)

    def multi_cu_backoff(self):
        """(launches still paused, current pause length) of the distance helpers' back-off (teb_amd_multi_cu_backoff)"""
        a = C.c_int32(0); k = C.c_int32(0)
        _chk(lib().teb_amd_multi_cu_backoff(self._h, C.byref(a), C.byref(k)), "teb_amd_multi_cu_backoff")
        return a.value, k.value

    def last_instantiation(self):
        """(layout, Jacobian mode, scene kind) of the kernel instantiation the last optimize() launched (teb_amd_debug_last_instantiation)"""
        a = C.c_int32(-1); j = C.c_int32(-1); k = C.c_int32(-1)
        _chk(lib().teb_amd_debug_last_instantiation(self._h, C.byref(a), C.byref(j), C.byref(k)), "teb_amd_debug_last_instantiation")
        return a.value, j.value, k.value

    def last_config_profile(self):
        """Which kernel the last optimize() ran: 1 = specialised on the TebConfig defaults, 2 = the same folds except via-points and the
        holonomic choice (*_WIDE kinds), 3 = every cost-term flag at run time (*_LIGHT kinds), 0 = the generic instantiation (teb_amd_options_t::generic_config_path forces it)"""
        L = lib()
        L.teb_amd_debug_last_config_profile.argtypes = [C.c_void_p, _abi.p_i32]
        v = C.c_int32(0)
        _chk(L.teb_amd_debug_last_config_profile(self._h, C.byref(v)), "teb_amd_debug_last_config_profile")
        return int(v.value)

    @staticmethod
    def build_info():
        """What the loaded binary was built from: (kernel hash, source hash, variant defines, threads per workgroup of the optimise
        kernel) - teb_amd_debug_build_info, include/teb_amd_debug.h"""
        L = lib()
        L.teb_amd_debug_build_info.argtypes = [C.c_char_p, C.c_int32, C.c_char_p, C.c_int32, C.c_char_p, C.c_int32, _abi.p_i32]
        kb = C.create_string_buffer(64); hb = C.create_string_buffer(64); db = C.create_string_buffer(1024); t = C.c_int32(0)
        _chk(L.teb_amd_debug_build_info(kb, 64, hb, 64, db, 1024, C.byref(t)), "teb_amd_debug_build_info")
        return kb.value.decode(), hb.value.decode(), db.value.decode(), t.value

    @staticmethod
    def rtc_stats():
        """run-time compiled instantiations of this process: (ready, compiling, failed, compile seconds of the last one, last error)"""
        L = lib()
        L.teb_amd_debug_rtc_stats.argtypes = [_abi.p_i32, _abi.p_i32, _abi.p_i32, _abi.p_f64, C.c_char_p, C.c_int32]
        r = C.c_int32(0); w = C.c_int32(0); f = C.c_int32(0); s = C.c_double(0); buf = C.create_string_buffer(4096)
        _chk(L.teb_amd_debug_rtc_stats(C.byref(r), C.byref(w), C.byref(f), C.byref(s), buf, 4096), "teb_amd_debug_rtc_stats")
        return r.value, w.value, f.value, s.value, buf.value.decode(errors="replace")

    def capacity(self):
        a = C.c_int32(0)
        b = C.c_int32(0)
        _chk(lib().teb_amd_capacity(self._h, C.byref(a), C.byref(b)), "teb_amd_capacity")
        return a.value, b.value

    # -- producers / consumers of the device-resident strips ----------------------
    @staticmethod
    def _opt3(v):
        return None if v is None else _abi._ptr(_abi.f64(v), C.c_double)

    @staticmethod
    def _opt1(v):
        return None if v is None else _abi._ptr(_abi.f64([v]), C.c_double)

    def _sync_count(self):
        c = C.c_int32(0)
        _chk(lib().teb_amd_get_pose_counts(self._h, None, C.byref(c)), "teb_amd_get_pose_counts")
        self.count = c.value

    def init_trajectory_line(self, b, start, goal, diststep, max_vel_x, min_samples, guess_backwards_motion=False):
        _chk(lib().teb_amd_init_trajectory_line(self._h, b, self._opt3(start), self._opt3(goal), diststep, max_vel_x, min_samples,
                                                int(guess_backwards_motion)), "teb_amd_init_trajectory_line")
        self._sync_count()

    def init_trajectory_plan(self, b, px, py, pyaw, max_vel_x, max_vel_theta, estimate_orient, min_samples,
                             guess_backwards_motion=False):
        px = _abi.f64(px); py = _abi.f64(py); pyaw = _abi.f64(pyaw)
        P = lambda a: _abi._ptr(a, C.c_double)
        _chk(lib().teb_amd_init_trajectory_plan(self._h, b, len(px), P(px), P(py), P(pyaw), max_vel_x, max_vel_theta,
                                                int(estimate_orient), min_samples, int(guess_backwards_motion)),
             "teb_amd_init_trajectory_plan")
        self._sync_count()

    def init_trajectory_path(self, b, px, py, max_vel_x, max_vel_theta, max_acc_x=None, start_orientation=None,
                             goal_orientation=None, min_samples=3, guess_backwards_motion=False):
        px = _abi.f64(px); py = _abi.f64(py)
        P = lambda a: _abi._ptr(a, C.c_double)
        _chk(lib().teb_amd_init_trajectory_path(self._h, b, len(px), P(px), P(py), max_vel_x, max_vel_theta, self._opt1(max_acc_x),
                                                self._opt1(start_orientation), self._opt1(goal_orientation), min_samples,
                                                int(guess_backwards_motion)), "teb_amd_init_trajectory_path")
        self._sync_count()

    def update_and_prune(self, new_start=None, new_goal=None, min_samples=3, b=-1):
        _chk(lib().teb_amd_update_and_prune(self._h, b, self._opt3(new_start), self._opt3(new_goal), min_samples),
             "teb_amd_update_and_prune")

    def set_velocity_start(self, v, fixed=True, b=-1):
        _chk(lib().teb_amd_set_velocity_start(self._h, b, int(fixed), self._opt3(v)), "teb_amd_set_velocity_start")

    def set_velocity_goal(self, v=None, fixed=True, b=-1):
        _chk(lib().teb_amd_set_velocity_goal(self._h, b, int(fixed), self._opt3(v)), "teb_amd_set_velocity_goal")

    def pose_counts(self):
        self._sync_count()
        n = np.zeros(max(self.count, 1), np.int32)
        c = C.c_int32(0)
        _chk(lib().teb_amd_get_pose_counts(self._h, _abi._ptr(n, C.c_int32), C.byref(c)), "teb_amd_get_pose_counts")
        return n[:c.value].copy()

    def velocity_command(self, b, look_ahead_poses=1, prevent_look_ahead_poses_near_goal=0):
        vx = C.c_double(0); vy = C.c_double(0); om = C.c_double(0); ok = C.c_int32(0)
        _chk(lib().teb_amd_get_velocity_command(self._h, b, look_ahead_poses, prevent_look_ahead_poses_near_goal, C.byref(vx),
                                                C.byref(vy), C.byref(om), C.byref(ok)), "teb_amd_get_velocity_command")
        return bool(ok.value), np.array([vx.value, vy.value, om.value])

    def velocity_profile(self, b):
        rows = C.c_int32(0)
        _chk(lib().teb_amd_get_velocity_profile(self._h, b, None, 0, C.byref(rows)), "teb_amd_get_velocity_profile")
        out = np.zeros((rows.value, 3))
        _chk(lib().teb_amd_get_velocity_profile(self._h, b, _abi._ptr(out, C.c_double), rows.value, C.byref(rows)),
             "teb_amd_get_velocity_profile")
        return out

    def full_trajectory(self, b):
        rows = C.c_int32(0)
        _chk(lib().teb_amd_get_full_trajectory(self._h, b, None, 0, C.byref(rows)), "teb_amd_get_full_trajectory")
        out = np.zeros((rows.value, 7))
        _chk(lib().teb_amd_get_full_trajectory(self._h, b, _abi._ptr(out, C.c_double), rows.value, C.byref(rows)),
             "teb_amd_get_full_trajectory")
        return out

    def has_diverged(self, b):
        d = C.c_int32(0)
        _chk(lib().teb_amd_has_diverged(self._h, b, C.byref(d)), "teb_amd_has_diverged")
        return bool(d.value)

    def batch_statistics(self):
        """(available [B] bool, back_chi2 [B]): what optimizer_->batchStatistics() of every band would hold after the last optimize() -
        not empty / .back().chi2 (zero when the band's last optimize() call stopped before its last requested iteration)."""
        self._sync_count()
        B = self.count
        av = np.zeros(max(B, 1), np.int32); ch = np.zeros(max(B, 1))
        _chk(lib().teb_amd_get_batch_statistics(self._h, _abi._ptr(av, C.c_int32), _abi._ptr(ch, C.c_double)), "teb_amd_get_batch_statistics")
        return av[:B].astype(bool), ch[:B]

    # -- feasibility of the resident bands against a costmap grid (arithmetic part) -----------
    def set_costmap(self, cells, resolution, origin_x, origin_y):
        cells = np.ascontiguousarray(cells, dtype=np.uint8)
        _chk(lib().teb_amd_set_costmap(self._h, cells.ctypes.data_as(C.c_void_p), cells.shape[1], cells.shape[0], float(resolution),
                                       float(origin_x), float(origin_y)), "teb_amd_set_costmap")

    def set_obstacles_from_costmap(self, robot_pose, costmap_obstacles_behind_robot_dist, custom=None):
        """updateObstacleContainerWithCostmap (reference src/teb_local_planner_ros.cpp:478-504) on the grid of the last set_costmap,
        followed by the custom ObstacleTable (or None), as the obstacle table. Returns (n, xs, ys): the number of cell obstacles and
        their centres in table order."""
        pose = _abi.f64([float(v) for v in robot_pose[:3]])
        cap = max(int(self.max_obstacles), 1)
        n = C.c_int32(0)
        xs = np.zeros(cap); ys = np.zeros(cap)
        _chk(lib().teb_amd_set_obstacles_from_costmap(self._h, _abi._ptr(pose, C.c_double), float(costmap_obstacles_behind_robot_dist),
                                                      C.byref(custom.freeze()) if custom is not None else None, C.byref(n),
                                                      _abi._ptr(xs, C.c_double), _abi._ptr(ys, C.c_double), cap),
             "teb_amd_set_obstacles_from_costmap")
        self._n_obst = n.value + (len(custom) if custom is not None else 0)
        return n.value, xs[:n.value].copy(), ys[:n.value].copy()

    def set_obstacles_from_costmap_polygons(self, robot_pose, costmap_obstacles_behind_robot_dist, tile_cells=8, custom=None):
        """The converter slot of the reference (updateObstacleContainerWithCostmapConverter, src/teb_local_planner_ros.cpp:506-549)
        fed by the device: the lethal cells of the last set_costmap that set_obstacles_from_costmap keeps, as the convex hulls of their
        8-connected components inside tiles of tile_cells x tile_cells cells (points, lines, polygons; include/teb_amd.h), followed by
        the custom ObstacleTable (or None), as the obstacle table. Returns the converted rows as an ObstacleTable.

        tile_cells = 8 (40 cm tiles on a 5 cm costmap) by default: on the seeded maps of walls, boxes and disks of
        tools/costmap_polygons_times.py it cut the rows 13 - 27 fold against the point route and the optimise kernel 4 - 9 fold, most
        of what larger tiles gain, while a row may lie at most (T - 1) * sqrt(2) * resolution = 0.49 m nearer than its cells (1.06 m at
        T = 16). On sparse random cells it gains little or loses (profiles/costmap_polygons_times.txt)."""
        pose = _abi.f64([float(v) for v in robot_pose[:3]])
        cap_o = max(int(self.max_obstacles), 1)
        cap_p = 2 * cap_o + int(self.max_obstacle_vertices)   # a successful call fits: <= 2 vertices per point / line row
        n_o, n_p = C.c_int32(0), C.c_int32(0)
        off = np.zeros(cap_o + 1, np.int32)
        xs = np.zeros(cap_p); ys = np.zeros(cap_p)
        _chk(lib().teb_amd_set_obstacles_from_costmap_polygons(
            self._h, _abi._ptr(pose, C.c_double), float(costmap_obstacles_behind_robot_dist), int(tile_cells),
            C.byref(custom.freeze()) if custom is not None else None, C.byref(n_o), C.byref(n_p), _abi._ptr(off, C.c_int32),
            _abi._ptr(xs, C.c_double), _abi._ptr(ys, C.c_double), cap_o, cap_p), "teb_amd_set_obstacles_from_costmap_polygons")
        self._n_obst = n_o.value + (len(custom) if custom is not None else 0)
        return _abi.ObstacleTable.from_polygon_list(off[:n_o.value + 1], xs[:n_p.value], ys[:n_p.value])

    def is_trajectory_feasible(self, b, footprint, inscribed_radius, min_resolution_collision_check_angular=3.141592653589793,
                               look_ahead_idx=-1, feasibility_check_lookahead_distance=-1.0):
        """isTrajectoryFeasible of band b (-1: every band): (feasible, first_infeasible) - bools / ints, arrays for b = -1."""
        cnt = self.count if b < 0 else 1
        fx = _abi.f64([p[0] for p in footprint]); fy = _abi.f64([p[1] for p in footprint])
        ok = np.zeros(cnt, np.int32); first = np.zeros(cnt, np.int32)
        _chk(lib().teb_amd_is_trajectory_feasible(self._h, int(b), len(footprint), _abi._ptr(fx, C.c_double), _abi._ptr(fy, C.c_double),
                                                  float(inscribed_radius), float(min_resolution_collision_check_angular), int(look_ahead_idx),
                                                  float(feasibility_check_lookahead_distance), _abi._ptr(ok, C.c_int32), _abi._ptr(first, C.c_int32)),
             "teb_amd_is_trajectory_feasible")
        if b < 0:
            return ok.astype(bool), first
        return bool(ok[0]), int(first[0])

    # -- equivalence classes of the resident bands (arithmetic core) ----------------------
    def h_signatures(self, prescaler=1.0, values=True):
        """[B, M] (HSignature3d, include_dynamic_obstacles) or [B, 2] (HSignature: re, im); values=False: compute only (the
        signatures stay in the handle for filter_equivalence_classes / explore_candidates)."""
        self._sync_count()
        w = C.c_int32(0)
        if not values:
            _chk(lib().teb_amd_compute_h_signatures(self._h, prescaler, None, C.byref(w)), "teb_amd_compute_h_signatures")
            return None
        width = max(getattr(self, "_n_obst", 0), 2)
        out = np.zeros((max(self.count, 1), width))
        _chk(lib().teb_amd_compute_h_signatures(self._h, prescaler, _abi._ptr(out, C.c_double), C.byref(w)),
             "teb_amd_compute_h_signatures")
        return out.ravel()[:self.count * w.value].reshape(self.count, w.value).copy()

    def filter_equivalence_classes(self, threshold=0.1, best=-1, max_number_plans_in_current_class=1):
        keep = np.zeros(self.count, np.int32); valid = np.zeros(self.count, np.int32); reas = np.zeros(self.count, np.int32)
        I = lambda a: _abi._ptr(a, C.c_int32)
        _chk(lib().teb_amd_filter_equivalence_classes(self._h, threshold, best, max_number_plans_in_current_class, I(keep), I(valid),
                                                      I(reas)), "teb_amd_filter_equivalence_classes")
        return keep, valid, reas

    # -- candidate generation: createGraph + DepthFirst + addAndInitNewTeb -----------------
    def set_optimized_flags(self, flags):
        f = _abi.i32(flags)
        _chk(lib().teb_amd_set_optimized_flags(self._h, _abi._ptr(f, C.c_int32)), "teb_amd_set_optimized_flags")

    def optimized_flags(self):
        self._sync_count()
        f = np.zeros(max(self.count, 1), np.int32)
        _chk(lib().teb_amd_get_optimized_flags(self._h, _abi._ptr(f, C.c_int32)), "teb_amd_get_optimized_flags")
        return f[:self.count]

    def band_flags(self):
        """(via_points_enabled, has_vel_start, has_vel_goal), each [B]."""
        self._sync_count()
        v = np.zeros(max(self.count, 1), np.int32); a = v.copy(); g = v.copy()
        I = lambda x: _abi._ptr(x, C.c_int32)
        _chk(lib().teb_amd_get_band_flags(self._h, I(v), I(a), I(g)), "teb_amd_get_band_flags")
        return v[:self.count], a[:self.count], g[:self.count]

    def filter_detours(self, keep, best, params=None):
        """deletePlansDetouringBackwards on the bands with keep != 0: returns the new keep array."""
        p = params if params is not None else self.cfg.hcp_params()
        keep = _abi.i32(keep).copy()
        _chk(lib().teb_amd_filter_detours(self._h, C.byref(p), int(best), _abi._ptr(keep, C.c_int32)), "teb_amd_filter_detours")
        return keep

    def compact_bands(self, keep, best=-1):
        """Keeps the bands with keep[b] != 0, last best band first (renewAndAnalyzeOldTebs): (n_kept, new_best)."""
        keep = _abi.i32(keep)
        nk = C.c_int32(0); nb = C.c_int32(-1)
        _chk(lib().teb_amd_compact_bands(self._h, _abi._ptr(keep, C.c_int32), int(best), C.byref(nk), C.byref(nb)),
             "teb_amd_compact_bands")
        self.count = nk.value
        return nk.value, nb.value

    def explore_candidates(self, start, goal, dist_to_obst=None, start_vel=None, free_goal_vel=False, best=-1, unit_samples=None,
                           max_paths=0, params=None, initial_plan=None):
        """exploreEquivalenceClassesAndInitTebs after renewAndAnalyzeOldTebs on the resident batch: dict(n_total, n_vertices, n_paths)."""
        p = params if params is not None else self.cfg.hcp_params()
        st = _abi.f64(start); gl = _abi.f64(goal)
        sv = None if start_vel is None else _abi.f64(start_vel)
        us = None if unit_samples is None else _abi.f64(np.asarray(unit_samples).ravel())
        dist_to_obst = self.cfg.obstacles.min_obstacle_dist if dist_to_obst is None else dist_to_obst
        nt = C.c_int32(0); nv = C.c_int32(0); npth = C.c_int32(0); ipt = C.c_int32(-1)
        plan = [None, None, None] if initial_plan is None else [_abi.f64(a) for a in initial_plan]      # (x, y, yaw) of the poses
        _chk(lib().teb_amd_explore_candidates(self._h, C.byref(p), _abi._ptr(st, C.c_double), _abi._ptr(gl, C.c_double),
                                              float(dist_to_obst), _abi._ptr(sv, C.c_double), int(bool(free_goal_vel)), int(best),
                                              _abi._ptr(us, C.c_double), int(max_paths), C.byref(nt), C.byref(nv), C.byref(npth),
                                              0 if initial_plan is None else len(plan[0]), _abi._ptr(plan[0], C.c_double),
                                              _abi._ptr(plan[1], C.c_double), _abi._ptr(plan[2], C.c_double), C.byref(ipt)),
             "teb_amd_explore_candidates")
        self.count = nt.value
        return dict(n_total=nt.value, n_vertices=nv.value, n_paths=npth.value, initial_plan_teb=ipt.value)

    def exploration_graph(self):
        """(vertices [N, 2], adjacency [N, N] uint8) of the last explore_candidates call."""
        nv = C.c_int32(0)
        _chk(lib().teb_amd_get_exploration_graph(self._h, None, None, None, 0, C.byref(nv)), "teb_amd_get_exploration_graph")
        N = nv.value
        vx = np.zeros(max(N, 1)); vy = np.zeros(max(N, 1)); adj = np.zeros((max(N, 1), max(N, 1)), np.uint8)
        if N:
            _chk(lib().teb_amd_get_exploration_graph(self._h, _abi._ptr(vx, C.c_double), _abi._ptr(vy, C.c_double),
                                                     adj.ctypes.data_as(C.POINTER(C.c_ubyte)), N, C.byref(nv)),
                 "teb_amd_get_exploration_graph")
        return np.stack([vx[:N], vy[:N]], 1), adj[:N, :N]

    # -- test hooks -----------------------------------------------------------------------------------
    def debug_linearize(self, b, n, weight_multiplier=1.0, assoc_cap=1 << 16):
        D = 4 * n
        H = np.zeros((D, D)); bv = np.zeros(D); chi2 = np.zeros(4)
        ap = np.zeros(assoc_cap, np.int32); ao = np.zeros(assoc_cap, np.int32)
        cnt = C.c_int32(0)
        _chk(lib().teb_amd_debug_linearize(self._h, b, weight_multiplier, _abi._ptr(H, C.c_double),
                                           _abi._ptr(bv, C.c_double), _abi._ptr(chi2, C.c_double),
                                           _abi._ptr(ap, C.c_int32), _abi._ptr(ao, C.c_int32), assoc_cap,
                                           C.byref(cnt)), "teb_amd_debug_linearize")
        k = min(cnt.value, assoc_cap)
        return dict(H=H, b=bv, chi2=chi2, assoc_pose=ap[:k].copy(), assoc_obst=ao[:k].copy())

    def debug_distance(self, obst_index, x, y, theta, t=None):
        oi = _abi.i32(obst_index); x = _abi.f64(x); y = _abi.f64(y); th = _abi.f64(theta)
        nq = len(oi)
        st = _abi.i32(np.zeros(nq) if t is None else np.ones(nq))
        tt = _abi.f64(np.zeros(nq) if t is None else t)
        d = np.zeros(nq); g = np.zeros((nq, 3))
        _chk(lib().teb_amd_debug_distance(self._h, nq, _abi._ptr(oi, C.c_int32), _abi._ptr(x, C.c_double),
                                          _abi._ptr(y, C.c_double), _abi._ptr(th, C.c_double),
                                          _abi._ptr(st, C.c_int32), _abi._ptr(tt, C.c_double),
                                          _abi._ptr(d, C.c_double), _abi._ptr(g, C.c_double)),
             "teb_amd_debug_distance")
        return d, g

    def debug_stream(self, n_doubles, repeats=1):
        _chk(lib().teb_amd_debug_stream(self._h, int(n_doubles), int(repeats)), "teb_amd_debug_stream")

    def debug_overflow_flags(self):
        f = np.zeros(self.count, np.int32)
        _chk(lib().teb_amd_debug_assoc_overflow(self._h, _abi._ptr(f, C.c_int32)), "debug_assoc_overflow")
        return f


def make_solver(cfg, obst, via, batch, device=0, stream=None, max_tebs=None, max_poses=None, options=None):
    """Creates a solver sized for the scene, uploads scene + batch. options: _abi.Options (layout pins etc.) or None."""
    nverts = len(obst.vert_x)
    s = TebBatchSolver(cfg, max_tebs or batch.count, max_poses or batch.stride, max(len(obst), 1), max(nverts, 1),
                       max(len(via), 1), device=device, stream=stream, options=options)
    s.set_obstacles(obst)
    s.set_via_points(via)
    s.upload(batch)
    return s


class TebOptimalPlanner:
    """Single-candidate view (reference include/teb_local_planner/optimal_planner.h:100-696)."""

    def __init__(self, cfg, obstacles=None, via_points=None, max_poses=None, device=0):
        self.cfg_ = cfg
        self.obstacles_ = obstacles if obstacles is not None else _abi.ObstacleTable()
        self.via_points_ = list(via_points or [])
        # capacity = whatever autoResize may produce (max_samples + 1, at most TEB_AMD_MAX_POSES); pass a smaller max_poses for the faster LDS layouts
        self.max_poses = max_poses or min(cfg.trajectory.max_samples + 1, _abi.MAX_POSES)
        self.teb_ = _abi.TebBatchHost(1, self.max_poses)
        self.cost_ = float("nan")
        self.optimized_ = False
        self.device = device
        self._solver = None
        self.last_results = None

    def teb(self):
        return self.teb_

    def setVelocityStart(self, vx, vy, omega):
        self.teb_.has_vel_start[0] = 1
        self.teb_.vel_start[0] = (vx, vy, omega)

    def setVelocityGoal(self, vx, vy, omega):
        self.teb_.has_vel_goal[0] = 1
        self.teb_.vel_goal[0] = (vx, vy, omega)

    def setVelocityGoalFree(self):
        self.teb_.has_vel_goal[0] = 0

    def getCurrentCost(self):
        return self.cost_

    def isOptimized(self):
        return self.optimized_

    def optimizeTEB(self, iterations_innerloop, iterations_outerloop, compute_cost_afterwards=False,
                    obst_cost_scale=1.0, viapoint_cost_scale=1.0, alternative_time_cost=False):
        if not self.cfg_.optim.optimization_activate:
            return False
        self.optimized_ = False
        if self._solver is None:
            self._solver = TebBatchSolver(self.cfg_, 1, self.max_poses, max(len(self.obstacles_), 1),
                                          max(len(self.obstacles_.vert_x), 1), max(len(self.via_points_), 1),
                                          device=self.device)
        s = self._solver
        s.set_config(self.cfg_)
        s.set_obstacles(self.obstacles_)
        s.set_via_points(self.via_points_)
        s.upload(self.teb_)
        s.optimize(iterations_innerloop, iterations_outerloop, compute_cost_afterwards, obst_cost_scale,
                   viapoint_cost_scale, alternative_time_cost)
        res = s.results()
        s.download(self.teb_)
        self.last_results = res
        if res.status[0] != _abi.TEB_OK:
            return False
        self.optimized_ = True
        if compute_cost_afterwards:
            self.cost_ = float(res.cost[0])
        return True


    # ---- plan(): warm start on the device-resident band, then optimizeTEB (src/optimal_planner.cpp:247-320) -------------------
    def _ensure_solver(self):
        if self._solver is None:
            self._solver = TebBatchSolver(self.cfg_, 1, self.max_poses, max(len(self.obstacles_), 1),
                                          max(len(self.obstacles_.vert_x), 1), max(len(self.via_points_), 1), device=self.device)
            self._resident = False
        return self._solver

    def clearPlanner(self):
        """clearPlanner(): the next plan() initialises a new band (optimal_planner.h:315-320)."""
        self.teb_.n[0] = 0
        self._resident = False
        self.optimized_ = False

    def _tick(self, init, start, goal, start_vel, free_goal_vel):
        import math
        s = self._ensure_solver()
        t = self.cfg_.trajectory
        n = int(self.teb_.n[0])
        warm = False
        if getattr(self, "_resident", False) and n > 0:
            gx, gy, gth = self.teb_.x[0, n - 1], self.teb_.y[0, n - 1], self.teb_.theta[0, n - 1]
            d = math.hypot(goal[0] - gx, goal[1] - gy)
            a = abs((goal[2] - gth + math.pi) % (2 * math.pi) - math.pi)      # fabs(g2o::normalize_theta(...))
            warm = d < t.force_reinit_new_goal_dist and a < t.force_reinit_new_goal_angular
        if warm:
            s.update_and_prune(start, goal, t.min_samples)                          # updateAndPruneTEB on the device
        else:
            init(s)                                                                 # initTrajectoryToGoal on the device
        self._resident = True
        if start_vel is not None:
            self.setVelocityStart(*start_vel)
        self.teb_.has_vel_goal[0] = 0 if free_goal_vel else 1                       # setVelocityGoalFree() / vel_goal_.first = true
        s.set_velocity_start(self.teb_.vel_start[0], bool(self.teb_.has_vel_start[0]))
        s.set_velocity_goal(self.teb_.vel_goal[0], bool(self.teb_.has_vel_goal[0]))
        s.set_config(self.cfg_)
        s.set_obstacles(self.obstacles_)
        s.set_via_points(self.via_points_)
        o = self.cfg_.optim
        if not o.optimization_activate:
            return False
        self.optimized_ = False
        s.optimize(o.no_inner_iterations, o.no_outer_iterations)
        res = s.results()
        s.download(self.teb_)               # host copy for teb() / the next warm-start test; the band itself stays on the device
        self.last_results = res
        self.optimized_ = res.status[0] == _abi.TEB_OK
        return bool(self.optimized_)

    def plan(self, start, goal, start_vel=None, free_goal_vel=False):
        """plan(const PoseSE2& start, const PoseSE2& goal, start_vel, free_goal_vel), src/optimal_planner.cpp:292-320.
        start / goal = (x, y, theta), start_vel = (vx, vy, omega) or None."""
        t, r = self.cfg_.trajectory, self.cfg_.robot
        return self._tick(lambda s: s.init_trajectory_line(0, start, goal, 0, r.max_vel_x, t.min_samples,
                                                           t.allow_init_with_backwards_motion), start, goal, start_vel, free_goal_vel)

    def planFromPath(self, plan_x, plan_y, plan_yaw, start_vel=None, free_goal_vel=False):
        """plan(const std::vector<geometry_msgs::PoseStamped>& initial_plan, ...), src/optimal_planner.cpp:247-283."""
        t, r = self.cfg_.trajectory, self.cfg_.robot
        start = (plan_x[0], plan_y[0], plan_yaw[0]); goal = (plan_x[-1], plan_y[-1], plan_yaw[-1])
        return self._tick(lambda s: s.init_trajectory_plan(0, plan_x, plan_y, plan_yaw, r.max_vel_x, r.max_vel_theta,
                                                           t.global_plan_overwrite_orientation, t.min_samples,
                                                           t.allow_init_with_backwards_motion), start, goal, start_vel, free_goal_vel)

    # ---- consumers (src/optimal_planner.cpp:1023-1247) on the device-resident band ---------------------------------------------
    def getVelocityCommand(self, look_ahead_poses=None):
        t = self.cfg_.trajectory
        ok, v = self._ensure_solver().velocity_command(0, t.control_look_ahead_poses if look_ahead_poses is None else look_ahead_poses,
                                                       t.prevent_look_ahead_poses_near_goal)
        return ok, float(v[0]), float(v[1]), float(v[2])

    def getVelocityProfile(self):
        return self._ensure_solver().velocity_profile(0)

    def getFullTrajectory(self):
        return self._ensure_solver().full_trajectory(0)

    def hasDiverged(self):
        return self._ensure_solver().has_diverged(0)

    def isTrajectoryFeasible(self, costmap, footprint_spec, inscribed_radius, circumscribed_radius=0.0, look_ahead_idx=-1,
                             feasibility_check_lookahead_distance=-1.0):
        """isTrajectoryFeasible (optimal_planner.h:500, src/optimal_planner.cpp:1250-1308) of the resident band. costmap: an object with
        cells [size_y, size_x] uint8, resolution, origin_x, origin_y (the grid of costmap_2d::Costmap2D) standing in for the
        base_local_planner::CostmapModel* of the reference; footprint_spec: [(x, y), ...]. circumscribed_radius is accepted and unused,
        as in CostmapModel::footprintCost."""
        s = self._ensure_solver()
        s.set_costmap(costmap.cells, costmap.resolution, costmap.origin_x, costmap.origin_y)
        return s.is_trajectory_feasible(0, footprint_spec, inscribed_radius, self.cfg_.trajectory.min_resolution_collision_check_angular,
                                        look_ahead_idx, feasibility_check_lookahead_distance)[0]


class TebFleetPlanner:
    """TebOptimalPlanner over a fleet: one band per robot on ONE handle, every robot with its own obstacles and via-points (a scene
    each, teb_amd_set_scenes), all bands optimised in one launch. Configuration and footprint are the fleet's - or, with robot_cfgs
    (the robot classes, a TebConfig each) and class_of_robot, those of every robot's class (teb_amd_set_scene_configs): robot r then
    takes the trajectory / robot parameters of its class for its warm-start test, initTrajectoryToGoal, updateAndPruneTEB and the
    look-ahead of its command, and its band runs under its class's configuration. The iteration counts and optimization_activate are
    one per launch: the classes must agree on them. Robot r is band r and scene r. Each robot's band ends with the bits of a single-scene handle that holds only its scene with the options
    generic_config_path = 1, multi_cu = -1 (no helper workgroups) and speculative_trials = -1, the same max_poses and the distance path
    of the fleet (include/teb_amd.h, fleet batches). A default TebOptimalPlanner of that robot runs a kernel folded on the TebConfig
    defaults, and on scenes that are not point-like it may use helper workgroups: it gives the same bits only as far as those kinds
    equal the generic one - they are held to that for point scenes (tests/test_gpu_fleet.py); for generic scenes DESIGN.md section 8
    lists an open defect of the distance helpers, so compare against a handle with the options above."""

    def __init__(self, cfg, n_robots, max_poses=None, max_obstacles=256, max_obstacle_vertices=256, max_via_points=64, device=0, options=None,
                 robot_cfgs=None, class_of_robot=None):
        self.cfg_ = cfg
        self.n_robots = int(n_robots)
        if (robot_cfgs is None) != (class_of_robot is None):
            raise ValueError("TebFleetPlanner: robot_cfgs and class_of_robot come together")
        self.robot_cfgs = list(robot_cfgs) if robot_cfgs is not None else None
        self.class_of_robot = None
        if self.robot_cfgs is not None:
            self.class_of_robot = [int(k) for k in class_of_robot]
            if len(self.class_of_robot) != self.n_robots:
                raise ValueError("TebFleetPlanner: %d class entries for %d robots" % (len(self.class_of_robot), self.n_robots))
            if not self.robot_cfgs or min(self.class_of_robot) < 0 or max(self.class_of_robot) >= len(self.robot_cfgs):
                raise ValueError("TebFleetPlanner: class_of_robot does not fit the %d classes" % len(self.robot_cfgs))
            o0 = self.robot_cfgs[0].optim
            for k, c in enumerate(self.robot_cfgs):   # one launch: one pair of iteration counts
                if (c.optim.no_inner_iterations, c.optim.no_outer_iterations, bool(c.optim.optimization_activate)) != \
                        (o0.no_inner_iterations, o0.no_outer_iterations, bool(o0.optimization_activate)):
                    raise ValueError("TebFleetPlanner: class %d differs from class 0 in no_inner_iterations / no_outer_iterations / "
                                     "optimization_activate, which are one per launch" % k)
        self._classes_installed = None   # the class map as last installed on the handle
        longest = max(c.trajectory.max_samples for c in (self.robot_cfgs or [cfg]))
        self.max_poses = max_poses or min(longest + 1, _abi.MAX_POSES)
        self.teb_ = _abi.TebBatchHost(self.n_robots, self.max_poses)
        self.device = device
        self._solver = TebBatchSolver(cfg, self.n_robots, self.max_poses, max(max_obstacles, 1), max(max_obstacle_vertices, 1),
                                      max(max_via_points, 1), device=device, options=options)
        self._solver.set_band_scenes(list(range(self.n_robots)))
        self._resident = [False] * self.n_robots
        self.optimized_ = np.zeros(self.n_robots, bool)
        self.last_results = None

    @property
    def solver(self):
        return self._solver

    def teb(self):
        return self.teb_

    def cfg_of(self, r):
        """the configuration robot r runs under: its class's, or the fleet's"""
        return self.cfg_ if self.robot_cfgs is None else self.robot_cfgs[self.class_of_robot[r]]

    def clearPlanner(self, r=None):
        """clearPlanner() of robot r (None: of every robot): its next plan() initialises a new band."""
        for k in (range(self.n_robots) if r is None else [r]):
            self.teb_.n[k] = 0
            self._resident[k] = False
            self.optimized_[k] = False

    def plan(self, starts, goals, start_vels=None, obstacles_per_robot=None, via_per_robot=None, free_goal_vel=False):
        """plan(start, goal, start_vel, free_goal_vel) of every robot (src/optimal_planner.cpp:292-320): per band the warm start on the
        resident band or initTrajectoryToGoal, exactly as TebOptimalPlanner.plan decides it, then ONE optimize over the fleet.
        starts / goals: [n_robots] (x, y, theta); start_vels: [n_robots] (vx, vy, omega) or None entries; obstacles_per_robot:
        [n_robots] ObstacleTable; via_per_robot: [n_robots] [(x, y), ...]. Returns [n_robots] bool (optimizeTEB's return)."""
        import math
        s = self._solver
        R = self.n_robots
        if len(starts) != R or len(goals) != R:
            raise ValueError("TebFleetPlanner.plan: %d starts / %d goals for %d robots" % (len(starts), len(goals), R))
        obstacles_per_robot = list(obstacles_per_robot) if obstacles_per_robot is not None else [_abi.ObstacleTable() for _ in range(R)]
        via_per_robot = list(via_per_robot) if via_per_robot is not None else [[] for _ in range(R)]
        for k in range(R):
            start, goal = starts[k], goals[k]
            t, r = self.cfg_of(k).trajectory, self.cfg_of(k).robot
            n = int(self.teb_.n[k])
            warm = False
            if self._resident[k] and n > 0:
                gx, gy, gth = self.teb_.x[k, n - 1], self.teb_.y[k, n - 1], self.teb_.theta[k, n - 1]
                d = math.hypot(goal[0] - gx, goal[1] - gy)
                a = abs((goal[2] - gth + math.pi) % (2 * math.pi) - math.pi)      # fabs(g2o::normalize_theta(...))
                warm = d < t.force_reinit_new_goal_dist and a < t.force_reinit_new_goal_angular
            if warm:
                s.update_and_prune(start, goal, t.min_samples, b=k)                 # updateAndPruneTEB on the device
            else:
                s.init_trajectory_line(k, start, goal, 0, r.max_vel_x, t.min_samples, t.allow_init_with_backwards_motion)
            self._resident[k] = True
            if start_vels is not None and start_vels[k] is not None:
                self.teb_.has_vel_start[k] = 1
                self.teb_.vel_start[k] = start_vels[k]
            self.teb_.has_vel_goal[k] = 0 if free_goal_vel else 1
            s.set_velocity_start(self.teb_.vel_start[k], bool(self.teb_.has_vel_start[k]), b=k)
            s.set_velocity_goal(self.teb_.vel_goal[k], bool(self.teb_.has_vel_goal[k]), b=k)
        s.set_config(self.cfg_)
        s.set_scenes(obstacles_per_robot, via_per_robot)
        if self.robot_cfgs is not None:   # the class map survives set_scenes of the same size: installed when it changed
            want = ([c.to_c() for c in self.robot_cfgs], list(self.class_of_robot))
            have = self._classes_installed
            if have is None or have[1] != want[1] or len(have[0]) != len(want[0]) or any(bytes(a) != bytes(b) for a, b in zip(have[0], want[0])):
                s.set_scene_configs(self.robot_cfgs, self.class_of_robot)
                self._classes_installed = want
        o = self.cfg_of(0).optim
        if not o.optimization_activate:
            return np.zeros(R, bool)
        self.optimized_[:] = False
        s.optimize(o.no_inner_iterations, o.no_outer_iterations)
        res = s.results()
        s.download(self.teb_)               # host copy for teb() / the next warm-start test; the bands themselves stay on the device
        self.last_results = res
        self.optimized_ = res.status[:R] == _abi.TEB_OK
        return self.optimized_.copy()

    def getVelocityCommands(self, look_ahead_poses=None):
        """[(ok, vx, vy, omega)] of every robot: getVelocityCommand on its resident band."""
        if self.robot_cfgs is None:
            t = self.cfg_.trajectory
            la = t.control_look_ahead_poses if look_ahead_poses is None else look_ahead_poses
            out = []
            for k in range(self.n_robots):
                ok, v = self._solver.velocity_command(k, la, t.prevent_look_ahead_poses_near_goal)
                out.append((ok, float(v[0]), float(v[1]), float(v[2])))
            return out
        # each robot's own look-ahead parameters. The handle keeps the commands of ONE (look-ahead, prevent) pair: the robots are asked
        # pair by pair, one launch over all bands per distinct pair and not one per robot where classes that differ in them interleave
        pairs = {}
        for k in range(self.n_robots):
            t = self.cfg_of(k).trajectory
            la = t.control_look_ahead_poses if look_ahead_poses is None else look_ahead_poses
            pairs.setdefault((int(la), int(t.prevent_look_ahead_poses_near_goal)), []).append(k)
        out = [None] * self.n_robots
        for (la, prevent), robots in pairs.items():
            ok, v = self._solver.velocity_commands(robots, la, prevent)
            for i, k in enumerate(robots):
                out[k] = (bool(ok[i]), float(v[i, 0]), float(v[i, 1]), float(v[i, 2]))
        return out

    def pose_counts(self):
        return self._solver.pose_counts()


class FleetHomotopyClassPlanner:
    """HomotopyClassPlanner::plan() of every robot of a fleet on ONE handle: robot r is scene r, its candidates are the bands
    the band -> scene map gives it. Configuration and footprint are the fleet's - or, with robot_cfgs (the robot classes, a TebConfig
    each) and class_of_robot, those of every robot's class (a heterogeneous fleet: set_scene_configs after set_scenes*, installed when
    it changed, and the four _per_class calls of include/teb_amd.h in place of their _per_scene siblings): robot r then runs under its
    class from updateAllTEBs to the saturated command - force_reinit_new_goal_dist / _angular, min_samples, the exploration's
    min_obstacle_dist and initialiser limits, the cost triple of selectBestTeb, switching_blocking_period, the divergence rule, the
    look-ahead of its command, the feasibility parameters and the saturation limits. What is one per call must agree over the classes
    (ValueError with the class and the field): every field of hcp_params(), delete_detours_backwards, max_number_classes, the iteration
    counts, optimization_activate, xy_goal_tolerance, costmap_obstacles_behind_robot_dist unless plan() is given one, and
    selection_dropping_probability == 0. A tick is set_config, set_scenes, updateAllTEBs per robot, then renewAndAnalyzeOldTebs
    (h_signatures_per_scene, filter_equivalence_classes_per_scene, filter_detours_per_scene, compact_bands_per_scene),
    explore_candidates_per_scene, one optimize over all bands and select_best_per_scene with switching_blocking_period per robot.
    Every robot's bands end with the bits of a HomotopyClassPlanner of its own whose handle follows the fleet contract of
    include/teb_amd.h. best_teb_ / initial_plan_teb_ [n_robots] are band indices of the batch (-1: none). With costmaps_per_robot,
    plan() also derives every robot's obstacle table from its own grid (set_costmaps, then set_scenes_from_costmaps or, with
    costmap_tile_cells, set_scenes_from_costmap_polygons), and
    isTrajectoryFeasible / hasDiverged / getVelocityCommands answer for every robot's best band in one call each.
    randomlyDropTebs is not carried over (selection_dropping_probability > 0: NotImplementedError)."""

    def __init__(self, cfg, n_robots, max_tebs=None, max_poses=None, max_obstacles=256, max_obstacle_vertices=256, max_via_points=64,
                 device=0, stream=None, options=None, robot_cfgs=None, class_of_robot=None):
        self.cfg_ = cfg
        self.n_robots = int(n_robots)
        if (robot_cfgs is None) != (class_of_robot is None):
            raise ValueError("FleetHomotopyClassPlanner: robot_cfgs and class_of_robot come together")
        self.robot_cfgs = list(robot_cfgs) if robot_cfgs is not None else None
        self.class_of_robot = None
        if self.robot_cfgs is not None:
            self.class_of_robot = [int(k) for k in class_of_robot]
            if len(self.class_of_robot) != self.n_robots:
                raise ValueError("FleetHomotopyClassPlanner: %d class entries for %d robots" % (len(self.class_of_robot), self.n_robots))
            if not self.robot_cfgs or min(self.class_of_robot) < 0 or max(self.class_of_robot) >= len(self.robot_cfgs):
                raise ValueError("FleetHomotopyClassPlanner: class_of_robot does not fit the %d classes" % len(self.robot_cfgs))
            for k, c in enumerate(self.robot_cfgs):
                if c.hcp.selection_dropping_probability > 0:
                    raise ValueError("FleetHomotopyClassPlanner: class %d has selection_dropping_probability > 0: randomlyDropTebs is "
                                     "not available per scene" % k)
                for field, a, b in self._one_per_call(self.robot_cfgs[0], c):
                    if a != b:
                        raise ValueError("FleetHomotopyClassPlanner: class %d differs from class 0 in %s, which is one per call" % (k, field))
        elif cfg.hcp.selection_dropping_probability > 0:
            raise NotImplementedError("FleetHomotopyClassPlanner: randomlyDropTebs (selection_dropping_probability > 0) is not available per scene")
        self._shared = self.robot_cfgs[0] if self.robot_cfgs is not None else cfg   # what is one per call: the classes agree on it
        self._classes_installed = None   # the class map as last installed on the handle
        self.solver = TebBatchSolver(cfg, max_tebs or self.n_robots * max(self._shared.hcp.max_number_classes, 1), max_poses or 224, max(max_obstacles, 1),
                                     max(max_obstacle_vertices, 1), max(max_via_points, 1), device=device, stream=stream, options=options)
        self.best_teb_ = np.full(self.n_robots, -1, np.int32)
        self.initial_plan_teb_ = np.full(self.n_robots, -1, np.int32)
        self.last_results = None
        self.last_exploration = None
        self._goal = [None] * self.n_robots
        self._last_switch = [0.0] * self.n_robots
        self._last_best_teb = np.full(self.n_robots, -1, np.int32)
        self._has_costmaps = False
        self._plans = None                                          # setPlans: the global plans as given, resident on the device
        self.no_infeasible_plans_ = np.zeros(self.n_robots, np.int32)   # computeVelocityCommands: failures in a row, robot by robot

    @staticmethod
    def _one_per_call(c0, c):
        """(field, value of class 0, value of the class) of everything a tick takes once for the whole fleet"""
        p0, p = c0.hcp_params(), c.hcp_params()
        for name, _ in _abi.HcpParams._fields_:
            yield name, getattr(p0, name), getattr(p, name)
        yield "delete_detours_backwards", bool(c0.hcp.delete_detours_backwards), bool(c.hcp.delete_detours_backwards)
        yield "max_number_classes", c0.hcp.max_number_classes, c.hcp.max_number_classes
        yield "no_inner_iterations", c0.optim.no_inner_iterations, c.optim.no_inner_iterations
        yield "no_outer_iterations", c0.optim.no_outer_iterations, c.optim.no_outer_iterations
        yield "optimization_activate", bool(c0.optim.optimization_activate), bool(c.optim.optimization_activate)
        yield "xy_goal_tolerance", c0.goal_tolerance.xy_goal_tolerance, c.goal_tolerance.xy_goal_tolerance

    def cfg_of(self, r):
        """the configuration robot r runs under: its class's, or the fleet's"""
        return self.cfg_ if self.robot_cfgs is None else self.robot_cfgs[self.class_of_robot[r]]

    def _of_class(self, v, k, nested=0):
        """v as given for class k: one value for all classes, or a sequence with one entry per class (nested: the depth of ONE value)"""
        if self.robot_cfgs is None:
            return v
        probe = v
        for _ in range(nested):
            probe = probe[0]
        if np.ndim(probe) == 0:
            return v
        if len(v) != len(self.robot_cfgs):
            raise ValueError("FleetHomotopyClassPlanner: %d entries for %d classes" % (len(v), len(self.robot_cfgs)))
        return v[k]

    def bands_of(self, r):
        """band indices of robot r, in band order"""
        return [int(b) for b in np.nonzero(self.solver.band_scenes() == r)[0]] if self.solver.count else []

    def _drop_bands(self, keep, best_only=False):
        """The bands with keep == 0 leave the batch, the kept ones move to the front in order: best_teb_, initial_plan_teb_ and
        _last_best_teb follow them (best_only: best_teb_ alone - updateAllTEBs, which leaves the other two as they are)."""
        if keep.all():
            return
        at = (np.cumsum(keep) - 1).astype(np.int32)
        move = lambda a: np.array([at[b] if b >= 0 else -1 for b in a], np.int32)
        self.best_teb_ = move(self.best_teb_)
        if not best_only:
            self.initial_plan_teb_, self._last_best_teb = move(self.initial_plan_teb_), move(self._last_best_teb)
        self.solver.compact_bands_per_scene(keep, None)

    # ---- updateAllTEBs (src/homotopy_class_planner.cpp:539-562) of every robot ---------------------------------------------------------
    def updateAllTEBs(self, starts, goals, start_vels=None):
        import math
        s = self.solver
        if s.count > 0:
            scene_of = s.band_scenes()
            keep = np.ones(s.count, np.int32)
            for r in range(self.n_robots):
                if self._goal[r] is None or not (scene_of == r).any():
                    continue
                t = self.cfg_of(r).trajectory
                d = math.hypot(goals[r][0] - self._goal[r][0], goals[r][1] - self._goal[r][1])
                a = abs((goals[r][2] - self._goal[r][2] + math.pi) % (2 * math.pi) - math.pi)
                if d >= t.force_reinit_new_goal_dist or a >= t.force_reinit_new_goal_angular:
                    keep[scene_of == r] = 0                       # tebs_.clear() of that robot only
                    self.best_teb_[r] = -1
            self._drop_bands(keep, best_only=True)                # the other robots' bands keep their order
        if s.count > 0:                                           # every band of every robot, one launch
            sv = hv = None
            if start_vels is not None and any(v is not None for v in start_vels):
                sv = [(0.0, 0.0, 0.0) if v is None else v for v in start_vels]
                hv = [0 if v is None else 1 for v in start_vels]
            if self.robot_cfgs is None:
                s.update_and_prune_per_scene(starts, goals, self.cfg_.trajectory.min_samples, sv, hv)
            else:
                s.update_and_prune_per_class(starts, goals, sv, hv)
        self._goal = [tuple(g) for g in goals]

    # ---- exploreEquivalenceClassesAndInitTebs (:318-340) of every robot ---------------------------------------------------------------
    def exploreEquivalenceClassesAndInitTebs(self, starts, goals, dist_to_obst, start_vels=None, free_goal_vel=False, initial_plans=None):
        s, h = self.solver, self._shared.hcp
        best = self.best_teb_
        if s.count > 0:
            s.h_signatures_per_scene(h.h_signature_prescaler, values=False)
            keep, _, _ = s.filter_equivalence_classes_per_scene(h.h_signature_threshold, best, h.max_number_plans_in_current_class)
            if h.delete_detours_backwards:
                keep = s.filter_detours_per_scene(keep, best)
            _, best = s.compact_bands_per_scene(keep, best)
        self.best_teb_ = np.asarray(best, np.int32).copy()
        sv = None
        if start_vels is not None and any(v is not None for v in start_vels):
            sv = [(0.0, 0.0, 0.0) if v is None else v for v in start_vels]   # a new band's default: fixed zero start velocity
        if self.robot_cfgs is None:
            self.last_exploration = s.explore_candidates_per_scene(starts, goals, dist_to_obst, sv, free_goal_vel, self.best_teb_,
                                                                   initial_plans=initial_plans)
        else:   # (dist_to_obst: min_obstacle_dist of every robot's class)
            self.last_exploration = s.explore_candidates_per_class(starts, goals, sv, free_goal_vel, self.best_teb_,
                                                                   params=self._shared.hcp_params(), initial_plans=initial_plans)
        scene_of = s.band_scenes() if s.count else np.zeros(0, np.int32)
        for r in range(self.n_robots):                            # getInitialPlanTEB() of selectBestTeb, as a band of the batch
            k = int(self.last_exploration["initial_plan_teb"][r])
            self.initial_plan_teb_[r] = np.nonzero(scene_of == r)[0][k] if k >= 0 else -1
        return self.last_exploration["n_total"]

    def plan(self, starts, goals, start_vels=None, obstacles_per_robot=None, via_per_robot=None, free_goal_vel=False, initial_plans=None,
             now=None, costmaps_per_robot=None, costmap_obstacles_behind_robot_dist=None, costmap_tile_cells=None):
        """plan(start, goal, start_vel, free_goal_vel) of every robot (:107-125), or plan(initial_plan, ...) (:84-96) for the robots with
        an entry in initial_plans ((x, y, yaw) arrays; start / goal are then the plan's first / last pose). starts / goals [n_robots]
        (x, y, theta); start_vels [n_robots] (vx, vy, omega) or None entries; obstacles_per_robot [n_robots] ObstacleTable;
        via_per_robot [n_robots] [(x, y), ...]. costmaps_per_robot [n_robots] (cells, resolution, origin_x, origin_y objects): every
        robot's table is updateObstacleContainerWithCostmap of its own grid seen from starts[r] (costmap_obstacles_behind_robot_dist:
        default cfg.obstacles.costmap_obstacles_behind_robot_dist) followed by obstacles_per_robot[r] as the custom rows, and the grids
        stay installed for isTrajectoryFeasible. costmap_tile_cells (an int or [n_robots], each 1 .. 64; needs costmaps_per_robot): the
        lethal cells become convex points / lines / polygons instead (set_scenes_from_costmap_polygons: robot r's grid in tiles of
        costmap_tile_cells[r] cells); None is the point route. Returns best_teb_."""
        R = self.n_robots
        if costmap_tile_cells is not None and costmaps_per_robot is None:
            raise ValueError("FleetHomotopyClassPlanner.plan: costmap_tile_cells needs costmaps_per_robot")
        if costmap_tile_cells is not None and np.ndim(costmap_tile_cells) != 0 and len(costmap_tile_cells) != R:
            raise ValueError("FleetHomotopyClassPlanner.plan: %d tile sizes for %d robots" % (len(costmap_tile_cells), R))
        for name, a in (("starts", starts), ("goals", goals), ("start velocities", start_vels), ("obstacle tables", obstacles_per_robot),
                        ("via-point lists", via_per_robot), ("initial plans", initial_plans), ("costmaps", costmaps_per_robot)):
            if a is not None and len(a) != R:
                raise ValueError("FleetHomotopyClassPlanner.plan: %d %s for %d robots" % (len(a), name, R))
        starts = [tuple(p) for p in starts]; goals = [tuple(p) for p in goals]
        if initial_plans is not None:
            for r, q in enumerate(initial_plans):
                if q is not None:
                    starts[r] = (q[0][0], q[1][0], q[2][0]); goals[r] = (q[0][-1], q[1][-1], q[2][-1])
        tables = list(obstacles_per_robot) if obstacles_per_robot is not None else [_abi.ObstacleTable() for _ in range(R)]
        vias = list(via_per_robot) if via_per_robot is not None else [[] for _ in range(R)]
        o, s = self._shared.optim, self.solver
        s.set_config(self.cfg_)
        if costmaps_per_robot is not None:
            if costmap_obstacles_behind_robot_dist is None and self.robot_cfgs is not None:
                for k, c in enumerate(self.robot_cfgs):
                    if c.obstacles.costmap_obstacles_behind_robot_dist != self._shared.obstacles.costmap_obstacles_behind_robot_dist:
                        raise ValueError("FleetHomotopyClassPlanner.plan: class %d differs from class 0 in costmap_obstacles_behind_robot_dist, "
                                         "which is one per call (or pass costmap_obstacles_behind_robot_dist)" % k)
            dist = self._shared.obstacles.costmap_obstacles_behind_robot_dist if costmap_obstacles_behind_robot_dist is None else costmap_obstacles_behind_robot_dist
            s.set_costmaps(costmaps_per_robot)
            if costmap_tile_cells is None:
                s.set_scenes_from_costmaps(starts, dist, tables, vias)
            else:
                s.set_scenes_from_costmap_polygons(starts, dist, costmap_tile_cells, tables, vias, return_tables=False)
        else:
            s.set_scenes(tables, vias)
        if self.robot_cfgs is not None:   # the class map survives set_scenes* of the same size: installed when it changed
            want = ([c.to_c() for c in self.robot_cfgs], list(self.class_of_robot))
            have = self._classes_installed
            if have is None or have[1] != want[1] or len(have[0]) != len(want[0]) or any(bytes(a) != bytes(b) for a, b in zip(have[0], want[0])):
                s.set_scene_configs(self.robot_cfgs, self.class_of_robot)
                self._classes_installed = want
        self._has_costmaps = costmaps_per_robot is not None
        self.updateAllTEBs(starts, goals, start_vels)
        self.exploreEquivalenceClassesAndInitTebs(starts, goals, self._shared.obstacles.min_obstacle_dist, start_vels, free_goal_vel, initial_plans)
        if s.count == 0:
            self.best_teb_[:] = -1
            return self.best_teb_.copy()
        self.optimizeAllTEBs(o.no_inner_iterations, o.no_outer_iterations)
        return self.selectBestTeb(now)

    def optimizeAllTEBs(self, iter_innerloop, iter_outerloop):
        if self.robot_cfgs is not None:   # the cost triple of every band's class
            self.solver.optimize_per_class(iter_innerloop, iter_outerloop, True)
            return
        h = self.cfg_.hcp
        self.solver.optimize(iter_innerloop, iter_outerloop, True, h.selection_obst_cost_scale, h.selection_viapoint_cost_scale,
                             h.selection_alternative_time_cost)

    def selectBestTeb(self, now=None):
        """selectBestTeb (:564-667) of every robot in one launch; switching_blocking_period (:648-663) robot by robot."""
        import time
        last = self.best_teb_.copy()
        self._last_best_teb = last.copy()                # last_best_teb_ (:566) of every robot
        best, _ = self.solver.select_best_per_scene(last, self.initial_plan_teb_)
        now = time.monotonic() if now is None else now
        for r in range(self.n_robots):
            if last[r] >= 0 and best[r] != last[r]:
                if now - self._last_switch[r] > self.cfg_of(r).hcp.switching_blocking_period:
                    self._last_switch[r] = now
                else:
                    best[r] = last[r]        # switching blocked
        self.best_teb_ = np.asarray(best, np.int32).copy()
        return self.best_teb_.copy()

    def getVelocityCommands(self, look_ahead_poses=None):
        """[(ok, vx, vy, omega)] of every robot: getVelocityCommand on its best band (:127-139), one call for all."""
        if self.robot_cfgs is None:
            t = self.cfg_.trajectory
            la = t.control_look_ahead_poses if look_ahead_poses is None else look_ahead_poses
            ok, v = self.solver.velocity_commands(self.best_teb_, la, t.prevent_look_ahead_poses_near_goal)
            return [(bool(ok[r]), float(v[r, 0]), float(v[r, 1]), float(v[r, 2])) for r in range(self.n_robots)]
        # each robot's own look-ahead parameters: one launch over all bands per distinct (look-ahead, prevent) pair, as TebFleetPlanner
        pairs = {}
        for r in range(self.n_robots):
            t = self.cfg_of(r).trajectory
            la = t.control_look_ahead_poses if look_ahead_poses is None else look_ahead_poses
            pairs.setdefault((int(la), int(t.prevent_look_ahead_poses_near_goal)), []).append(r)
        out = [None] * self.n_robots
        for (la, prevent), robots in pairs.items():
            ok, v = self.solver.velocity_commands([self.best_teb_[r] for r in robots], la, prevent)
            for i, r in enumerate(robots):
                out[r] = (bool(ok[i]), float(v[i, 0]), float(v[i, 1]), float(v[i, 2]))
        return out

    def isTrajectoryFeasible(self, footprint_spec, inscribed_radius, circumscribed_radius=0.0, look_ahead_idx=-1,
                             feasibility_check_lookahead_distance=-1.0):
        """HomotopyClassPlanner::isTrajectoryFeasible (src/homotopy_class_planner.cpp:686-709) of every robot against ITS grid of the
        costmaps plan(costmaps_per_robot=...) installed: a list of bools. Every round checks the best band of every undecided robot in
        one call; an infeasible best band is removed and the robot's next best tried in the next round, unless it was already the best
        band of the previous tick (then False). A robot without bands: False. With robot classes footprint_spec, inscribed_radius,
        look_ahead_idx and feasibility_check_lookahead_distance are one value, or one per class; the angular resolution is the class's."""
        s, R = self.solver, self.n_robots
        specs = None
        if self.robot_cfgs is not None:
            specs = [dict(footprint=self._of_class(footprint_spec, k, 2), inscribed_radius=self._of_class(inscribed_radius, k),
                          min_resolution_collision_check_angular=c.trajectory.min_resolution_collision_check_angular,
                          look_ahead_idx=self._of_class(look_ahead_idx, k),
                          feasibility_check_lookahead_distance=self._of_class(feasibility_check_lookahead_distance, k))
                     for k, c in enumerate(self.robot_cfgs)]
        if not self._has_costmaps:
            raise ValueError("FleetHomotopyClassPlanner.isTrajectoryFeasible: plan(costmaps_per_robot=...) installs the grids the bands are checked against")
        verdict = [None] * R
        ang = self.cfg_.trajectory.min_resolution_collision_check_angular
        while any(v is None for v in verdict):
            scene_of = s.band_scenes() if s.count else np.zeros(0, np.int32)
            open_ = [r for r in range(R) if verdict[r] is None]
            for r in open_:
                if not (scene_of == r).any():
                    verdict[r] = False
            open_ = [r for r in open_ if verdict[r] is None]
            if not open_:
                break
            if any(self.best_teb_[r] < 0 for r in open_):          # findBestTeb (:711-723): re-select where the best band is gone
                lb = np.array([-1 if (verdict[r] is None and self.best_teb_[r] < 0) else self.best_teb_[r] for r in range(R)], np.int32)
                best, _ = s.select_best_per_scene(lb, self.initial_plan_teb_)
                for r in open_:
                    if self.best_teb_[r] < 0:
                        self.best_teb_[r] = best[r]
                        self._last_best_teb[r] = -1
            bands = np.array([self.best_teb_[r] if verdict[r] is None else -1 for r in range(R)], np.int32)
            for r in open_:
                if bands[r] < 0:
                    verdict[r] = False
            if not (bands >= 0).any():
                break
            if specs is None:
                ok, _ = s.is_trajectory_feasible_per_scene(bands, footprint_spec, inscribed_radius, ang, look_ahead_idx,
                                                           feasibility_check_lookahead_distance)
            else:
                ok, _ = s.is_trajectory_feasible_per_class(bands, specs)   # (spec k belongs to class k: the map picks it)
            keep = np.ones(s.count, np.int32)
            for r in range(R):
                if bands[r] < 0:
                    continue
                if ok[r] == 1:
                    verdict[r] = True
                    continue
                best = int(bands[r])
                keep[best] = 0                                       # removeTeb (:725-744)
                if self._last_best_teb[r] == best:
                    verdict[r] = False                               # "not failing could result in oscillations between trajectories"
                    self._last_best_teb[r] = -1
                if self.initial_plan_teb_[r] == best:
                    self.initial_plan_teb_[r] = -1
                self.best_teb_[r] = -1
            self._drop_bands(keep)
        return [bool(v) for v in verdict]

    def hasDiverged(self):
        """TebOptimalPlanner::hasDiverged (src/optimal_planner.cpp:1023-1039) of every robot's best band: a list of bools (no best band:
        False), from one download of the batch statistics."""
        if self.solver.count == 0:
            return [False] * self.n_robots
        available, back_chi2 = self.solver.batch_statistics()
        out = []
        for r in range(self.n_robots):
            b, c = int(self.best_teb_[r]), self.cfg_of(r)
            out.append(bool(b >= 0 and c.recovery.divergence_detection_enable and available[b]
                            and back_chi2[b] > c.recovery.divergence_detection_max_chi_squared))
        return out

    def bands(self, stride=None):
        """Host copy of the resident bands: list of (x, y, theta, dt), in band order (bands_of(r): those of robot r)."""
        s = self.solver
        if s.count == 0:
            return []
        b = _abi.TebBatchHost(s.count, stride or s.max_poses)
        s.download(b)
        return [b.get_teb(k) for k in range(s.count)]

    def results(self):
        self.last_results = self.solver.results()
        return self.last_results

    # ---- the adapter's entry point (TebLocalPlannerROS::computeVelocityCommands, src/teb_local_planner_ros.cpp:236-462) of every robot ----
    def clearPlanner(self, r):
        """HomotopyClassPlanner::clearPlanner of robot r (an index or a list of them): its bands leave the batch in one compaction, the other
        robots' bands keep their order; its next plan() starts from new candidates."""
        s = self.solver
        rs = [int(r)] if np.ndim(r) == 0 else [int(k) for k in r]
        for k in rs:
            self.best_teb_[k] = self.initial_plan_teb_[k] = self._last_best_teb[k] = -1
            self._goal[k] = None
        if s.count == 0 or not rs:
            return
        self._drop_bands((~np.isin(s.band_scenes(), rs)).astype(np.int32))

    def setPlans(self, plans, robots=None):
        """setPlan of every robot: plans[r] = (x, y, yaw) arrays in the plan frame (None: no plan), resident on the device from here on.
        With robots given, plans holds the new plans of those robots only; the others keep theirs and their pruning cursors."""
        R = self.n_robots
        if self._plans is None:
            self._plans = [None] * R
        if robots is None:
            if len(plans) != R:
                raise ValueError("FleetHomotopyClassPlanner.setPlans: %d plans for %d robots" % (len(plans), R))
            self._plans = list(plans)
            begin = None
        else:
            if len(plans) != len(robots):
                raise ValueError("FleetHomotopyClassPlanner.setPlans: %d plans for %d robots to replace" % (len(plans), len(robots)))
            begin = self.solver.plan_cursors() if self.solver._plan_counts is not None else np.zeros(R, np.int32)
            for r, p in zip(robots, plans):
                self._plans[int(r)] = p
                begin[int(r)] = 0
        self.solver.set_global_plans(self._plans, begin)

    def computeVelocityCommands(self, robot_poses, robot_vels, costmaps_per_robot, footprint_spec, inscribed_radius, adapter=None,
                                plan_to_global=None, now=None, window_params=None, obstacles_per_robot=None,
                                costmap_obstacles_behind_robot_dist=None, costmap_tile_cells=None):
        """computeVelocityCommands of every robot at once, in the reference's order: the plan windows from the resident global plans
        (setPlans) and robot_poses [n_robots] (x, y, theta), thresholds from every grid's size (:729-731); the goal-reached test
        (:290-304); plan(initial_plans = windows, via_per_robot = the windows' via-points, costmaps_per_robot) for the others; hasDiverged,
        isTrajectoryFeasible, getVelocityCommands; saturateVelocity and, with adapter.cmd_angle_instead_rotvel, the steering angle.
        robot_vels [n_robots] (vx, vy, omega) is the odometry twist; adapter: adapter_defaults() or alike; plan_to_global [n_robots, 5]
        = (cos, sin, tx, ty, yaw_tf) or None; window_params: _abi.PlanWindowParams or None. Returns (status [n_robots], cmd [n_robots, 3]):
        SUCCESS with the saturated command, GOAL_REACHED / NO_VALID_CMD / INTERNAL_ERROR (a robot without a plan) with a zero command. A
        robot with NO_VALID_CMD has its bands dropped (clearPlanner) and no_infeasible_plans_[r] incremented; a success resets it.
        cfg.robot.max_vel_trans is used as it stands: the reference's reconfigure step sets it to max_vel_x when it is 0
        (src/teb_config.cpp:219-223), and a caller does the same in cfg.robot - at 0 saturateVelocity scales vx and vy to 0.
        last_tick holds the windows, the raw commands and the verdicts of the call."""
        import math
        R = self.n_robots
        a = adapter if adapter is not None else adapter_defaults()
        if self._plans is None:
            raise ValueError("FleetHomotopyClassPlanner.computeVelocityCommands: setPlans first")
        poses = [tuple(float(v) for v in p) for p in robot_poses]
        vels = [tuple(float(v) for v in p) for p in robot_vels]
        if len(poses) != R or len(vels) != R or len(costmaps_per_robot) != R:
            raise ValueError("FleetHomotopyClassPlanner.computeVelocityCommands: %d poses, %d velocities, %d costmaps for %d robots"
                             % (len(poses), len(vels), len(costmaps_per_robot), R))
        thr = []
        for c in costmaps_per_robot:
            sy, sx = np.shape(c.cells)
            thr.append(max(sx * c.resolution / 2.0, sy * c.resolution / 2.0) * 0.85)
        win = self.solver.plan_windows(poses, thr, window_params, plan_to_global)
        status = [self.SUCCESS] * R
        for r in range(R):
            if win["window_count"][r] == 0:
                status[r] = self.INTERNAL_ERROR               # "Could not transform the global plan" (:275-281): no plan
                continue
            gg = win["global_goal"][r]
            dx, dy = gg[0] - poses[r][0], gg[1] - poses[r][1]
            delta_orient = normalize_theta(gg[2] - poses[r][2])
            stopped = (abs(vels[r][2]) <= a.theta_stopped_vel and abs(vels[r][0]) <= a.trans_stopped_vel
                       and abs(vels[r][1]) <= a.trans_stopped_vel)   # base_local_planner::stopped
            if (abs(math.sqrt(dx * dx + dy * dy)) < self._shared.goal_tolerance.xy_goal_tolerance and abs(delta_orient) < a.yaw_goal_tolerance
                    and (not a.complete_global_plan or win["via_count"][r] == 0) and (stopped or a.free_goal_vel)):
                status[r] = self.GOAL_REACHED
        active = [status[r] == self.SUCCESS for r in range(R)]
        # a robot that needs no plan still needs a scene: start = goal = its pose, its result is ignored and its bands dropped below
        goals = [tuple(win["goal"][r]) if active[r] else poses[r] for r in range(R)]
        plans = [win["windows"][r] if active[r] else None for r in range(R)]
        vias = [win["vias"][r] if active[r] else [] for r in range(R)]
        best = self.plan(poses, goals, vels, obstacles_per_robot, vias, a.free_goal_vel, plans, now, costmaps_per_robot,
                         costmap_obstacles_behind_robot_dist, costmap_tile_cells)
        planned = [bool(best[r] >= 0) for r in range(R)]
        diverged = self.hasDiverged()
        if self.robot_cfgs is None:
            t = self.cfg_.trajectory
            feasible = self.isTrajectoryFeasible(footprint_spec, inscribed_radius, 0.0, t.feasibility_check_no_poses,
                                                 t.feasibility_check_lookahead_distance)
        else:   # every class's own look-ahead pair
            feasible = self.isTrajectoryFeasible(footprint_spec, inscribed_radius, 0.0,
                                                 [c.trajectory.feasibility_check_no_poses for c in self.robot_cfgs],
                                                 [c.trajectory.feasibility_check_lookahead_distance for c in self.robot_cfgs])
        raw = self.getVelocityCommands()
        cmd = np.zeros((R, 3))
        for r in range(R):
            if not active[r]:
                continue
            rb = self.cfg_of(r).robot
            ok = planned[r] and not diverged[r] and feasible[r] and raw[r][0]
            if ok:
                v = saturate_velocity(raw[r][1], raw[r][2], raw[r][3], rb.max_vel_x, rb.max_vel_y, rb.max_vel_trans, rb.max_vel_theta,
                                      rb.max_vel_x_backwards, a.use_proportional_saturation)
                if a.cmd_angle_instead_rotvel:
                    v = (v[0], v[1], steering_angle(v[0], v[2], a.wheelbase, 0.95 * rb.min_turning_radius))
                    ok = math.isfinite(v[2])
            if ok:
                cmd[r] = v
                self.no_infeasible_plans_[r] = 0
            else:
                status[r] = self.NO_VALID_CMD
                self.no_infeasible_plans_[r] += 1
        self.last_tick = dict(windows=win, raw=raw, planned=planned, diverged=diverged, feasible=feasible)
        self.clearPlanner([r for r in range(R) if status[r] != self.SUCCESS])
        return status, cmd


FleetHomotopyClassPlanner.SUCCESS, FleetHomotopyClassPlanner.GOAL_REACHED = "SUCCESS", "GOAL_REACHED"
FleetHomotopyClassPlanner.NO_VALID_CMD, FleetHomotopyClassPlanner.INTERNAL_ERROR = "NO_VALID_CMD", "INTERNAL_ERROR"


def adapter_defaults():
    """What computeVelocityCommands reads beside TebConfig, with the reference's defaults (teb_config.h:286-298): no part
    of TebConfig. The velocity limits come from cfg.robot, xy_goal_tolerance from cfg.goal_tolerance."""
    from types import SimpleNamespace
    return SimpleNamespace(yaw_goal_tolerance=0.2, free_goal_vel=False, trans_stopped_vel=0.1, theta_stopped_vel=0.1,
                           complete_global_plan=True, use_proportional_saturation=False, cmd_angle_instead_rotvel=False, wheelbase=1.0)


def saturate_velocity(vx, vy, omega, max_vel_x, max_vel_y, max_vel_trans, max_vel_theta, max_vel_x_backwards,
                      use_proportional_saturation=False):
    """TebLocalPlannerROS::saturateVelocity (src/teb_local_planner_ros.cpp:874-919) -> (vx, vy, omega)"""
    import math
    ratio_x = ratio_omega = ratio_y = 1.0
    if vx > max_vel_x:
        ratio_x = max_vel_x / vx
    if vy > max_vel_y or vy < -max_vel_y:
        ratio_y = abs(max_vel_y / vy)
    if omega > max_vel_theta or omega < -max_vel_theta:
        ratio_omega = abs(max_vel_theta / omega)
    if max_vel_x_backwards > 0 and vx < -max_vel_x_backwards:   # (<= 0: the reference warns and leaves vx alone)
        ratio_x = -max_vel_x_backwards / vx
    if use_proportional_saturation:
        ratio = min(min(ratio_x, ratio_y), ratio_omega)
        vx, vy, omega = vx * ratio, vy * ratio, omega * ratio
    else:
        vx, vy, omega = vx * ratio_x, vy * ratio_y, omega * ratio_omega
    vel_linear = math.hypot(vx, vy)
    if vel_linear > max_vel_trans:
        k = max_vel_trans / vel_linear
        vx, vy = vx * k, vy * k
    return vx, vy, omega


def steering_angle(v, omega, wheelbase, min_turning_radius):
    """convertTransRotVelToSteeringAngle (:922-933); a radius of exactly 0 gives +-pi / 2 as atan(+-inf) does"""
    import math
    if omega == 0 or v == 0:
        return 0.0
    radius = v / omega
    if abs(radius) < min_turning_radius:
        radius = (1.0 if radius > 0 else (-1.0 if radius < 0 else 0.0)) * min_turning_radius
    if radius == 0:
        return math.copysign(math.pi / 2, wheelbase) * math.copysign(1.0, radius)
    return math.atan(wheelbase / radius)


class HomotopyClassPlanner:
    """Batch view: owns the candidates resident on one GPU (reference homotopy_class_planner.h). Either constructed around a host
    batch (optimizeAllTEBs / selectBestTeb on given bands) or empty (batch=None): plan() then runs the reference's whole tick on the
    device-resident bands - updateAllTEBs, exploreEquivalenceClassesAndInitTebs (incl. the initial-plan candidate), optimizeAllTEBs,
    selectBestTeb (src/homotopy_class_planner.cpp:84-125), incl. randomlyDropTebs (off by default; own random stream - the reference
    seeds from std::random_device) and switching_blocking_period."""

    def __init__(self, cfg, obstacles, via_points, batch=None, device=0, stream=None, max_tebs=None, max_poses=None):
        self.cfg_ = cfg
        self.tebs_ = batch
        self.obstacles_ = obstacles
        self.via_points_ = list(via_points or [])
        if batch is not None:
            self.solver = make_solver(cfg, obstacles, via_points, batch, device=device, stream=stream, max_tebs=max_tebs,
                                      max_poses=max_poses)
        else:
            # pose capacity: 224 keeps the normal matrix as 8x8 blocks in LDS (the fastest layout, <= 238 poses); pass up to _abi.MAX_POSES for longer bands
            self.solver = TebBatchSolver(cfg, max_tebs or max(cfg.hcp.max_number_classes, 1), max_poses or 224, max(len(obstacles), 1),
                                         max(len(obstacles.vert_x), 1), max(len(self.via_points_), 1), device=device, stream=stream)
            self.solver.set_obstacles(obstacles)
            self.solver.set_via_points(self.via_points_)
        self.best_teb_ = -1
        self.initial_plan_teb_ = -1
        self.last_results = None
        self.last_exploration = None
        self._goal = None

    # ---- src/homotopy_class_planner.cpp:539-562 ---------------------------------------------------------------------------------
    def updateAllTEBs(self, start, goal, start_velocity=None):
        import math
        s, t = self.solver, self.cfg_.trajectory
        if s.count > 0 and self._goal is not None:
            d = math.hypot(goal[0] - self._goal[0], goal[1] - self._goal[1])
            a = abs((goal[2] - self._goal[2] + math.pi) % (2 * math.pi) - math.pi)
            if d >= t.force_reinit_new_goal_dist or a >= t.force_reinit_new_goal_angular:
                s.compact_bands(np.zeros(s.count, np.int32))      # tebs_.clear(); equivalence_classes_.clear()
                self.best_teb_ = -1
        if s.count > 0:
            s.update_and_prune(start, goal, t.min_samples)        # every band, one launch
            if start_velocity is not None:
                s.set_velocity_start(start_velocity, True)
        self._goal = tuple(goal)

    # ---- :318-340 (renewAndAnalyzeOldTebs :214-254, deletePlansDetouringBackwards :766-817, createGraph) -------------------------
    def exploreEquivalenceClassesAndInitTebs(self, start, goal, dist_to_obst, start_vel=None, free_goal_vel=False, initial_plan=None):
        s, h = self.solver, self.cfg_.hcp
        if s.count > 0:
            s.h_signatures(h.h_signature_prescaler, values=False)
            keep, _, _ = s.filter_equivalence_classes(h.h_signature_threshold, self.best_teb_, h.max_number_plans_in_current_class)
            if h.delete_detours_backwards:
                keep = s.filter_detours(keep, self.best_teb_)
            if h.selection_dropping_probability > 0:       # randomlyDropTebs (:539-560): every band but the best one, with that probability
                if not hasattr(self, "_rng"):
                    self._rng = np.random.default_rng()
                drop = self._rng.random(len(keep)) <= h.selection_dropping_probability
                drop[self.best_teb_] = False if self.best_teb_ >= 0 else drop[self.best_teb_]
                keep = np.where(drop, 0, keep).astype(np.int32)
            _, self.best_teb_ = s.compact_bands(keep, self.best_teb_)
        self.last_exploration = s.explore_candidates(start, goal, dist_to_obst, start_vel, free_goal_vel, self.best_teb_,
                                                     initial_plan=initial_plan)
        self.initial_plan_teb_ = self.last_exploration["initial_plan_teb"]      # getInitialPlanTEB() of selectBestTeb
        return self.last_exploration["n_total"]

    def plan(self, start, goal, start_vel=None, free_goal_vel=False, initial_plan=None):
        """plan(const PoseSE2& start, const PoseSE2& goal, const geometry_msgs::Twist* start_vel, bool free_goal_vel), :107-125;
        initial_plan = (x, y, yaw) arrays: plan(const std::vector<geometry_msgs::PoseStamped>& initial_plan, ...), :84-96 (start / goal
        are then its first / last pose)."""
        if initial_plan is not None:
            px, py, pyaw = initial_plan
            start = (px[0], py[0], pyaw[0]); goal = (px[-1], py[-1], pyaw[-1])
        o = self.cfg_.optim
        self.solver.set_config(self.cfg_)
        self.updateAllTEBs(start, goal, start_vel)
        self.exploreEquivalenceClassesAndInitTebs(start, goal, self.cfg_.obstacles.min_obstacle_dist, start_vel, free_goal_vel, initial_plan)
        if self.solver.count == 0:
            self.best_teb_ = -1
            return True
        self.optimizeAllTEBs(o.no_inner_iterations, o.no_outer_iterations)
        self.selectBestTeb()
        return True

    def getVelocityCommand(self, look_ahead_poses=None):
        """(ok, vx, vy, omega) of the best band (:127-139)."""
        if self.best_teb_ < 0:
            return False, 0.0, 0.0, 0.0
        t = self.cfg_.trajectory
        ok, v = self.solver.velocity_command(self.best_teb_, t.control_look_ahead_poses if look_ahead_poses is None else look_ahead_poses,
                                             t.prevent_look_ahead_poses_near_goal)
        return ok, float(v[0]), float(v[1]), float(v[2])

    def isTrajectoryFeasible(self, costmap, footprint_spec, inscribed_radius, circumscribed_radius=0.0, look_ahead_idx=-1,
                             feasibility_check_lookahead_distance=-1.0):
        """HomotopyClassPlanner::isTrajectoryFeasible (src/homotopy_class_planner.cpp:686-709): the best band is checked; an infeasible
        one is removed and the next best tried, unless it was already the best band of the previous tick (then False: "not failing could
        result in oscillations between trajectories")."""
        s = self.solver
        if s.count == 0:
            return False
        s.set_costmap(costmap.cells, costmap.resolution, costmap.origin_x, costmap.origin_y)
        feasible = False
        while not feasible and s.count > 0:
            if self.best_teb_ < 0:                       # findBestTeb (:711-723): re-select when the best band is gone
                self.selectBestTeb()
            best = self.best_teb_
            if best < 0:
                return False
            feasible = s.is_trajectory_feasible(best, footprint_spec, inscribed_radius, self.cfg_.trajectory.min_resolution_collision_check_angular,
                                                look_ahead_idx, feasibility_check_lookahead_distance)[0]
            if not feasible:
                same_as_before = getattr(self, "_last_best_teb", -1) == best
                keep = np.ones(s.count, np.int32)
                keep[best] = 0
                s.compact_bands(keep, -1)                # removeTeb (:725-744)
                lb = getattr(self, "_last_best_teb", -1)
                self._last_best_teb = -1 if lb == best else (lb - 1 if lb > best else lb)
                if 0 <= self.initial_plan_teb_:
                    self.initial_plan_teb_ = -1 if self.initial_plan_teb_ == best else self.initial_plan_teb_ - (self.initial_plan_teb_ > best)
                self.best_teb_ = -1
                if same_as_before:
                    return False
        return feasible

    def bands(self, stride=None):
        """Host copy of the resident bands: list of (x, y, theta, dt)."""
        s = self.solver
        if s.count == 0:
            return []
        b = _abi.TebBatchHost(s.count, stride or s.max_poses)
        s.download(b)
        return [b.get_teb(k) for k in range(s.count)]

    def optimizeAllTEBs(self, iter_innerloop, iter_outerloop):
        h = self.cfg_.hcp
        self.solver.optimize(iter_innerloop, iter_outerloop, True, h.selection_obst_cost_scale,
                             h.selection_viapoint_cost_scale, h.selection_alternative_time_cost)

    def selectBestTeb(self, now=None):
        """selectBestTeb (:564-667). now [s]: wall clock for hcp.switching_blocking_period (:648-663: a switch to another candidate is
        only allowed when more than that period has passed since the last switch); None = time.monotonic()."""
        import time
        last = self.best_teb_
        self._last_best_teb = last                       # last_best_teb_ (:566)
        best, _ = self.solver.select_best(self.best_teb_, self.initial_plan_teb_)
        if last >= 0 and best != last:
            now = time.monotonic() if now is None else now
            if now - getattr(self, "_last_switch", 0.0) > self.cfg_.hcp.switching_blocking_period:
                self._last_switch = now
            else:
                best = last        # switching blocked
        self.best_teb_ = best
        return best

    def results(self):
        self.last_results = self.solver.results()
        return self.last_results

    def download(self):
        return self.solver.download(self.tebs_)
