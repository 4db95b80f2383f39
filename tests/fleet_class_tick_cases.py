"""Fixtures of the whole tick per robot class (include/teb_amd.h: the _per_class calls) - tests/test_fleet_class_tick_cases.py proves on
the CPU, with the oracle, that they discriminate; tests/test_gpu_fleet_class_tick.py runs them on the device. Each takes a fixture the
per-scene tests already use and puts a class map over it whose classes differ in what the call reads from the configuration.

  exploration   fleet_explore_cases.explore_fleet (8 scenes, stride 48) under EXPLORE_CLASS_OF and explore_classes(): three classes that
                differ in min_obstacle_dist (0.2 / 0.35 / 0.1 beside the fixture's DIST_TO_OBST = 0.2), max_vel_x, max_vel_theta,
                acc_lim_x, min_samples (3 against 12, above the vertex count of a short path: the padding of initTrajectoryToGoal runs
                for class 2 only) and weight_viapoint (0 for class 2, which owns PLAN_NEW: an initial plan and two via-points);
  costs         fleet_config_cases' mixed classes with four selection triples, one with selection_alternative_time_cost = 1, one with
                selection_viapoint_cost_scale != 1 on a scene that has via-points;
  feasibility   fleet_tick_cases.feasibility_fleet() with three specs - a rectangle with FEAS_PARAMS[0], a triangle with FEAS_PARAMS[1],
                a single vertex - and FEAS_SPEC_OF;
  pruning       fleet_tick_cases.prune_fleet() with min_samples 3 and 8 per class: a band of 3 to 6 poses lies below 8."""
import copy

import numpy as np

import feasibility_cases
import fleet_config_cases as FC
import fleet_explore_cases as FE
import fleet_tick_cases as FT

# ---- exploration -------------------------------------------------------------------------------------------------------------------
#                   PLAIN FULL LINE AT_GOAL BEST PLAN_NEW PLAN_OLD EMPTY
EXPLORE_CLASS_OF = [2,    0,   2,   0,      1,   2,       1,       1]
EXPLORE_MIN_OBSTACLE_DIST = (0.2, 0.35, 0.1)
EXPLORE_MIN_SAMPLES = (3, 3, 12)


def explore_classes(base):
    """three classes on the configuration of an explore_fleet (which carries the graph and signature parameters of the call)"""
    c0, c1, c2 = copy.deepcopy(base), copy.deepcopy(base), copy.deepcopy(base)
    c0.obstacles.min_obstacle_dist = EXPLORE_MIN_OBSTACLE_DIST[0]
    c1.obstacles.min_obstacle_dist = EXPLORE_MIN_OBSTACLE_DIST[1]
    c1.robot.max_vel_x, c1.robot.max_vel_theta, c1.robot.acc_lim_x = 0.8, 0.6, 0.8
    c2.obstacles.min_obstacle_dist = EXPLORE_MIN_OBSTACLE_DIST[2]
    c2.robot.max_vel_x, c2.robot.max_vel_theta, c2.robot.acc_lim_x = 0.25, 0.15, 0.3
    c2.optim.weight_viapoint = 0.0
    for c, ms in zip((c0, c1, c2), EXPLORE_MIN_SAMPLES):
        c.trajectory.min_samples = ms
    return [c0, c1, c2]


def explore_handle_config(cfgs):
    """the handle's own configuration: no class equals it in any field the exploration reads"""
    c = FC.handle_config_that_differs(cfgs)
    c.robot.max_vel_theta, c.robot.acc_lim_x = 0.45, 0.33
    c.trajectory.min_samples = 7
    c.optim.weight_viapoint = 2.5
    return c


def scene_case(f, cfgs, s):
    """fleet_explore_cases.ExploreFleet.scene_case under the scene's class"""
    case = f.scene_case(s)
    case["cfg"] = cfgs[EXPLORE_CLASS_OF[s]]
    return case


def explore_on_host(oracle, f, cfg, s, us):
    """renewAndAnalyzeOldTebs and the exploration of scene s on the CPU oracle under cfg, dist_to_obst = its min_obstacle_dist:
    (bands before, oracle result). The oracle states the via-point rule for weight_viapoint > 0; at 0 the reference's rule returns before
    it touches a flag (src/homotopy_class_planner.cpp:286-290), so the kept bands keep theirs and a new band its constructor's 0 -
    result["via_enabled"] holds that."""
    from test_reference_pinning import renew_on_host, kept_via_flags
    case = f.scene_case(s)
    case["cfg"] = cfg
    b, n_tebs, best = renew_on_host(oracle, case, slots=8)
    kept = kept_via_flags(oracle, case, b.count)
    o = oracle.explore_candidates(cfg, f.tables[s], b, n_tebs, best, case["start"], case["goal"], unit_samples=us[s], max_paths=f.max_paths,
                                  dist_to_obst=cfg.obstacles.min_obstacle_dist, initial_plan=case["initial_plan"], via_enabled=kept)
    if f.vias[s] and cfg.optim.weight_viapoint <= 0:
        flags = np.zeros(o["n_total"], np.int32)
        flags[:n_tebs] = kept[:n_tebs]
        o["via_enabled"] = flags
    return n_tebs, o


def same_exploration(a, b):
    """two oracle results agree in band count, graph and every band's bits"""
    if a["n_total"] != b["n_total"] or len(a["vertices"]) != len(b["vertices"]) or a["adjacency"] != b["adjacency"]:
        return False
    return all(np.array_equal(u, v) for k in range(a["n_total"]) for u, v in zip(a["batch"].get_teb(k), b["batch"].get_teb(k)))


# ---- costs -------------------------------------------------------------------------------------------------------------------------
# (selection_obst_cost_scale, selection_viapoint_cost_scale, selection_alternative_time_cost) of the four mixed classes
COST_TRIPLES = ((1.0, 1.0, False), (1.0, 1.0, True), (3.0, 0.25, False), (2.0, 1.0, False))   # class 2 owns a scene with via-points and their weight


def cost_classed_fleet(stride=96):
    cf = FC.classed_mixed_fleet(stride)
    for c, (o, v, a) in zip(cf.cfgs, COST_TRIPLES):
        c.hcp.selection_obst_cost_scale, c.hcp.selection_viapoint_cost_scale, c.hcp.selection_alternative_time_cost = o, v, a
    return cf


# ---- feasibility -------------------------------------------------------------------------------------------------------------------
FEAS_SPEC_OF = [0, 1, 2, 1, 2, 0, 1, 2]


def feasibility_specs():
    out = []
    for fp, (radius, ang, look, dist) in ((feasibility_cases.FOOTPRINTS["rect"], FT.FEAS_PARAMS[0]), (feasibility_cases.FOOTPRINTS["tri"], FT.FEAS_PARAMS[1]),
                                          (feasibility_cases.FOOTPRINTS["point1"], (0.3, 0.2, 3, -1.0))):
        out.append(dict(footprint=[tuple(p) for p in fp], inscribed_radius=radius, min_resolution_collision_check_angular=ang, look_ahead_idx=look,
                        feasibility_check_lookahead_distance=dist))
    return out


def spec_args(q):
    """a spec as the positional arguments of the single calls and of the oracle"""
    return (q["footprint"], q["inscribed_radius"], q["min_resolution_collision_check_angular"], q["look_ahead_idx"],
            q["feasibility_check_lookahead_distance"])


# ---- pruning -----------------------------------------------------------------------------------------------------------------------
PRUNE_MIN_SAMPLES = (3, 8)
PRUNE_CLASS_OF = [0, 1, 0, 1, 1]    # the scenes with bands of 3, 4, 5 and 6 poses belong to the class with min_samples = 8


def prune_classes(base):
    out = [copy.deepcopy(base), copy.deepcopy(base)]
    for c, ms in zip(out, PRUNE_MIN_SAMPLES):
        c.trajectory.min_samples = ms
    return out


def as_int32(a):
    return np.asarray(a, np.int32)
