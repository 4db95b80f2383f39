"""Cases of tests/test_hp_lm_trial.py and tests/test_gpu_hp_lm_trial.py. NOT a test file.

A SCENE is one band on the compact scenes of tests/hp_solve_cases.py (steps that are large against the rounding of the state) with
one launch of one LM iteration (teb_autosize off, inner = outer = 1); it has one fixture entry (tests/golden/hp_lm_trial_*.npz), which
does not depend on the layout. A RUN is a scene in one layout with one set of options: RUNS[name] = (scene, layout, extra options).
Every run sets multi_cu = -1 and speculative_trials = -1 (the distance helpers are left out on purpose: DESIGN.md section 8 has their
open defect), except the solver-helper runs.

Pose counts: 3 (one free pose), 5, 64, 65 (a wavefront either side), 255 .. 258 (the workgroup's 256 lanes and the first pose a lane
owns twice), the capacities' neighbours 238, 337, 338, and 513 in the HBM layout alone. Each runs in the layouts that hold it (blocks in
LDS: <= 238 poses, band in LDS: <= 337, band in HBM: all); n <= 65 also in the host's own pick.
Edge families, n = 17 each on top of the default scene: see FAMILIES.
Rejected first trial: "rough" scenes (independent uniform perturbations: the linear model of the first trial is poor), seeds found with
the oracle; tests/test_hp_lm_trial.py asserts k >= 2 for them and k >= 3 for one.
Further down: the solver-helper runs (HELPERS), two outer iterations (OUTER2) and three ragged bands in one launch, as one scene and as
a fleet batch of two scenes (RAGGED, FLEET); the GPU test has a function of its own for the last two.
"""
import numpy as np

from teb_local_planner_amd import _abi
from teb_local_planner_amd.config import RobotFootprintModel

import hp_solve_cases as SC
from hp_linearize_cases import LAYOUT_INDEX  # noqa: F401

SIZES = (3, 5, 64, 65, 238, 255, 256, 257, 258, 337, 338, 513)
CAPACITY = {"cr": 238, "band": 337, "bandg": 944}
LAYOUTS = ("cr", "band", "bandg")
SHORT = 65          # up to here a scene also runs in the host's own pick
FAMILY_N = 17


def _two_circles(cfg, obst, via, batch):
    cfg.robot_model = RobotFootprintModel.two_circles(0.2, 0.12, 0.1, 0.15)


def _via(cfg, obst, via, batch):
    n = int(batch.n[0])
    cfg.optim.weight_viapoint = 1.0
    batch.via_points_enabled[0] = 1
    for i, off in ((n // 3, 0.3), (2 * n // 3, -0.25)):
        via.append((float(batch.x[0, i]) + 0.05, float(batch.y[0, i]) + off))


def _holonomic(cfg, obst, via, batch):
    cfg.robot.max_vel_y = 0.2
    cfg.robot.acc_lim_y = 0.3
    cfg.optim.weight_kinematics_nh = 1.0


def _carlike(cfg, obst, via, batch):
    cfg.robot.min_turning_radius = 0.6


def _carlike_exact(cfg, obst, via, batch):
    cfg.robot.min_turning_radius = 0.6
    cfg.trajectory.exact_arc_length = True


def _shortest_vor(cfg, obst, via, batch):
    cfg.optim.weight_shortest_path = 0.7
    cfg.optim.weight_velocity_obstacle_ratio = 3.0
    cfg.obstacles.obstacle_proximity_lower_bound, cfg.obstacles.obstacle_proximity_upper_bound = 0.2, 0.7
    cfg.obstacles.obstacle_proximity_ratio_max_vel = 0.8


def _exponent(cfg, obst, via, batch):
    cfg.optim.obstacle_cost_exponent = 1.7


def _legacy(cfg, obst, via, batch):
    cfg.obstacles.legacy_obstacle_association = True
    cfg.obstacles.obstacle_poses_affected = 6


def _plain_obstacle(cfg, obst, via, batch):
    cfg.obstacles.inflation_dist = 0.5 * cfg.obstacles.min_obstacle_dist   # EdgeObstacle, not the inflated edge


def _static(cfg, obst, via, batch):
    cfg.obstacles.include_dynamic_obstacles = False


def _rotdir(cfg, obst, via, batch):
    cfg.optim.weight_prefer_rotdir = 50.0
    batch.prefer_rotdir[0] = _abi.ROT_LEFT


# family -> (scene keywords, modification, extra options of its runs)
FAMILIES = {
    "polygon": (dict(footprint="polygon"), None, {}),
    "two_circles": ({}, _two_circles, {}),
    "via_points": ({}, _via, {}),
    "holonomic": ({}, _holonomic, {}),
    "carlike": ({}, _carlike, {}),
    "carlike_exact_arc": ({}, _carlike_exact, {}),
    "shortest_path_velocity_obstacle_ratio": ({}, _shortest_vor, {}),
    "obstacle_cost_exponent": ({}, _exponent, {}),
    "legacy_association": ({}, _legacy, {}),
    "plain_obstacle_edge": ({}, _plain_obstacle, {}),
    "prefer_rotdir": ({}, _rotdir, {}),
}
# (edge type, row) kinds that must be non-zero on some row of the family's graph at the start state (names of hp_linearize.EDGE_NAMES)
FAMILY_ACTIVE = {
    "polygon": [("inflated_obstacle", 0), ("inflated_obstacle", 1)], "two_circles": [("inflated_obstacle", 0), ("dynamic_obstacle", 0), ("dynamic_obstacle", 1)],
    "via_points": [("via_point", 0)], "holonomic": [("velocity_holonomic", 1), ("acceleration_holonomic", 1)],
    "carlike": [("kinematics_carlike", 0), ("kinematics_carlike", 1)], "carlike_exact_arc": [("kinematics_carlike", 0), ("kinematics_carlike", 1)],
    "shortest_path_velocity_obstacle_ratio": [("shortest_path", 0), ("velocity_obstacle_ratio", 0), ("velocity_obstacle_ratio", 1)],
    "obstacle_cost_exponent": [("inflated_obstacle", 0)], "legacy_association": [("inflated_obstacle", 0)],
    "plain_obstacle_edge": [("obstacle", 0)], "prefer_rotdir": [("prefer_rotdir", 0)],
}
# scene -> (n, seed): rough scenes whose first trial the oracle rejects; "rejected3" takes k >= 3
REJECTED = {"rejected_cr": (33, 2), "rejected_band": (65, 3), "rejected_bandg": (129, 3), "rejected3": (17, 1)}
REJECTED_LAYOUT = {"rejected_cr": "cr", "rejected_band": "band", "rejected_bandg": "bandg", "rejected3": "band"}
MIN_K = {"rejected_cr": 2, "rejected_band": 2, "rejected_bandg": 2, "rejected3": 3, "helpers_n120": 2}
# which piece of the lambda factor max(1/3, min(2/3, 1 - (2 rho - 1)^3)) each scene's accepted trial lands on (asserted on the CPU from
# the reference's rho interval, clear of the clamp points): clamped at 1/3, clamped at 2/3, strictly between
KIND = {
    "n3": "third", "n5": "between", "n17": "between", "n64": "between", "n65": "two_thirds", "n238": "two_thirds", "n255": "two_thirds",
    "n256": "between", "n257": "between", "n258": "between", "n337": "two_thirds", "n338": "two_thirds", "n513": "two_thirds",
    "polygon": "third", "two_circles": "two_thirds", "via_points": "between", "holonomic": "between", "carlike": "between",
    "carlike_exact_arc": "between", "shortest_path_velocity_obstacle_ratio": "between", "obstacle_cost_exponent": "third",
    "legacy_association": "between", "plain_obstacle_edge": "between", "prefer_rotdir": "two_thirds", "rejected_cr": "between",
    "rejected_band": "third", "rejected_bandg": "two_thirds", "rejected3": "two_thirds", "helpers_n120": "two_thirds",
    "outer2_n17": "two_thirds", "outer2_polygon": "between", "ragged_n3": "third", "ragged_n17": "between", "ragged_n65": "between",
    "fleet_n17": "between",
}
# solver helpers (speculative_trials = 3, the launch's own multi_cu choice) on a rejected first trial, as hp_solve_cases.HELPERS: one
# scene, one run per LDS layout with the stride of tests/test_gpu_multi_cu.py
HELPERS_SCENE = "helpers_n120"
HELPERS = {"helpers_cr": ("cr", 208), "helpers_band": ("band", 288)}
# two outer iterations: the second graph is built at the state after the first iteration, weight_multiplier = weight_adapt_factor;
# the fixture is of the SECOND iteration (s0: the oracle's state after the first one). Dynamic obstacles are taken as static here
# (include_dynamic_obstacles off): their time stamps would hang on the first iteration's time differences, a dependence the fixture's
# gradient (taken at the final state alone) does not carry.
# (seed 1 of the polygon scene leaves a closest-feature choice of the footprint 1.9e-10 from a tie after the first iteration: the
# reference raises; the next seed is free of it)
OUTER2 = {"outer2_n17": ({}, 1), "outer2_polygon": (dict(footprint="polygon"), 2)}   # (scene keywords, seed)
D1_MAX = 1e-8      # the device state after the first of two outer iterations must be this close to the oracle's (CPU: the forward bound is below it)
SENS_MAX = 1e3     # sup |d rho / d (start state)| in the 1-norm, asserted on the CPU from the reference (observed 575 and 787): with the
RHO_SLACK_MAX = D1_MAX * SENS_MAX   # device's start state d1 from the oracle's, rho moves by <= SENS_MAX d1; the kind holds up to this
# three ragged bands in one launch, n = 3, 17, 65: as one scene (every band against the union of the three default scenes' obstacles)
# and as a fleet batch of two scenes (bands 0 and 2 on that table, band 1 on the obstacles of another seed)
RAGGED = ("ragged_n3", "ragged_n17", "ragged_n65")
FLEET = ("ragged_n3", "fleet_n17", "ragged_n65")
FLEET_SCENE_OF = (0, 1, 0)


def _scenes():
    S = {}
    for n in SIZES:
        S["n%d" % n] = dict(n=n, seed=1, kw={}, mod=None)
    S["n%d" % FAMILY_N] = dict(n=FAMILY_N, seed=1, kw={}, mod=None)
    for fam, (kw, mod, opt) in FAMILIES.items():
        S[fam] = dict(n=FAMILY_N, seed=1, kw=dict(kw), mod=mod)
    for name, (n, seed) in REJECTED.items():
        S[name] = dict(n=n, seed=seed, kw=dict(rough=True), mod=None)
    S[HELPERS_SCENE] = dict(n=SC.HELPERS["cr"][0], seed=SC.HELPERS["cr"][2], kw=dict(rough=True), mod=None)
    for name, (kw, seed) in OUTER2.items():
        S[name] = dict(n=FAMILY_N, seed=seed, kw=dict(kw), mod=_static, outer=2)
    for name in RAGGED:
        S[name] = dict(n=int(name.split("_n")[1]), seed=1, kw={}, mod=None, table="union")
    S["fleet_n17"] = dict(n=17, seed=1, kw={}, mod=None, table="other")
    return S


SCENES = _scenes()


def _runs():
    R = {}

    def add(name, scene, layout, **opt):
        R[name] = (scene, layout, opt)

    for n in SIZES:
        for layout in LAYOUTS:
            if n <= CAPACITY[layout] and not (n == 513 and layout != "bandg"):
                add("n%d_%s" % (n, layout), "n%d" % n, layout)
        if n <= SHORT:
            add("n%d_auto" % n, "n%d" % n, "auto")
    for fam, (kw, mod, opt) in FAMILIES.items():
        add(fam, fam, "auto", **opt)
    add("point_scene_on_the_lds_path", "n%d" % FAMILY_N, "auto")
    add("point_scene_on_the_generic_distance_path", "n%d" % FAMILY_N, "auto", generic_distance_path=True)
    add("no_near_cache", "n%d" % FAMILY_N, "auto", no_near_cache=True)
    add("no_near_cache_polygon", "polygon", "auto", no_near_cache=True)
    add("no_near_cache_two_circles", "two_circles", "auto", no_near_cache=True)   # (5 of its dynamic-obstacle edges are inside min_obstacle_dist)
    for name in REJECTED:
        add(name, name, REJECTED_LAYOUT[name])
    for name, (layout, stride) in HELPERS.items():
        add(name, HELPERS_SCENE, layout, multi_cu=0, speculative_trials=3)
    return R


RUNS = _runs()


def _points(scenes_):
    """one table of the point obstacles of several default scenes, in order"""
    t = _abi.ObstacleTable()
    for n, seed in scenes_:
        o = SC.scene(n, seed)[1]
        for i in range(len(o)):
            t.add_point(o.ax[i], o.ay[i], vel=(o.vx[i], o.vy[i]) if o.dynamic[i] else None)
    return t


def build(scene, stride=None):
    """dict(cfg, obst, via, batch, n) of a scene; stride: of the host batch (the solver-helper runs size their handle with it)"""
    s = SCENES[scene]
    cfg, obst, via, batch = SC.scene(s["n"], s["seed"], stride=stride, **s["kw"])
    via = list(via)
    if s.get("table") == "union":
        obst = _points([(int(name.split("_n")[1]), 1) for name in RAGGED])
    elif s.get("table") == "other":
        obst = _points([(17, 2), (33, 2)])
    if s["mod"] is not None:
        s["mod"](cfg, obst, via, batch)
    return dict(cfg=cfg, obst=obst, via=via, batch=batch, n=s["n"], name=scene, outer=s.get("outer", 1))


def ragged_batch(names):
    """(cfg, [case per band], the three bands in one host batch)"""
    cases = [build(name) for name in names]
    batch = _abi.TebBatchHost(len(cases), 96)
    for b, c in enumerate(cases):
        batch.set_teb(b, *c["batch"].get_teb(0))
        for key in ("has_vel_start", "vel_start", "has_vel_goal", "vel_goal", "prefer_rotdir", "via_points_enabled"):
            getattr(batch, key)[b] = getattr(c["batch"], key)[0]
    return cases[0]["cfg"], cases, batch


def options_of(layout, **opt):
    kw = dict(layout=layout, multi_cu=-1, speculative_trials=-1)
    kw.update(opt)
    return _abi.Options(**kw)


def options(run):
    scene, layout, opt = RUNS[run]
    return options_of(layout, **opt)


def state_of(batch, b=0):
    """[4][n]: x, y, theta, dt (padded with one 0) of band b"""
    n = int(batch.n[b])
    x, y, th, dt = batch.get_teb(b)
    return np.stack([x[:n], y[:n], th[:n], np.append(np.asarray(dt)[:n - 1], 0.0)])
