"""FleetHomotopyClassPlanner.computeVelocityCommands on the device: global plans and odometry in, saturated commands and a status per
robot out. Three robots on grids of tests/fleet_tick_cases.py with plans of 40 poses. The entry point equals the hand-composed sequence
- restated windows (tests/plan_window_cases.py), plan(initial_plans, via_per_robot, costmaps_per_robot), isTrajectoryFeasible,
getVelocityCommands, restated saturation - bit for bit in bands, best indices and raw commands: the plans run along +x, so the
moving-average goal yaw is atan2(0, d) = 0 on both sides and no libm result enters a band."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import feasibility_cases  # noqa: E402
import fleet_tick_cases as FT  # noqa: E402
import plan_window_cases as PW  # noqa: E402
from oracle.oracle_py import Costmap  # noqa: E402
from teb_local_planner_amd import _abi, planner  # noqa: E402
from teb_local_planner_amd.config import TebConfig  # noqa: E402

pytestmark = pytest.mark.gpu
R = 3
N_PLAN = 40
SINGLE = dict(generic_config_path=True, multi_cu=-1, speculative_trials=-1)
PARAMS = dict(global_plan_prune_distance=0.25, max_global_plan_lookahead_dist=1.5, global_plan_viapoint_sep=0.5)
FOOTPRINT = feasibility_cases.FOOTPRINTS["tri"]


def _bits(v):
    return np.ascontiguousarray(np.asarray(v, np.float64)).view(np.uint64)


def _same(u, v, what=""):
    u, v = _bits(u), _bits(v)
    assert u.shape == v.shape and np.array_equal(u, v), what


def _cfg():
    cfg = TebConfig()
    cfg.hcp.max_number_classes = 3
    cfg.optim.no_inner_iterations = 3; cfg.optim.no_outer_iterations = 2
    cfg.robot.max_vel_trans = cfg.robot.max_vel_x          # the reference's reconfigure step (src/teb_config.cpp:219-223)
    return cfg


def _grids():
    """a 120 x 120 grid with scattered lethal cells, an all-free 63 x 65 grid, an all-free 120 x 120 grid"""
    return [FT.table_set("six").grids[4], FT.table_set("six").grids[5], FT.table_set("three").grids[1]]


def _plans(grids):
    """40 poses along +x through every grid, from 0.2 to 0.8 of its width; yaws that are only ever copied. In the grid with lethal cells the
    lane lies at 0.7 of the height: its nearest lethal cells are half a metre to the side - they bend the bands and touch no footprint."""
    out = []
    for r, g in enumerate(grids):
        sy, sx = g.cells.shape
        w = sx * g.resolution
        x = g.origin_x + 0.2 * w + (0.6 * w / (N_PLAN - 1)) * np.arange(N_PLAN)
        y = np.full(N_PLAN, g.origin_y + (0.7, 0.5, 0.5)[r] * sy * g.resolution)
        out.append((x, y, 0.01 * (r + 1) * np.ones(N_PLAN)))
    return out


def _thresholds(grids):
    return [max(g.cells.shape[1] * g.resolution / 2.0, g.cells.shape[0] * g.resolution / 2.0) * 0.85 for g in grids]


def _fleet(cfg):
    return planner.FleetHomotopyClassPlanner(cfg, R, max_tebs=3 * R, max_poses=96, max_obstacles=R * 256, max_obstacle_vertices=8,
                                             max_via_points=16, options=_abi.Options(**SINGLE))


def _pose_on(plan, k, yaw=0.0):
    return (float(plan[0][k]), float(plan[1][k]) + 0.02, yaw)


def test_the_entry_point_equals_the_hand_composed_sequence_over_three_ticks():
    cfg = _cfg()
    grids = _grids()
    plans, thr = _plans(grids), _thresholds(grids)
    fleet, ref = _fleet(cfg), _fleet(cfg)
    fleet.setPlans(plans)
    wp = _abi.PlanWindowParams(**dict(PW.DEFAULTS, **PARAMS))
    cursor = [0] * R
    rb, t = cfg.robot, cfg.trajectory
    seen = []
    for tick in range(3):
        poses = [_pose_on(plans[r], 8 * tick + r, 0.05 * r) for r in range(R)]
        vels = [(0.1 * tick, 0.0, 0.02 * r) for r in range(R)]
        status, cmd = fleet.computeVelocityCommands(poses, vels, grids, FOOTPRINT, 0.2, window_params=wp, now=float(tick + 1))
        # the same tick by hand
        wins = [PW.plan_window(plans[r], cursor[r], poses[r], None, thr[r], **PARAMS) for r in range(R)]
        cursor = [w["cursor"] for w in wins]
        best = ref.plan(poses, [w["goal"] for w in wins], vels, None, [w["vias"] for w in wins], False,
                        [tuple(np.array(a) for a in w["window"]) for w in wins], float(tick + 1), grids)
        diverged = ref.hasDiverged()
        feasible = ref.isTrajectoryFeasible(FOOTPRINT, 0.2, 0.0, t.feasibility_check_no_poses, t.feasibility_check_lookahead_distance)
        raw = ref.getVelocityCommands()
        assert list(fleet.solver.plan_cursors()) == cursor, tick
        seen.append(list(cursor))
        got = fleet.last_tick
        for r in range(R):
            assert int(got["windows"]["window_count"][r]) == wins[r]["window_count"] and wins[r]["via_count"] >= 1
            for u, v in zip(got["windows"]["windows"][r], wins[r]["window"]):
                _same(u, v, "tick %d window of robot %d" % (tick, r))
        assert got["planned"] == [bool(b >= 0) for b in best] and got["diverged"] == diverged and got["feasible"] == feasible, tick
        assert list(fleet.best_teb_) == list(ref.best_teb_), tick
        mine, want = fleet.bands(), ref.bands()
        assert len(mine) == len(want) >= R
        for k, (p, q) in enumerate(zip(mine, want)):
            for u, v in zip(p, q):
                _same(u, v, "tick %d band %d" % (tick, k))
        for r in range(R):
            assert got["raw"][r][0] == raw[r][0]
            _same(got["raw"][r][1:], raw[r][1:], "tick %d raw command of robot %d" % (tick, r))
            assert status[r] == fleet.SUCCESS and feasible[r] and raw[r][0], (tick, r, status, feasible, raw)
            sat = PW.saturate_velocity(raw[r][1], raw[r][2], raw[r][3], rb.max_vel_x, rb.max_vel_y, rb.max_vel_trans, rb.max_vel_theta,
                                       rb.max_vel_x_backwards, False)
            _same(cmd[r], sat, "tick %d command of robot %d" % (tick, r))
            assert abs(cmd[r][0]) <= rb.max_vel_x and abs(cmd[r][2]) <= rb.max_vel_theta
        assert list(fleet.no_infeasible_plans_) == [0] * R
    assert all(a < b for a, b in zip(seen[0], seen[2])) and all(a <= b for a, b in zip(seen[0], seen[1])), seen   # the cursors advance
    fleet.solver.close(); ref.solver.close()


def test_a_robot_on_its_goal_stops_and_its_neighbours_do_not_notice():
    cfg = _cfg()
    grids = _grids()
    plans = _plans(grids)
    wp = _abi.PlanWindowParams(**dict(PW.DEFAULTS, **PARAMS))
    out = []
    for on_goal in (True, False):
        fleet = _fleet(cfg)
        fleet.setPlans(plans)
        poses = [_pose_on(plans[r], 5) for r in range(R)]
        if on_goal:
            poses[1] = (float(plans[1][0][-1]), float(plans[1][1][-1]) + 0.02, float(plans[1][2][-1]) + 0.05)
        vels = [(0.05, 0.0, 0.0)] * R
        status, cmd = fleet.computeVelocityCommands(poses, vels, grids, FOOTPRINT, 0.2, window_params=wp, now=1.0)
        bands = fleet.bands()
        out.append((status, cmd, {r: [bands[b] for b in fleet.bands_of(r)] for r in range(R)}, list(fleet.no_infeasible_plans_)))
        fleet.solver.close()
    (sa, ca, ba, na), (sb, cb, bb, nb) = out
    assert sa == ["SUCCESS", "GOAL_REACHED", "SUCCESS"] and sb == ["SUCCESS"] * 3
    assert (ca[1] == 0.0).all() and ba[1] == [] and na == [0, 0, 0] and nb == [0, 0, 0]
    assert (cb[1] != 0.0).any()
    for r in (0, 2):
        _same(ca[r], cb[r], "command of robot %d" % r)
        assert len(ba[r]) == len(bb[r]) >= 1
        for p, q in zip(ba[r], bb[r]):
            for u, v in zip(p, q):
                _same(u, v, "bands of robot %d" % r)


def test_a_moving_robot_on_its_goal_has_not_reached_it():
    """the stopped test of :299: with the odometry above trans_stopped_vel the robot plans on, unless free_goal_vel"""
    cfg = _cfg()
    grids = _grids()
    plans = _plans(grids)
    wp = _abi.PlanWindowParams(**dict(PW.DEFAULTS, **PARAMS))
    fleet = _fleet(cfg)
    fleet.setPlans(plans)
    poses = [(float(p[0][-1]), float(p[1][-1]) + 0.02, float(p[2][-1])) for p in plans]
    vels = [(0.0, 0.0, 0.0), (0.3, 0.0, 0.0), (0.3, 0.0, 0.0)]
    a = planner.adapter_defaults()
    status, _ = fleet.computeVelocityCommands(poses, vels, grids, FOOTPRINT, 0.2, adapter=a, window_params=wp, now=1.0)
    assert status[0] == "GOAL_REACHED" and status[1] != "GOAL_REACHED" and status[2] != "GOAL_REACHED"
    a.free_goal_vel = True
    status, cmd = fleet.computeVelocityCommands(poses, vels, grids, FOOTPRINT, 0.2, adapter=a, window_params=wp, now=2.0)
    assert status == ["GOAL_REACHED"] * 3 and (cmd == 0.0).all()
    fleet.solver.close()


def test_an_infeasible_band_gives_no_valid_command_and_drops_the_bands():
    cfg = _cfg()
    grids = _grids()
    plans = _plans(grids)
    g = grids[2]
    cells = g.cells.copy()
    mx = int((plans[2][0][5] + 0.25 - g.origin_x) / g.resolution)
    cells[:, mx] = 254                                       # a wall across the grid, 0.25 m ahead of robot 2
    grids[2] = Costmap(cells, g.resolution, g.origin_x, g.origin_y)
    square = [(-0.3, -0.3), (0.3, -0.3), (0.3, 0.3), (-0.3, 0.3)]   # reaches the wall from the start pose on
    wp = _abi.PlanWindowParams(**dict(PW.DEFAULTS, **PARAMS))
    fleet = _fleet(cfg)
    fleet.setPlans(plans)
    poses = [_pose_on(plans[r], 5) for r in range(R)]
    vels = [(0.05, 0.0, 0.0)] * R
    status, cmd = fleet.computeVelocityCommands(poses, vels, grids, square, 0.3, window_params=wp, now=1.0)
    assert status[2] == "NO_VALID_CMD" and (cmd[2] == 0.0).all()
    assert fleet.last_tick["planned"][2] and not fleet.last_tick["feasible"][2]
    assert fleet.bands_of(2) == [] and fleet.best_teb_[2] == -1
    assert fleet.no_infeasible_plans_[2] == 1
    assert status[1] == "SUCCESS" and fleet.no_infeasible_plans_[1] == 0 and len(fleet.bands_of(1)) >= 1
    status, _ = fleet.computeVelocityCommands(poses, vels, grids, square, 0.3, window_params=wp, now=2.0)
    assert status[2] == "NO_VALID_CMD" and fleet.no_infeasible_plans_[2] == 2 and fleet.no_infeasible_plans_[1] == 0
    fleet.solver.close()


def test_a_carlike_fleet_gets_proportionally_saturated_steering_commands():
    """cmd_angle_instead_rotvel and use_proportional_saturation: the entry point's command is the restated saturation of the raw command
    followed by the restated steering angle at 0.95 min_turning_radius, bit for bit - and the case is one where limits clip: the raw
    commands of robots that start from rest with a short horizon overshoot max_vel_x or max_vel_theta, as soft constraints let them."""
    import math
    cfg = _cfg()
    cfg.robot.min_turning_radius = 0.5
    cfg.robot.max_vel_theta = 0.2
    grids = _grids()
    plans = _plans(grids)
    wp = _abi.PlanWindowParams(**dict(PW.DEFAULTS, **PARAMS))
    a = planner.adapter_defaults()
    a.cmd_angle_instead_rotvel = True
    a.use_proportional_saturation = True
    a.wheelbase = 0.6
    fleet = _fleet(cfg)
    fleet.setPlans(plans)
    rb = cfg.robot
    clipped = clamped = 0
    for tick in range(3):
        poses = [_pose_on(plans[r], 8 * tick + r, 0.3 - 0.3 * r) for r in range(R)]       # headings off the plan: the bands have to turn
        vels = [(0.1 * tick, 0.0, 0.0)] * R
        status, cmd = fleet.computeVelocityCommands(poses, vels, grids, FOOTPRINT, 0.2, adapter=a, window_params=wp, now=float(tick + 1))
        raw = fleet.last_tick["raw"]
        for r in range(R):
            assert status[r] == fleet.SUCCESS and raw[r][0], (tick, r, status)
            sat = PW.saturate_velocity(raw[r][1], raw[r][2], raw[r][3], rb.max_vel_x, rb.max_vel_y, rb.max_vel_trans, rb.max_vel_theta,
                                       rb.max_vel_x_backwards, True)
            angle = PW.steering_angle(sat[0], sat[2], a.wheelbase, 0.95 * rb.min_turning_radius)
            _same(cmd[r], (sat[0], sat[1], angle), "tick %d robot %d" % (tick, r))
            assert math.isfinite(angle) and abs(angle) <= math.atan(a.wheelbase / (0.95 * rb.min_turning_radius))
            if sat != tuple(raw[r][1:]):
                clipped += 1
                k = sat[0] / raw[r][1]                                                   # proportional: one ratio on vx and omega
                assert k < 1.0 and abs(sat[2] - raw[r][3] * k) <= 1e-15
                assert abs(sat[0]) <= rb.max_vel_x and abs(sat[2]) <= rb.max_vel_theta * (1 + 1e-15)
            if sat[2] != 0 and abs(sat[0] / sat[2]) < 0.95 * rb.min_turning_radius:
                clamped += 1
    assert clipped >= 1, "no command of the case met a velocity limit"
    print("clipped %d, radius clamped %d of %d commands" % (clipped, clamped, 3 * R))
    # a steering angle that is not finite (:437-447; here through a wheelbase that is not a number): zero command, NO_VALID_CMD, the
    # planner of that robot cleared, its counter raised
    a.wheelbase = float("nan")
    poses = [_pose_on(plans[r], 24 + r, 0.3 - 0.3 * r) for r in range(R)]
    status, cmd = fleet.computeVelocityCommands(poses, [(0.3, 0.0, 0.0)] * R, grids, FOOTPRINT, 0.2, adapter=a, window_params=wp, now=4.0)
    turning = [r for r in range(R) if fleet.last_tick["raw"][r][0] and fleet.last_tick["raw"][r][3] != 0 and fleet.last_tick["raw"][r][1] != 0]
    assert turning, "no robot turns in the last tick"
    for r in turning:
        assert status[r] == fleet.NO_VALID_CMD and (cmd[r] == 0.0).all() and fleet.bands_of(r) == [] and fleet.no_infeasible_plans_[r] == 1
    fleet.solver.close()
