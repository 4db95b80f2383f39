"""The restatement of the adapter arithmetic (tests/plan_window_cases.py) against hand-worked answers, fixture by fixture, hand-written
known answers of saturateVelocity and the steering angle for the product's host code and the restatement alike, and the C-ABI surface of the plan-window calls as far as no GPU is needed. No GPU."""
import ctypes as C
import math
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import plan_window_cases as PW  # noqa: E402
from teb_local_planner_amd import _abi, planner  # noqa: E402

# (window_count, goal_idx, cursor, pruned, via_count) of every fixture, worked by hand from the fixture's geometry - not recomputed.
# Lines of 0.125 with the robot 0.0625 beside pose T: squared distance of pose T + m is (0.125 m)^2 + 0.00390625, so with
# dist_threshold 0.5 the first pose beyond is T + 4 (0.25390625 > 0.25) and the window is T .. T + 4 where the plan lasts; a
# one-pose window counts 2 (the inserted start).
EXPECT = {
    "empty": (0, 0, 0, 1, 0), "one_pose": (2, 0, 0, 1, 0), "two_poses": (2, 1, 0, 1, 0), "three_poses": (2, 2, 0, 1, 0),
    "cursor_at_end": (0, 0, 3, 1, 0),
    "one_pose_window": (2, 2, 0, 0, 0),        # pose 2 is pushed, plan_length = 0.25 > 0.125 ends the loop
    "yaw_branch_5_4": (5, 4, 0, 1, 0), "yaw_branch_5_3": (4, 3, 0, 1, 0), "yaw_branch_5_2": (3, 2, 0, 1, 0), "yaw_branch_5_1": (2, 1, 0, 1, 0),
    "yaw_average_9": (3, 2, 0, 1, 0), "yaw_average_9_edge": (5, 4, 0, 1, 0), "yaw_global_9": (6, 5, 0, 1, 0), "yaw_kept": (3, 2, 0, 1, 0),
    "closest_63_62": (2, 62, 0, 0, 0), "closest_64_62": (2, 63, 0, 0, 0), "closest_64_63": (2, 63, 0, 0, 0),
    "closest_65_62": (3, 64, 0, 0, 0), "closest_65_63": (2, 64, 0, 0, 0), "closest_65_64": (2, 64, 0, 0, 0),
    "closest_255_62": (5, 66, 0, 0, 0), "closest_255_254": (2, 254, 0, 0, 0),
    "closest_256_254": (2, 255, 0, 0, 0), "closest_256_255": (2, 255, 0, 0, 0),
    "closest_257_254": (3, 256, 0, 0, 0), "closest_257_255": (2, 256, 0, 0, 0), "closest_257_256": (2, 256, 0, 0, 0),
    "closest_513_255": (5, 259, 0, 0, 0), "closest_513_256": (5, 260, 0, 0, 0), "closest_513_511": (2, 512, 0, 0, 0),
    "closest_513_512": (2, 512, 0, 0, 0),
    "prune_513_63_0": (5, 4, 63, 1, 0), "prune_513_255_0": (5, 4, 255, 1, 0), "prune_513_256_0": (5, 4, 256, 1, 0),
    "prune_513_300_0": (5, 4, 300, 1, 0), "prune_513_258_3": (5, 4, 258, 1, 0), "prune_257_256_0": (2, 0, 256, 1, 0),
    "prune_65_64_1": (2, 0, 64, 1, 0),
    "window_end_63": (64, 63, 0, 1, 0), "window_end_64": (65, 64, 0, 1, 0), "window_end_255": (256, 255, 0, 1, 0),
    "window_end_256": (257, 256, 0, 1, 0), "window_end_257": (258, 257, 0, 1, 0),
    "length_end_257": (258, 257, 0, 1, 0),     # plan_length after pose k is 0.25 k: pose k + 1 is pushed while 0.25 k <= 64
    "tie_wave_edge": (67, 129, 0, 0, 0),       # poses 63 and 64 mirror the robot: 63 wins, the window is 63 .. 129
    "tie_three": (3, 2, 0, 1, 0),
    "loop_first_minimum": (15, 18, 0, 0, 0),   # pose 4 at 0.2 m (0.04 < 0.05): the scan breaks at pose 5, the window is 4 .. 18
    "loop_global_minimum": (5, 18, 0, 0, 0),   # pose 4 at 0.3 m (0.09): no break, pose 14 at 0.1 m wins, the window is 14 .. 18
    "beyond_threshold": (2, 39, 0, 0, 0),      # the injected goal and the inserted start
    "farther_than_1e5": (5, 4, 0, 0, 0),       # i stays 0 and sq_dist 1e10 <= 1e12: the window starts at pose 0, not at the closest pose 4
    "length_equal_keeps": (5, 6, 0, 0, 0),     # from pose 2: 0.25 (the segment before the window), 0.5, 0.75, 1.0 <= 1.0 keeps pose 6
    "length_equal_from_0": (6, 5, 0, 1, 0),    # from pose 0: 0, 0.25, .. 1.0 <= 1.0 keeps pose 5
    "length_off": (5, 6, 0, 0, 0),
    "via_equal_sep": (9, 8, 0, 1, 8), "via_130_0": (130, 129, 0, 1, 0), "via_130_1": (130, 129, 0, 1, 1), "via_130_40": (130, 129, 0, 1, 40),
    "via_off": (9, 8, 0, 1, 0),
    "prune_none": (32, 39, 0, 0, 0), "prune_at_cursor": (9, 8, 4, 1, 0), "prune_strict": (40, 39, 0, 0, 0),
    "prune_strict_far": (2, 1, 3, 1, 0),       # pose 2 at exactly 1 m is not < 1: pose 3 is the match
    "transform_rigid": (5, 7, 1, 1, 2), "transform_wraps_yaw": (5, 6, 0, 1, 0),
}


def test_every_fixture_has_a_hand_worked_answer():
    assert sorted(EXPECT) == sorted(c.name for c in PW.cases())


@pytest.mark.parametrize("name", sorted(EXPECT))
def test_restatement_gives_the_hand_worked_answer(name):
    r = PW.case(name).restated()
    assert (r["window_count"], r["goal_idx"], r["cursor"], r["pruned"], r["via_count"]) == EXPECT[name]
    assert len(r["window"][0]) == len(r["window"][1]) == len(r["window"][2]) == r["window_count"]
    if r["window_count"]:
        c = PW.case(name)
        assert (r["window"][0][0], r["window"][1][0], r["window"][2][0]) == c.pose                      # the start is the robot pose
        assert (r["window"][0][-1], r["window"][1][-1], r["window"][2][-1]) == r["goal"]


def test_goal_yaw_branches():
    th = [0.15 * k for k in range(9)]
    assert PW.case("yaw_branch_5_4").restated()["goal"][2] == th[4]           # goal_idx = n - 1: the local goal's own yaw
    assert PW.case("yaw_branch_5_3").restated()["goal"][2] == th[4]           # n - 2: the global goal's yaw
    assert PW.case("yaw_branch_5_2").restated()["goal"][2] == th[4]           # n - mal - 1: still the global goal's
    assert abs(PW.case("yaw_branch_5_1").restated()["goal"][2] - 0.225) < 1e-12   # n - mal - 2: headings 0.15 and 0.3
    assert abs(PW.case("yaw_average_9").restated()["goal"][2] - 0.45) < 1e-12     # headings 0.3, 0.45, 0.6
    assert abs(PW.case("yaw_average_9_edge").restated()["goal"][2] - 0.75) < 1e-12
    assert PW.case("yaw_global_9").restated()["goal"][2] == th[8]
    assert PW.case("yaw_kept").restated()["goal"][2] == th[2]                 # no overwrite: the plan's yaw
    # min(moving_average_length, n - goal_idx - 1) never shortens the average: the branch is entered with goal_idx <= n - mal - 2 only


def test_moving_averages_are_well_conditioned():
    """every fixture with a moving-average goal has a resultant >= 0.5: atan2 of the sums is well conditioned, 1e-12 is meaningful"""
    seen = 0
    for c in PW.cases():
        r = c.restated()
        if r["resultant"] is not None:
            seen += 1
            assert r["resultant"] >= 0.5, c.name
    assert seen >= 10


def test_via_points_and_the_tie():
    r = PW.case("via_equal_sep").restated()
    assert r["vias"] == [(0.25 * k, 0.0) for k in range(1, 9)]                # spacing == sep is accepted ('<' skips)
    assert PW.case("via_130_1").restated()["vias"] == [(15.28125, 0.0)]
    v = PW.case("via_130_40").restated()["vias"]
    assert v[0] == (0.375, 0.0) and v[-1] == (15.0, 0.0)
    w = PW.case("tie_wave_edge").restated()["window"]
    assert w[0][1] == 0.125 * 64                                              # the window's second pose: the first was pose 63
    assert PW.case("tie_three").restated()["window"][0][1] == 0.5            # pose 0 won the tie and was replaced by the robot pose


def test_transformed_window():
    c = PW.case("transform_rigid")
    r = c.restated()
    co, si, tx, ty, a = c.tf
    x, y, yaw = c.plan
    k = r["cursor"] + r["goal_idx"]
    assert r["goal"][:2] == ((co * x[k] - si * y[k]) + tx, (si * x[k] + co * y[k]) + ty)
    assert r["global_goal"] == ((co * x[-1] - si * y[-1]) + tx, (si * x[-1] + co * y[-1]) + ty, PW.normalize_theta(yaw[-1] + a))
    w = PW.case("transform_wraps_yaw").restated()
    assert all(-math.pi <= t < math.pi for t in w["window"][2]) and w["global_goal"][2] < 0   # 3.1 + 0.11 wraps


# The known answers below are written out by hand. They hold the product's host code (planner.saturate_velocity / steering_angle, what
# computeVelocityCommands runs) and the restatement the GPU tests compare with (tests/plan_window_cases.py) alike.
IMPLS = {"product": (planner.saturate_velocity, planner.steering_angle) if hasattr(planner, "saturate_velocity") else (None, None),
         "restatement": (PW.saturate_velocity, PW.steering_angle)}


@pytest.mark.parametrize("impl", sorted(IMPLS))
def test_saturate_velocity_known_answers(impl):
    S = IMPLS[impl][0]
    assert S is not None, "planner.saturate_velocity is missing"
    # (vx, vy, omega, max_vel_x, max_vel_y, max_vel_trans, max_vel_theta, max_vel_x_backwards[, use_proportional_saturation])
    assert S(0.25, 0.0, 0.125, 0.5, 0.0, 0.5, 0.25, 0.25) == (0.25, 0.0, 0.125)               # inside every limit
    assert S(1.0, 0.0, 0.5, 0.5, 0.0, 0.5, 0.25, 0.25) == (0.5, 0.0, 0.25)                    # each axis by its own ratio (0.5, 0.5)
    assert S(1.0, 0.0, -0.5, 0.5, 0.0, 0.5, 0.25, 0.25) == (0.5, 0.0, -0.25)                  # omega below -max_vel_theta keeps its sign
    assert S(2.0, 0.0, 0.5, 0.5, 0.0, 0.5, 0.25, 0.25) == (0.5, 0.0, 0.25)                    # ratios 0.25 and 0.5, not proportional
    assert S(2.0, 0.0, 0.5, 0.5, 0.0, 0.5, 0.25, 0.25, True) == (0.5, 0.0, 0.125)             # proportional: the smallest ratio (0.25) on all
    assert S(0.5, 0.0, -1.0, 0.5, 0.0, 0.5, 0.25, 0.25, True) == (0.125, 0.0, -0.25)          # ... here omega's 0.25
    assert S(-0.5, 0.0, 0.0, 0.5, 0.0, 0.5, 0.25, 0.25) == (-0.25, 0.0, 0.0)                  # the backwards limit: ratio 0.5, vx stays negative
    assert S(-1.0, 0.0, 0.5, 0.5, 0.0, 0.5, 1.0, 0.25, True) == (-0.25, 0.0, 0.125)           # ... proportional: 0.25 on omega too
    assert S(-1.0, 0.0, 0.0, 2.0, 0.0, 0.5, 0.25, 0.0) == (-0.5, 0.0, 0.0)                    # max_vel_x_backwards <= 0: only max_vel_trans acts
    assert S(0.5, 0.25, 0.0, 1.0, 0.125, 8.0, 0.25, 0.25) == (0.5, 0.125, 0.0)                # strafing: ratio 0.5
    assert S(0.5, -0.25, 0.0, 1.0, 0.125, 8.0, 0.25, 0.25) == (0.5, -0.125, 0.0)              # ... the other way
    assert S(0.75, 1.0, 0.0, 2.0, 2.0, 0.625, 0.25, 0.25) == (0.375, 0.5, 0.0)                # max_vel_trans 0.625 on the norm 1.25
    assert S(0.0, 0.0, 0.0, 0.5, 0.0, 0.5, 0.25, 0.25) == (0.0, 0.0, 0.0)                     # v = 0
    assert S(0.0, 0.0, 1.0, 0.5, 0.0, 0.5, 0.25, 0.25) == (0.0, 0.0, 0.25)
    assert S(0.25, 0.0, 0.0, 0.5, 0.0, 0.0, 0.25, 0.25) == (0.0, 0.0, 0.0)                    # max_vel_trans = 0 as constructed: vx goes to 0


@pytest.mark.parametrize("impl", sorted(IMPLS))
def test_steering_angle_known_answers(impl):
    A = IMPLS[impl][1]
    assert A is not None, "planner.steering_angle is missing"
    q = math.pi / 4
    assert A(0.0, 0.5, 1.0, 0.5) == 0.0 and A(0.5, 0.0, 1.0, 0.5) == 0.0                      # v = 0 or omega = 0
    assert A(0.5, 0.5, 1.0, 0.5) == q and A(0.5, -0.5, 1.0, 0.5) == -q                        # radius +-1, wheelbase 1: atan(+-1)
    assert A(-0.5, 0.5, 1.0, 0.5) == -q and A(-0.5, -0.5, 1.0, 0.5) == q                      # backwards
    assert A(1.0, 0.5, 2.0, 0.5) == q                                                         # radius 2, wheelbase 2
    assert abs(A(1.0, 0.5, 1.0, 0.5) - 0.4636476090008061) < 1e-15                            # atan(1 / 2)
    assert A(0.125, 0.5, 0.5, 0.5) == q                                                       # radius 0.25 below the minimum 0.5: clamped, atan(0.5 / 0.5)
    assert A(-0.125, 0.5, 0.5, 0.5) == -q                                                     # ... keeping its sign
    assert abs(A(0.125, 0.5, 0.5, 0.0) - 1.1071487177940904) < 1e-15                          # no minimum: atan(0.5 / 0.25) = atan(2)
    assert A(1e-300, 1e300, 1.0, 0.0) == math.pi / 2 and A(-1e-300, 1e300, 1.0, 0.0) == -math.pi / 2   # v / omega underflows: atan(+-inf)
    assert A(-1e-300, 1e300, 1.0, 0.5) == math.pi / 2                                         # sign(-0) = 0: the clamp yields +0


NEW_SYMBOLS = ("teb_amd_set_global_plans", "teb_amd_plan_windows", "teb_amd_get_plan_cursors")
PARAM_HELPERS = ("teb_amd_plan_window_params_default", "teb_amd_sizeof_plan_window_params")


def test_library_exports_the_calls_and_the_params_mirror_matches():
    L = planner.lib()
    for name in NEW_SYMBOLS + PARAM_HELPERS:
        assert hasattr(L, name), name
    assert L.teb_amd_sizeof_plan_window_params() == C.sizeof(_abi.PlanWindowParams)
    p = _abi.PlanWindowParams(2.0, 3.0, 0.5, False, 7)
    L.teb_amd_plan_window_params_default(C.byref(p))
    assert p.struct_size == C.sizeof(_abi.PlanWindowParams)
    d = _abi.PlanWindowParams()
    for k, _ in _abi.PlanWindowParams._fields_:
        assert getattr(p, k) == getattr(d, k), k
    assert (p.global_plan_prune_distance, p.max_global_plan_lookahead_dist, p.global_plan_viapoint_sep,
            p.global_plan_overwrite_orientation, p.moving_average_length) == (1.0, 1.0, -1.0, 1, 3)   # teb_config.h:261-264
    assert L.teb_amd_abi_version() == 3
    for name in ("set_global_plans", "plan_windows", "plan_cursors"):
        assert callable(getattr(planner.TebBatchSolver, name))
    for name in ("setPlans", "computeVelocityCommands", "clearPlanner"):
        assert callable(getattr(planner.FleetHomotopyClassPlanner, name))


def test_a_null_handle_is_refused():
    L = planner.lib()
    assert L.teb_amd_set_global_plans(None, 0, None, None, None, None, None) == _abi.ERR_INVALID_ARG
    assert L.teb_amd_set_global_plans(None, 1, None, None, None, None, None) == _abi.ERR_INVALID_ARG
    assert L.teb_amd_plan_windows(None, 1, None, None, None, None, None, None, None, None, None, None, None, None, None, None, None, 0,
                                  None, None, None, 0) == _abi.ERR_INVALID_ARG
    assert L.teb_amd_get_plan_cursors(None, None) == _abi.ERR_INVALID_ARG
    assert b"null handle" in L.teb_amd_last_error()


def test_every_library_variant_exports_and_refuses_alike():
    """the three calls use no scene state and are part of every variant build() makes: the matrix-core library beside the product"""
    from teb_local_planner_amd import build
    for path in (build.LIB, build.LIB_MFMA):
        assert os.path.exists(path), "%s is missing: __graft_entry__.build() builds it" % os.path.basename(path)
        L = C.CDLL(path)
        for name in NEW_SYMBOLS + PARAM_HELPERS:
            assert hasattr(L, name), (os.path.basename(path), name)
        assert L.teb_amd_sizeof_plan_window_params() == C.sizeof(_abi.PlanWindowParams)
        p = _abi.PlanWindowParams(2.0, 3.0, 0.5, False, 7)
        L.teb_amd_plan_window_params_default.restype = None
        L.teb_amd_plan_window_params_default(C.byref(p))
        assert (p.struct_size, p.global_plan_prune_distance, p.global_plan_viapoint_sep, p.moving_average_length) == (C.sizeof(p), 1.0, -1.0, 3)
        assert L.teb_amd_set_global_plans(None, 1, None, None, None, None, None) == _abi.ERR_INVALID_ARG
        assert L.teb_amd_get_plan_cursors(None, None) == _abi.ERR_INVALID_ARG
