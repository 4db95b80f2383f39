"""Inputs ON the thresholds of the band producers and read-outs (tests/hp_strip.py restates them; tests/golden/make_hp_strip.py writes
what it gives on these cases into tests/golden/hp_strip_<family>.npz; tests/test_hp_strip.py asserts what the cases cover). NOT a test file.

CASES: name -> dict. The name's first word is the family: line, plan, path, prune, cons (the read-outs), lanes (bands across the 256
lanes of a workgroup, up to MAX_POSES), fleet (members of the FLEETS below). Every case has
  op      "line" | "plan" | "path" | "prune" | "cons"
  cap     the pose capacity of the handle it runs on (16: the capacity cases, 64, MAX_POSES)
  rungs   the kinds (hp_strip.RUNG_KINDS) whose comparison the case puts on a rounded rung ON PURPOSE
  ref     False where the reference's own code cannot run the case: it asserts dt > 0 when a time difference is added, and it cannot hold
          a band that was not built by its own functions
and the arguments of its op. Coordinates, time differences and velocities are binary fractions wherever a tie or an exact outcome is
wanted; all magnitudes stay below 100.
"""
import math

import numpy as np

MAX_POSES = 944      # TEB_AMD_MAX_POSES (checked against _abi in the CPU test)
LANES = 256          # TEB_AMD_THREADS
PI = math.pi
FAMILIES = ["line", "plan", "path", "prune", "cons", "lanes", "fleet"]
VS, VG = (0.125, 0.03125, -0.0625), (0.0625, 0.0, 0.015625)
CASES = {}


def up(x, k=1):
    for _ in range(k):
        x = math.nextafter(x, math.inf)
    return x


def down(x, k=1):
    for _ in range(k):
        x = math.nextafter(x, -math.inf)
    return x


def _add(name, **kw):
    assert name not in CASES and name.split("_")[0] in FAMILIES, name
    kw.setdefault("rungs", ())
    kw.setdefault("ref", True)
    CASES[name] = kw


# ---- line: initTrajectoryToGoal(start, goal, diststep, max_vel_x, min_samples, guess_backwards_motion) ----------------------------------------
def line(name, start, goal, diststep, max_vel_x=0.5, min_samples=3, back=False, cap=64, **kw):
    _add(name, op="line", start=tuple(map(float, start)), goal=tuple(map(float, goal)), diststep=float(diststep), max_vel_x=float(max_vel_x),
         min_samples=int(min_samples), back=bool(back), cap=cap, **kw)


Z = (0.0, 0.0, 0.0)
line("line_diststep_0", Z, (1.0, 0.5, 0.3), 0.0)
line("line_diststep_negative_vel_0", Z, (1.0, 0.0, 0.0), -0.25, max_vel_x=0.0)      # the samples step AWAY from the goal; timestep stays 0.1
line("line_diststep_negative", Z, (1.125, 0.0, 0.0), -0.25, ref=False)               # timestep = diststep / max_vel_x < 0
line("line_vel_0", Z, (1.125, 0.5, 0.0), 0.25, max_vel_x=0.0)
line("line_back_tie_goal_straight_left", Z, (0.0, 1.125, 0.0), 0.25, back=True)      # dot = 0 * 1 + 1.125 * 0: exactly 0, no flip
line("line_back_goal_behind", Z, (-1.0, 0.25, 0.0), 0.25, back=True)
line("line_back_goal_ahead", Z, (1.0, 0.25, 0.0), 0.25, back=True)
line("line_back_off_goal_behind", Z, (-1.0, 0.25, 0.0), 0.25, back=False)
line("line_flip_of_dir_0_wraps_to_minus_pi", (0.0, 0.0, PI), (1.125, 0.0, 0.0), 0.25, back=True)   # normalize_theta(0 + M_PI): M_PI < M_PI is false
line("line_flip_of_negative_dir_stays_in_range", (0.0, 0.0, PI), (1.0, -0.5, 0.0), 0.25, back=True)
line("line_flip_of_positive_dir_wraps", (0.0, 0.0, PI), (1.0, 0.5, 0.0), 0.25, back=True)
line("line_quotient_0.9_0.3_lands_on_3", Z, (0.9, 0.0, 0.0), 0.3, rungs=("steps_floor", "steps_drop"))
line("line_quotient_2.0_0.5_is_4", Z, (2.0, 0.0, 0.0), 0.5)
line("line_quotient_0.3_0.1_below_3", Z, (0.3, 0.0, 0.0), 0.1, rungs=("steps_floor",))
line("line_quotient_0.6_0.2_below_3", Z, (0.6, 0.0, 0.0), 0.2, rungs=("steps_floor",))
line("line_quotient_1.2_0.4_below_3", Z, (1.2, 0.0, 0.0), 0.4, rungs=("steps_floor",))


def _floor_rung():
    """(goal x, diststep) whose quotient is 3.0 in fp64 and below 3 exactly: fp64 floors to 3 where the exact floor is 2"""
    from fractions import Fraction
    for k in range(1, 400):
        b = k / 128.0 + 0.1
        a = down(3 * b)
        for a in (a, up(a), up(a, 2)):
            if a / b == 3.0 and Fraction(a) / Fraction(b) < 3 and math.sqrt(a * a) == a:
                return a, b
    raise AssertionError("no rung")


_A, _B = _floor_rung()
line("line_quotient_lands_on_3_from_below", Z, (_A, 0.0, 0.0), _B, rungs=("steps_floor", "steps_drop"))
line("line_quotient_one_ulp_above_3", Z, (up(0.75), 0.0, 0.0), 0.25)
line("line_quotient_one_ulp_below_3", Z, (down(0.75), 0.0, 0.0), 0.25)
line("line_quotient_2.5", Z, (0.625, 0.0, 0.0), 0.25)                               # rounding the quotient gives 3 (ties away) - floor gives 2
line("line_quotient_2.75", Z, (0.6875, 0.0, 0.0), 0.25)
line("line_negative_vel", Z, (1.125, 0.5, 0.0), 0.25, max_vel_x=-0.5, min_samples=8)
line("line_no_steps_0", Z, (0.125, 0.0, 0.5), 0.25)
line("line_no_steps_1_dropped", Z, (0.25, 0.0, 0.5), 0.25)                           # the start only, then the tail
line("line_start_equals_goal", (1.0, 2.0, 0.5), (1.0, 2.0, 0.5), 0.25, max_vel_x=0.0, back=True)
line("line_start_equals_goal_dt_0", (1.0, 2.0, 0.5), (1.0, 2.0, 0.5), 0.25, ref=False)
line("line_tail_n_is_min_samples_minus_1", Z, (0.375, 0.0, 0.25), 0.25, min_samples=3)     # 2 poses before the goal: no insert
line("line_tail_n_is_min_samples_minus_2", Z, (0.375, 0.0, 0.25), 0.25, min_samples=4)     # one insert
line("line_tail_min_samples_2", Z, (0.125, 0.25, 0.25), 0.25, min_samples=2)               # start and goal
line("line_tail_min_samples_3", Z, (0.125, 0.25, 0.25), 0.25, min_samples=3)
line("line_tail_40_inserts", Z, (2.0, 1.0, 0.75), 0.0, min_samples=42)
line("line_tail_inserts_vel_0", Z, (2.0, 1.0, 0.75), 0.0, max_vel_x=0.0, min_samples=6)
line("line_capacity_goal_in_the_last_slot", Z, (3.625, 0.0, 0.0), 0.25, cap=16)
line("line_capacity_one_more", Z, (3.875, 0.0, 0.0), 0.25, cap=16)
line("line_capacity_samples", Z, (10.125, 0.0, 0.0), 0.25, cap=16)
line("line_capacity_tail_insert", Z, (2.0, 1.0, 0.75), 0.0, min_samples=20, cap=16)
line("line_capacity_tail_fills_the_last_slot", Z, (2.0, 1.0, 0.75), 0.0, min_samples=16, cap=16)


# ---- plan: initTrajectoryToGoal(plan, max_vel_x, max_vel_theta, estimate_orient, min_samples, guess_backwards_motion) -------------------------
def plan(name, px, py, pyaw, max_vel_x=0.5, max_vel_theta=0.25, estimate=False, min_samples=3, back=False, cap=64, **kw):
    _add(name, op="plan", px=np.array(px, np.float64), py=np.array(py, np.float64), pyaw=np.array(pyaw, np.float64), max_vel_x=float(max_vel_x),
         max_vel_theta=float(max_vel_theta), estimate=bool(estimate), min_samples=int(min_samples), back=bool(back), cap=cap, **kw)


plan("plan_1_pose", [1.0], [2.0], [0.5], max_vel_x=0.0)
plan("plan_1_pose_dt_0", [1.0], [2.0], [0.5], ref=False)
plan("plan_2_poses", [0.0, 1.0], [0.0, 0.5], [0.25, 0.75])
plan("plan_3_poses_yaw_given", [0.0, 0.5, 1.0], [0.0, 0.25, 0.0], [0.25, 0.5, -0.25])
plan("plan_3_poses_yaw_estimated", [0.0, 0.5, 1.0], [0.0, 0.25, 0.0], [0.25, 0.5, -0.25], estimate=True)
plan("plan_5_poses_yaw_estimated", [0.0, 0.5, 1.0, 1.25, 1.5], [0.0, 0.25, 0.0, 0.5, 1.0], [0.25, 0.0, 0.0, 0.0, -0.25], estimate=True)
plan("plan_back_tie_goal_straight_left", [0.0, 0.25, 0.0], [0.0, 0.5, 1.0], [0.0, 0.5, 1.0], estimate=True, back=True)
plan("plan_back_goal_behind_estimated", [0.0, -0.5, -1.0, -1.5], [0.0, 0.25, 0.0, 0.25], [0.0, 0.0, 0.0, 0.5], estimate=True, back=True)
plan("plan_back_goal_behind_given", [0.0, -0.5, -1.0, -1.5], [0.0, 0.25, 0.0, 0.25], [0.0, 3.0, -3.0, 0.5], back=True)
plan("plan_back_goal_ahead", [0.0, 0.5, 1.0, 1.5], [0.0, 0.25, 0.0, 0.25], [0.0, 0.0, 0.0, 0.5], estimate=True, back=True)
plan("plan_estimated_yaw_0_flipped_to_minus_pi", [0.0, -1.0, -0.5, -2.0], [0.0, 0.5, 0.5, 0.0], [0.0, 0.0, 0.0, 0.0], estimate=True, back=True)
plan("plan_vel_0", [0.0, 0.5, 1.0], [0.0, 0.25, 0.0], [0.25, 0.5, -0.25], max_vel_x=0.0)
plan("plan_vel_theta_0", [0.0, 0.5, 1.0], [0.0, 0.25, 0.0], [0.25, 0.5, -0.25], max_vel_theta=0.0)
plan("plan_negative_vel", [0.0, 0.5, 1.0], [0.0, 0.25, 0.0], [0.25, 0.5, -0.25], max_vel_x=-0.5, min_samples=5)
plan("plan_negative_vel_theta", [0.0, 0.5, 1.0], [0.0, 0.25, 0.0], [0.25, 0.5, -0.25], max_vel_theta=-0.25, min_samples=5)
plan("plan_vel_0_vel_theta_0", [0.0, 0.5, 1.0], [0.0, 0.25, 0.0], [0.25, 0.5, -0.25], max_vel_x=0.0, max_vel_theta=0.0)
for _label, _yaw in (("tie", 0.25), ("one_ulp_above", up(0.25)), ("one_ulp_below", down(0.25)), ("rotation_wins", 0.375), ("distance_wins", 0.125)):
    plan("plan_dt_max_" + _label, [0.0, 0.25, 0.75], [0.0, 0.0, 0.0], [0.0, _yaw, 0.0], max_vel_x=0.25, max_vel_theta=0.25)
plan("plan_repeated_point", [0.0, 0.5, 0.5, 1.0], [0.0, 0.25, 0.25, 0.0], [0.0, 0.25, 0.75, 0.0])
plan("plan_repeated_point_estimated", [0.0, 0.5, 0.5, 1.0], [0.0, 0.25, 0.25, 0.0], [0.0, 0.25, 0.75, 0.0], estimate=True)
plan("plan_yaw_difference_pi", [0.0, 0.5, 1.0, 1.5], [0.0, 0.0, 0.0, 0.0], [0.0, PI, 0.0, down(PI)])      # + M_PI, - M_PI, one ulp inside
plan("plan_yaw_difference_7", [0.0, 0.5, 1.0, 1.5], [0.0, 0.0, 0.0, 0.0], [-3.0, 4.0, -3.0, 0.5])           # + 7 and - 7: the floor path
plan("plan_tail_fills", [0.0, 1.0], [0.0, 0.5], [0.25, 0.75], min_samples=6)
plan("plan_tail_fills_estimated_start", [0.0, 0.5, 1.0], [0.0, 0.25, 0.0], [0.25, 0.5, -0.25], estimate=True, min_samples=7)
plan("plan_tail_n_is_min_samples_minus_1", [0.0, 0.5, 1.0], [0.0, 0.25, 0.0], [0.25, 0.5, -0.25], min_samples=3)
plan("plan_tail_n_is_min_samples_minus_2", [0.0, 0.5, 1.0], [0.0, 0.25, 0.0], [0.25, 0.5, -0.25], min_samples=4)
_t = np.arange(18)
plan("plan_capacity_goal_in_the_last_slot", _t[:16] * 0.25, (_t[:16] % 3) * 0.125, (_t[:16] % 5) * 0.125, cap=16)
plan("plan_capacity_one_more", _t[:17] * 0.25, (_t[:17] % 3) * 0.125, (_t[:17] % 5) * 0.125, cap=16)
plan("plan_capacity_two_more", _t[:18] * 0.25, (_t[:18] % 3) * 0.125, (_t[:18] % 5) * 0.125, cap=16)       # refused before the launch
plan("plan_capacity_tail_insert", [0.0, 1.0], [0.0, 0.5], [0.25, 0.75], min_samples=20, cap=16)


# ---- path: the template overload ----------------------------------------------------------------------------------------------------------------
def path(name, px, py, max_vel_x=0.5, acc=None, so=None, go=None, min_samples=3, back=False, cap=64, **kw):
    _add(name, op="path", px=np.array(px, np.float64), py=np.array(py, np.float64), max_vel_x=float(max_vel_x), max_vel_theta=0.25, acc=acc,
         so=so, go=go, min_samples=int(min_samples), back=bool(back), cap=cap, **kw)


_PX, _PY = [0.0, 0.5, 1.0, 1.25, 2.0], [0.0, 0.25, 0.0, 0.5, 0.25]
path("path_start_and_goal_orientation", _PX, _PY, so=0.25, go=-0.5, acc=0.5)
path("path_goal_orientation_only", _PX, _PY, go=-0.5, acc=0.5)
path("path_start_orientation_only", _PX, _PY, so=0.25, acc=0.5)                     # the goal gets start_orient
path("path_no_orientation", _PX, _PY, acc=0.5)
path("path_no_acc", _PX, _PY, so=0.25, go=-0.5)
path("path_2_points", [0.0, 1.0], [0.0, 0.5], so=0.25, go=-0.5, acc=0.5)
path("path_back_goal_behind_with_start_orientation", [0.0, -0.5, -1.0, -2.0], [0.0, 0.25, 0.0, 0.25], so=0.25, acc=0.5, back=True)
path("path_back_goal_behind_without_start_orientation", [0.0, -0.5, -1.0, -2.0], [0.0, 0.25, 0.0, 0.25], acc=0.5, back=True)
path("path_back_goal_ahead", _PX, _PY, so=0.25, acc=0.5, back=True)
path("path_back_tie_goal_straight_left", [0.0, 0.25, 0.0], [0.0, 0.5, 1.0], so=0.0, acc=0.5, back=True)
for _label, _d in (("tie", 1.0), ("one_ulp_above", up(1.0)), ("one_ulp_below", down(1.0)), ("vel_wins", 2.0), ("acc_wins", 0.5)):
    path("path_acc_" + _label, [0.0, _d, _d + 0.5], [0.0, 0.0, 0.0], max_vel_x=0.5, acc=0.5, so=0.0, go=0.0,      # d = 2 v^2 / a = 1: both 2.0
         rungs=("acc",) if "ulp" in _label else ())                                                                  # (the square root rounds)
path("path_acc_tie_on_the_goal_segment", [0.0, 0.5, 1.5], [0.0, 0.0, 0.0], max_vel_x=0.5, acc=0.5, so=0.0, go=0.0)
path("path_repeated_middle_point", [0.0, 0.5, 0.5, 1.0], [0.0, 0.25, 0.25, 0.0], so=0.25, go=0.0, acc=0.5)    # timestep 0 -> 0.2, yaw atan2(0, 0) = 0
path("path_repeated_middle_point_no_acc", [0.0, 0.5, 0.5, 1.0], [0.0, 0.25, 0.25, 0.0], so=0.25, go=0.0)
path("path_repeated_middle_point_backwards", [0.0, -0.5, -0.5, -1.0], [0.0, 0.25, 0.25, 0.0], so=0.25, go=0.0, acc=0.5, back=True)   # ... -M_PI
path("path_negative_vel", _PX, _PY, max_vel_x=-0.5, so=0.25, go=0.0, ref=False)      # every middle timestep < 0 -> 0.2; the goal's is not guarded
path("path_1_halving", [0.0, 1.0], [0.0, 0.5], so=0.25, go=-0.5, acc=0.5, min_samples=3)
path("path_2_halvings", [0.0, 1.0], [0.0, 0.5], so=0.25, go=-0.5, acc=0.5, min_samples=4)
path("path_40_halvings", [0.0, 1.0], [0.0, 0.5], so=0.25, go=-0.5, acc=0.5, min_samples=42)
path("path_tail_n_is_min_samples_minus_1", [0.0, 0.5, 1.0], [0.0, 0.25, 0.0], so=0.25, go=0.0, min_samples=3)
path("path_tail_opposite_headings_average", [0.0, 1.0], [0.0, 0.0], so=0.5, go=0.5 - 3.0, acc=0.5, min_samples=4)
path("path_capacity_goal_in_the_last_slot", _t[:16] * 0.25, (_t[:16] % 3) * 0.125, so=0.0, go=0.0, acc=0.5, cap=16)
path("path_capacity_one_more", _t[:17] * 0.25, (_t[:17] % 3) * 0.125, so=0.0, go=0.0, acc=0.5, cap=16)
path("path_capacity_two_more", _t[:18] * 0.25, (_t[:18] % 3) * 0.125, so=0.0, go=0.0, acc=0.5, cap=16)
path("path_capacity_tail_insert", [0.0, 1.0], [0.0, 0.5], so=0.25, go=-0.5, acc=0.5, min_samples=20, cap=16)


# ---- prune: updateAndPruneTEB ---------------------------------------------------------------------------------------------------------------------
def band(n, x=None, y=None):
    """n poses 0.5 apart along x (or at x, y), headings and time differences all different: a shift by one shows"""
    i = np.arange(n, dtype=np.float64)
    x = i * 0.5 if x is None else np.array(x, np.float64)
    y = np.zeros(n) if y is None else np.array(y, np.float64)
    return x, y, ((i % 23) - 11) * 0.125, 0.25 + (np.arange(max(n - 1, 0)) % 61) / 64.0


def prune(name, b, new_start, new_goal, min_samples=3, cap=64, **kw):
    _add(name, op="prune", band=b, new_start=None if new_start is None else tuple(map(float, new_start)),
         new_goal=None if new_goal is None else tuple(map(float, new_goal)), min_samples=int(min_samples), cap=cap, **kw)


_S2, _G = (1.125, 0.125, 0.75), (4.0, 0.25, -0.5)
prune("prune_start_only", band(8), _S2, None)
prune("prune_goal_only", band(8), None, _G)
prune("prune_start_and_goal", band(8), _S2, _G)              # the goal lands on index n - k - 1
prune("prune_neither", band(8), None, None)
prune("prune_empty_band_stays_empty", band(0), _S2, _G, cap=16, ref=False)
for _d in (-3, 0, 1, 9, 10, 11):   # n - min_samples; the new start lies beyond pose 12: every pose of the search is nearer than the one before
    prune("prune_n_minus_min_samples_%+d" % _d, band(5 + _d), (6.25, 0.125, 0.5), None, min_samples=5)
prune("prune_n_minus_min_samples_+11_pose_11_is_nearest", band(16), (5.5, 0.125, 0.5), None, min_samples=5)      # the nearest pose lies beyond the limit
prune("prune_start_equals_pose_0", band(8), (0.0, 0.0, 0.5), None)
prune("prune_equidistant_from_pose_0_and_pose_1", band(8), (0.25, 0.375, 0.5), None)      # the tie breaks: nothing is pruned
prune("prune_equidistant_from_pose_2_and_pose_3", band(8), (1.25, 0.375, 0.5), _G)
prune("prune_nearer_recedes_nearer_still", band(9, x=[4.0, 3.0, 3.5, 1.0, 0.5, 0.25, 5.0, 6.0, 7.0]), (0.0, 0.0, 0.5), None)   # breaks at the first minimum
prune("prune_min_samples_2_leaves_start_and_goal", band(5), (1.5, 0.0, 0.5), _G, min_samples=2)
# (min_samples 1 would let the search reach the last pose: deleteTimeDiffs(1, n - 1) of n - 1 time differences, which the reference asserts against)


def _near_rung():
    """A pose 1 that is nearer than pose 0 exactly and equally far in fp64: the smallest number of ulps of x that does it"""
    x0, y0 = 0.3, 0.7      # the smaller coordinate moves: a few of its ulps vanish in the sum of squares
    d0 = math.sqrt(x0 * x0 + y0 * y0)
    for k in range(1, 64):
        x1 = down(x0, k)
        if math.sqrt(x1 * x1 + y0 * y0) == d0:
            return k, x1
    raise AssertionError("no rung")


NEAR_RUNG_ULPS, _x1 = _near_rung()
prune("prune_rung_pose_1_nearer_exactly_equal_in_fp64", band(8, x=[0.3, _x1, 0.25, 0.125, 0.0625, 2.0, 3.0, 4.0], y=[0.7] * 8), (0.0, 0.0, 0.5), None,
      rungs=("near",))
prune("prune_rung_pose_1_nearer_by_many_ulps", band(8, x=[0.3, down(0.3, 64), 2.0, 2.5, 3.0, 3.5, 4.0, 4.5], y=[0.7] * 8), (0.0, 0.0, 0.5), None,
      rungs=("near",))


# ---- cons: getVelocityCommand / getVelocityProfile / getFullTrajectory -------------------------------------------------------------------------------
def cons(name, b, look=1, prevent=0, max_vel_y=0.0, dt_ref=0.3, cap=64, **kw):
    _add(name, op="cons", band=tuple(np.array(a, np.float64) for a in b), look=int(look), prevent=int(prevent), max_vel_y=float(max_vel_y),
         dt_ref=float(dt_ref), vs=VS, vg=VG, cap=cap, **kw)


def walk(n, dt=0.25, th=None, step=0.25):
    i = np.arange(n, dtype=np.float64)
    return i * step, (i % 3) * step / 2, ((i % 7) - 3) * 0.25 if th is None else np.array(th, np.float64), np.full(n - 1, dt) if np.isscalar(dt) else np.array(dt, np.float64)


cons("cons_2_poses", walk(2))
cons("cons_2_poses_holonomic", walk(2), max_vel_y=0.3)
cons("cons_1_pose", (np.array([0.5]), np.array([0.25]), np.array([0.75]), np.zeros(0)), ref=False)   # no command; a profile of 2 entries
for _la in (1, 7, 8, 100):          # lim = 7
    cons("cons_look_ahead_%d_of_lim_7" % _la, walk(8), look=_la, dt_ref=16.0)
cons("cons_look_ahead_0", walk(8), look=0, dt_ref=16.0)
cons("cons_prevent_2_makes_lim_0", walk(3), look=3, prevent=2, dt_ref=16.0)
cons("cons_prevent_5_makes_lim_negative", walk(3), look=3, prevent=5, dt_ref=16.0)
cons("cons_prevent_2_lim_5", walk(8), look=6, prevent=2, dt_ref=16.0)
cons("cons_time_tie_at_the_last_counter", walk(4, dt=[0.25, 0.25, 0.25]), look=2, dt_ref=0.25)
cons("cons_time_tie_at_an_earlier_counter", walk(4, dt=[0.5, 0.25, 0.25]), look=2, dt_ref=0.25)
cons("cons_time_rung_six_times_0.2", walk(16, dt=0.2), look=12, dt_ref=0.1, rungs=("la_time",))   # 1.2 against 0.1 * 12 = 1.2000000000000002
cons("cons_time_one_ulp_above_the_tie", walk(6, dt=[0.25, up(0.25, 2), 0.25, 0.25, 0.25]), look=4, dt_ref=0.125)      # the sum is 0.5 + one ulp
cons("cons_time_one_ulp_below_the_tie", walk(6, dt=[0.25, down(0.25, 2), 0.25, 0.25, 0.25]), look=4, dt_ref=0.125)   # cut one pose later
cons("cons_time_cut_separated", walk(8, dt=0.5), look=5, dt_ref=0.25)
cons("cons_first_time_differences_0_look_2", walk(6, dt=[0.0, 0.0, 0.25, 0.25, 0.25]), look=2, ref=False)      # dt <= 0 on the tie: no command
cons("cons_first_time_differences_0_look_3", walk(6, dt=[0.0, 0.0, 0.25, 0.25, 0.25]), look=3, ref=False)
cons("cons_time_difference_0_in_the_middle", walk(6, dt=[0.25, 0.25, 0.0, 0.25, 0.25]), look=1, max_vel_y=0.3, ref=False)
cons("cons_negative_time_difference", walk(6, dt=[-0.25, 0.125, 0.25, 0.25, 0.25]), look=1, ref=False)
cons("cons_negative_sum_turns_positive", walk(6, dt=[-0.25, 0.5, 0.25, 0.25, 0.25]), look=2, dt_ref=16.0, ref=False)
# theta = 0: cos = 1 and sin = 0 exactly. A step along +y gives dir = 0 exactly: sign 0, vx = 0
cons("cons_dir_0_step_along_y", (np.array([0.0, 0.0, 0.25, 0.0]), np.array([0.0, 0.25, 0.25, 0.25]), np.zeros(4), np.full(3, 0.25)), look=1)
cons("cons_dir_positive_and_negative", (np.array([0.0, 0.25, 0.0, -0.25]), np.array([0.0, 0.125, 0.25, 0.25]), np.zeros(4), np.full(3, 0.25)), look=1)
cons("cons_dir_negative_first", (np.array([0.0, -0.25, 0.0]), np.array([0.0, 0.125, 0.25]), np.zeros(3), np.full(2, 0.25)), look=1)
cons("cons_max_vel_y_0", walk(6), look=2, dt_ref=16.0, max_vel_y=0.0)
cons("cons_max_vel_y_1e-300", walk(6), look=2, dt_ref=16.0, max_vel_y=1e-300)
cons("cons_max_vel_y_0.3", walk(6), look=2, dt_ref=16.0, max_vel_y=0.3)
_TH = [0.0, PI, 0.0, down(PI), 0.0, 7.0, 0.0, -7.0, 0.25, up(-PI), 0.0]      # differences: +pi, -pi, one ulp inside either end, +-7, beyond 2 pi
cons("cons_angle_differences_on_every_branch", walk(11, th=_TH), look=1)
cons("cons_angle_differences_on_every_branch_holonomic", walk(11, th=_TH), look=1, max_vel_y=0.3)
cons("cons_command_over_an_angle_difference_of_6", walk(4, th=[-3.0, 0.5, 3.0, 0.25]), look=2, dt_ref=16.0)
cons("cons_command_over_an_angle_difference_of_minus_6", walk(4, th=[3.0, 0.5, -3.0, 0.25]), look=2, dt_ref=16.0, max_vel_y=0.3)
cons("cons_command_over_an_angle_difference_of_pi", walk(4, th=[0.0, 0.5, PI, 0.25]), look=2, dt_ref=16.0)


# ---- lanes: bands across the 256 lanes of the workgroup -----------------------------------------------------------------------------------------
for _idx in (255, 256, 257, 513):      # the last sample at this index, the goal behind it
    line("lanes_line_last_sample_at_%d" % _idx, (0.0, 0.5, 0.0), (_idx * 0.0625 + 0.03125, 0.5, 0.25), 0.0625, cap=MAX_POSES)
for _n in (256, 257, 258):
    _i = np.arange(_n)
    plan("lanes_plan_%d_poses" % _n, _i * 0.0625, (_i % 4) * 0.03125, ((_i % 9) - 4) * 0.25, estimate=False, cap=MAX_POSES)
    plan("lanes_plan_%d_poses_estimated" % _n, _i * 0.0625, (_i % 4) * 0.03125, ((_i % 9) - 4) * 0.25, estimate=True, cap=MAX_POSES)
    path("lanes_path_%d_poses" % _n, _i * 0.0625, (_i % 4) * 0.03125, so=0.25, go=0.0, acc=0.5, cap=MAX_POSES)
for _k in (1, 10):
    for _m in (256, 257):              # n - k poses remain
        prune("lanes_prune_k_%d_leaves_%d" % (_k, _m), band(_m + _k, x=np.arange(_m + _k) * 0.0625), (_k * 0.0625, 0.03125, 0.5), _G, cap=MAX_POSES)
prune("lanes_prune_k_10_of_max_poses", band(MAX_POSES, x=np.arange(MAX_POSES) * 0.0625), (10 * 0.0625, 0.03125, 0.5), _G, cap=MAX_POSES)
prune("lanes_prune_k_3_of_max_poses_start_only", band(MAX_POSES, x=np.arange(MAX_POSES) * 0.0625), (3 * 0.0625, 0.03125, 0.5), None, cap=MAX_POSES)
for _n in (255, 256, 257, MAX_POSES):
    cons("lanes_readout_%d_poses" % _n, walk(_n, dt=0.0625 + (np.arange(_n - 1) % 5) / 256.0, step=0.0625), look=3, cap=MAX_POSES, max_vel_y=0.0 if _n % 2 else 0.3)


# ---- fleet: the prune and read-out cases as bands of several scenes -------------------------------------------------------------------------------
# FLEETS: name -> dict(entry, members (cases, one band each, scene s = band s), and what the call shares)
FLEETS = {}
_FS = [(6.25, 0.125, 0.5), (0.25, 0.375, 0.5), (1.125, 0.125, 0.75), (5.5, 0.125, 0.5)]
_FG = [(9.0, 0.25, -0.5), (4.0, 0.5, 0.25), (4.5, -0.25, 0.0), (8.0, 0.0, 1.0)]
for _s, _n in enumerate((15, 8, 9, 16)):
    prune("fleet_scene_prune_%d" % _s, band(_n), _FS[_s], _FG[_s], min_samples=5)
FLEETS["per_scene"] = dict(entry="update_and_prune_per_scene", members=["fleet_scene_prune_%d" % s for s in range(4)], min_samples=5)
for _s, _n in enumerate((15, 8, 16, 2)):
    prune("fleet_all_prune_%d" % _s, band(_n), (5.5, 0.125, 0.5), _G, min_samples=5)
FLEETS["all_bands"] = dict(entry="update_and_prune", members=["fleet_all_prune_%d" % s for s in range(4)], min_samples=5)
# two classes: min_samples 4 and 3. Bands of 14 poses: n - min_samples = 10 and 11; bands of 13: 9 and 10 (the search ends one pose apart)
for _s, (_n, _ms) in enumerate(((14, 4), (14, 3), (13, 4), (13, 3))):
    prune("fleet_class_prune_%d" % _s, band(_n), (6.25, 0.125, 0.5), _FG[_s], min_samples=_ms)
FLEETS["per_class"] = dict(entry="update_and_prune_per_class", members=["fleet_class_prune_%d" % s for s in range(4)], class_min_samples=[4, 3],
                           class_of_scene=[0, 1, 0, 1])
# two classes that differ in max_vel_y and dt_ref, in one launch
for _s, (_vy, _ref, _dt0) in enumerate(((0.0, 0.25, 0.25), (0.3, 0.125, 0.125), (0.0, 0.25, 0.5), (0.3, 0.125, 0.25))):   # scenes 2 and 3: cut by time
    cons("fleet_class_cmd_%d" % _s, walk(6 + _s, dt=[_dt0] + [0.25] * (4 + _s)), look=2, max_vel_y=_vy, dt_ref=_ref)
FLEETS["commands"] = dict(entry="velocity_commands", members=["fleet_class_cmd_%d" % s for s in range(4)], class_max_vel_y=[0.0, 0.3],
                          class_dt_ref=[0.25, 0.125], class_of_scene=[0, 1, 0, 1], look=2, prevent=0)


# ---- running a case through the restatement --------------------------------------------------------------------------------------------------------
def evaluate(case, mode="both", mut=None):
    """(result, Strip). result: ("refused", where) | ("band", x, y, th, dt) as lists of numbers | ("cons", cmd (ok, vx, vy, om) or None,
    profile rows, trajectory rows or None)"""
    import hp_strip as HS
    c = case
    k = HS.Strip(c["rungs"], mode, mut)
    op = c["op"]
    try:
        if op == "line":
            b = k.run(HS.Strip.init_line, c["start"], c["goal"], c["diststep"], c["max_vel_x"], c["min_samples"], c["back"], c["cap"])
        elif op == "plan":
            if len(c["px"]) > c["cap"] + 1:          # the plan does not fit the staging buffers: refused before anything runs
                return ("refused", "host"), k
            b = k.run(HS.Strip.init_plan, c["px"], c["py"], c["pyaw"], c["max_vel_x"], c["max_vel_theta"], c["estimate"], c["min_samples"], c["back"], c["cap"])
        elif op == "path":
            if len(c["px"]) > c["cap"] + 1:
                return ("refused", "host"), k
            b = k.run(HS.Strip.init_path, c["px"], c["py"], c["max_vel_x"], c["max_vel_theta"], c["acc"], c["so"], c["go"], c["min_samples"], c["back"], c["cap"])
        elif op == "prune":
            b = k.run(HS.Strip.prune, *c["band"], c["new_start"], c["new_goal"], c["min_samples"])
        else:
            x, y, th, dt = c["band"]
            cmd = k.run(HS.Strip.velocity_command, x, y, th, dt, c["max_vel_y"], c["dt_ref"], c["look"], c["prevent"])
            prof = k.run(HS.Strip.velocity_profile, x, y, th, dt, c["max_vel_y"], c["vs"], c["vg"])
            traj = k.run(HS.Strip.full_trajectory, x, y, th, dt, c["max_vel_y"], c["vs"], c["vg"]) if len(x) != 1 else None
            return ("cons", cmd, prof, traj), k
    except HS.Refused as e:
        return ("refused", str(e)), k
    return ("band",) + tuple(b), k
