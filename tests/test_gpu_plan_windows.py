"""teb_amd_set_global_plans / teb_amd_plan_windows / teb_amd_get_plan_cursors on the device against the sequential restatement of
tests/plan_window_cases.py. Every integer (window_count, goal_idx, cursor, pruned, via_count, offsets) is equal; every position, and
every yaw that is only copied, is bit-equal; yaws that pass atan2 / sin / cos (the moving-average goal) or normalize_theta of a sum (a
transform with yaw_tf != 0) are within 1e-12, the device-libm-against-host bound of tests/test_gpu_strip_ops.py. No case is skipped."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import plan_window_cases as PW  # noqa: E402
from teb_local_planner_amd import _abi, planner  # noqa: E402
from teb_local_planner_amd.config import TebConfig  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1e-12
MAX_ROBOTS = 4


@pytest.fixture(scope="module")
def solver():
    s = planner.TebBatchSolver(TebConfig(), MAX_ROBOTS, 32, 1, 1, 1)
    yield s
    s.close()


def _bits(v):
    return np.ascontiguousarray(np.asarray(v, np.float64)).view(np.uint64)


def _same(u, v, what=""):
    u, v = _bits(u), _bits(v)
    assert u.shape == v.shape and np.array_equal(u, v), what


def _check_robot(o, r, want, yaw_tf, what):
    """robot r of a plan_windows result against its restatement"""
    for k in ("window_count", "goal_idx", "cursor", "pruned", "via_count"):
        assert int(o[k][r]) == want[k], (what, k, int(o[k][r]), want[k])
    wx, wy, wyaw = o["windows"][r]
    _same(wx, want["window"][0], what + ": window x")
    _same(wy, want["window"][1], what + ": window y")
    n = want["window_count"]
    copied = yaw_tf == 0
    averaged = want["resultant"] is not None
    if n:
        _same(wyaw[:1], want["window"][2][:1], what + ": the start's yaw is the robot's")
        if copied:
            _same(wyaw[:n - 1], want["window"][2][:n - 1], what + ": copied yaws")
        assert np.abs(np.asarray(wyaw) - np.asarray(want["window"][2])).max(initial=0.0) <= TOL, what + ": yaws"
    _same(o["goal"][r][:2], want["goal"][:2], what + ": goal position")
    _same(o["global_goal"][r][:2], want["global_goal"][:2], what + ": global goal position")
    if copied:
        _same(o["global_goal"][r][2:], want["global_goal"][2:], what + ": global goal yaw")
        if not averaged:
            _same(o["goal"][r][2:], want["goal"][2:], what + ": goal yaw")
    assert abs(o["goal"][r][2] - want["goal"][2]) <= TOL and abs(o["global_goal"][r][2] - want["global_goal"][2]) <= TOL, what
    if n:
        assert _bits(wyaw[-1:])[0] == _bits(o["goal"][r][2:])[0], what + ": the window's last yaw is the goal yaw"
    _same([p[0] for p in o["vias"][r]], [p[0] for p in want["vias"]], what + ": via x")
    _same([p[1] for p in o["vias"][r]], [p[1] for p in want["vias"]], what + ": via y")


@pytest.mark.parametrize("name", [c.name for c in PW.cases()])
def test_device_equals_the_restatement(solver, name):
    c = PW.case(name)
    solver.set_global_plans([c.plan], [c.begin])
    o = solver.plan_windows([c.pose], [c.thr], c.abi_params(), None if c.tf is None else [c.tf])
    want = c.restated()
    _check_robot(o, 0, want, 0.0 if c.tf is None else c.tf[4], name)
    assert list(o["offset"]) == [0, want["window_count"]] and list(o["via_offset"]) == [0, want["via_count"]]
    assert list(solver.plan_cursors()) == [want["cursor"]]


def test_null_transform_is_the_identity_bit_for_bit(solver):
    for name in ("yaw_average_9", "closest_257_255", "via_130_40", "beyond_threshold"):
        c = PW.case(name)
        outs = []
        for tf in (None, [(1.0, 0.0, 0.0, 0.0, 0.0)]):
            solver.set_global_plans([c.plan], [c.begin])
            outs.append(solver.plan_windows([c.pose], [c.thr], c.abi_params(), tf))
        a, b = outs
        for k in ("window_count", "goal_idx", "cursor", "pruned", "via_count", "offset", "via_offset"):
            assert np.array_equal(a[k], b[k]), (name, k)
        for k in ("win_x", "win_y", "win_yaw", "via_x", "via_y", "goal", "global_goal"):
            _same(a[k], b[k], name + ": " + k)


def test_a_fleet_call_equals_one_call_per_robot(solver):
    plans, poses, tfs, thr, params = PW.fleet_plans()
    p = _abi.PlanWindowParams(**dict(PW.DEFAULTS, **params))
    solver.set_global_plans(plans)
    fleet = solver.plan_windows(poses, thr, p, tfs)
    assert list(fleet["offset"]) == [0] + list(np.cumsum(fleet["window_count"]))
    assert list(fleet["via_offset"]) == [0] + list(np.cumsum(fleet["via_count"]))
    assert list(solver.plan_cursors()) == list(fleet["cursor"])
    for r in range(3):
        want = PW.plan_window(plans[r], 0, poses[r], tfs[r], thr[r], **params)
        _check_robot(fleet, r, want, tfs[r][4], "fleet robot %d" % r)
        solver.set_global_plans([plans[r]])
        one = solver.plan_windows([poses[r]], [thr[r]], p, [tfs[r]])
        for k in ("window_count", "goal_idx", "cursor", "pruned", "via_count"):
            assert one[k][0] == fleet[k][r], (r, k)
        for k in ("goal", "global_goal"):
            _same(one[k][0], fleet[k][r], k)
        for u, v in zip(one["windows"][0], fleet["windows"][r]):
            _same(u, v, "window of robot %d" % r)
        _same(np.array(one["vias"][0]), np.array(fleet["vias"][r]), "vias of robot %d" % r)
    assert fleet["window_count"].min() >= 2 and fleet["via_count"].max() >= 1


def test_the_second_call_starts_from_the_first_calls_cursor(solver):
    plans = [PW.line(40, 0.125), PW.line(300, 0.125), PW.line(65, 0.125)]
    thr = [0.5, 0.5, 0.5]
    params = dict(global_plan_prune_distance=0.125, max_global_plan_lookahead_dist=0.0)
    p = _abi.PlanWindowParams(**dict(PW.DEFAULTS, **params))
    at1, at2 = (3, 100, 10), (9, 260, 64)
    pose = lambda at: [(0.125 * k, 0.0625, 0.1) for k in at]
    solver.set_global_plans(plans)
    first = solver.plan_windows(pose(at1), thr, p)
    assert list(first["cursor"]) == list(at1) and list(solver.plan_cursors()) == list(at1)
    second = solver.plan_windows(pose(at2), thr, p)
    assert list(second["cursor"]) == list(at2) and list(solver.plan_cursors()) == list(at2)
    for r in range(3):
        _check_robot(first, r, PW.plan_window(plans[r], 0, pose(at1)[r], None, thr[r], **params), 0.0, "first call, robot %d" % r)
        _check_robot(second, r, PW.plan_window(plans[r], at1[r], pose(at2)[r], None, thr[r], **params), 0.0, "second call, robot %d" % r)
    # robot 1 gets a new plan; the cursors of robots 0 and 2 travel through `begin`
    begin = solver.plan_cursors()
    begin[1] = 0
    plans[1] = PW.line(50, 0.25)
    solver.set_global_plans(plans, begin)
    assert list(solver.plan_cursors()) == [at2[0], 0, at2[2]]
    at3 = [(0.125 * 9, 0.0625, 0.1), (0.25 * 5, 0.0625, 0.1), (0.125 * 64, 0.0625, 0.1)]
    third = solver.plan_windows(at3, thr, p)
    assert list(third["cursor"]) == [at2[0], 5, at2[2]]
    for r in range(3):
        _check_robot(third, r, PW.plan_window(plans[r], int(begin[r]), at3[r], None, thr[r], **params), 0.0, "third call, robot %d" % r)


def _raw_windows(solver, n, poses, thr, cap_w, cap_v, params=None):
    """the C call with sentinel-filled arrays"""
    I = lambda a: _abi._ptr(a, C.c_int32)
    D = lambda a: _abi._ptr(a, C.c_double)
    poses = _abi.f64(poses).reshape(-1); thr = _abi.f64(thr)
    o = {k: np.full(max(n, 1), -7, np.int32) for k in ("window_count", "goal_idx", "cursor", "pruned", "via_count")}
    o["offset"] = np.full(max(n, 1) + 1, -7, np.int32); o["via_offset"] = np.full(max(n, 1) + 1, -7, np.int32)
    for k in ("win_x", "win_y", "win_yaw", "via_x", "via_y"):
        o[k] = np.full(512, -7.0)
    o["rc"] = planner.lib().teb_amd_plan_windows(solver._h, n, C.byref(params) if params is not None else None, D(poses), None, D(thr),
                                                 I(o["window_count"]), I(o["goal_idx"]), I(o["cursor"]), I(o["pruned"]), None, None, I(o["via_count"]),
                                                 I(o["offset"]), D(o["win_x"]), D(o["win_y"]), D(o["win_yaw"]), cap_w, I(o["via_offset"]),
                                                 D(o["via_x"]), D(o["via_y"]), cap_v)
    return o


def test_arrays_that_do_not_fit_are_left_alone(solver):
    c = PW.case("via_equal_sep")                       # 9 poses, 8 via-points
    p = c.abi_params()
    for cap_w, cap_v, rc in ((8, 8, _abi.ERR_CAPACITY), (9, 7, _abi.ERR_CAPACITY), (9, 8, _abi.OK)):
        solver.set_global_plans([c.plan])
        o = _raw_windows(solver, 1, [c.pose], [c.thr], cap_w, cap_v, p)
        assert o["rc"] == rc
        assert (o["window_count"][0], o["goal_idx"][0], o["cursor"][0], o["pruned"][0], o["via_count"][0]) == (9, 8, 0, 1, 8)
        assert list(o["offset"]) == [0, 9] and list(o["via_offset"]) == [0, 8]
        assert (o["win_x"][:9] == -7.0).all() == (cap_w < 9) and (o["win_x"][9:] == -7.0).all()
        assert (o["via_x"][:8] == -7.0).all() == (cap_v < 8) and (o["via_x"][8:] == -7.0).all()
    o = solver.plan_windows([c.pose], [c.thr], p, capacity_window=3)
    assert o["status"] == _abi.ERR_CAPACITY and o["window_count"][0] == 9


def test_argument_errors_leave_the_previous_set(solver):
    L = planner.lib()
    I = lambda a: _abi._ptr(_abi.i32(a), C.c_int32)
    c = PW.case("length_equal_keeps")
    want = c.restated()
    solver.set_global_plans([c.plan, c.plan])
    x = _abi.f64(np.arange(6.0))
    D = _abi._ptr(x, C.c_double)

    def still_answers():
        o = solver.plan_windows([c.pose, c.pose], [c.thr, c.thr], c.abi_params())
        for r in range(2):
            _check_robot(o, r, want, 0.0, "after a refused call")

    h = solver._h
    bad = [
        (L.teb_amd_set_global_plans(h, -1, I([3]), D, D, D, None), _abi.ERR_INVALID_ARG),                  # n < 0
        (L.teb_amd_set_global_plans(h, MAX_ROBOTS + 1, I([1] * 5), D, D, D, None), _abi.ERR_CAPACITY),     # n > max_tebs
        (L.teb_amd_set_global_plans(h, 2, None, D, D, D, None), _abi.ERR_INVALID_ARG),                     # null counts
        (L.teb_amd_set_global_plans(h, 2, I([3, -1]), D, D, D, None), _abi.ERR_INVALID_ARG),               # a count < 0
        (L.teb_amd_set_global_plans(h, 2, I([3, 3]), D, D, D, I([0, 4])), _abi.ERR_INVALID_ARG),           # a cursor past the end
        (L.teb_amd_set_global_plans(h, 2, I([3, 3]), D, D, D, I([-1, 0])), _abi.ERR_INVALID_ARG),          # a negative cursor
        (L.teb_amd_set_global_plans(h, 2, I([3, 3]), D, None, D, None), _abi.ERR_INVALID_ARG),             # a null array, 6 poses
    ]
    for k, (rc, code) in enumerate(bad):
        assert rc == code, (k, rc)
    still_answers()
    assert L.teb_amd_set_global_plans(h, 2, I([3, 3]), D, D, D, I([0, 3])) == _abi.OK                       # a cursor AT the end is a plan used up
    assert list(solver.plan_cursors()) == [0, 3]
    solver.set_global_plans([c.plan, c.plan])
    # the windows call: another number of robots, null poses / thresholds, a params struct of another size, negative capacities
    assert _raw_windows(solver, 1, [c.pose], [c.thr], 64, 64)["rc"] == _abi.ERR_INVALID_ARG
    assert _raw_windows(solver, 3, [c.pose] * 3, [c.thr] * 3, 64, 64)["rc"] == _abi.ERR_INVALID_ARG
    wrong = c.abi_params()
    wrong.struct_size = 8
    assert _raw_windows(solver, 2, [c.pose] * 2, [c.thr] * 2, 64, 64, wrong)["rc"] == _abi.ERR_INVALID_ARG
    assert _raw_windows(solver, 2, [c.pose] * 2, [c.thr] * 2, -1, 64)["rc"] == _abi.ERR_INVALID_ARG
    assert L.teb_amd_plan_windows(h, 2, None, None, None, None, None, None, None, None, None, None, None, None, None, None, None, 0, None, None, None,
                                  0) == _abi.ERR_INVALID_ARG
    assert L.teb_amd_get_plan_cursors(h, None) == _abi.ERR_INVALID_ARG
    still_answers()
    # no set: both calls refuse; a new set answers again
    solver.set_global_plans([])
    assert _raw_windows(solver, 2, [c.pose] * 2, [c.thr] * 2, 64, 64)["rc"] == _abi.ERR_INVALID_ARG
    b = np.zeros(2, np.int32)
    assert L.teb_amd_get_plan_cursors(h, _abi._ptr(b, C.c_int32)) == _abi.ERR_INVALID_ARG
    solver.set_global_plans([c.plan, c.plan])
    still_answers()


def test_robots_without_a_plan_beside_robots_with_one(solver):
    c = PW.case("yaw_average_9")
    solver.set_global_plans([None, c.plan, ([], [], [])])
    o = solver.plan_windows([c.pose] * 3, [c.thr] * 3, c.abi_params())
    assert list(o["window_count"]) == [0, 3, 0] and list(o["goal_idx"]) == [0, 2, 0] and list(o["offset"]) == [0, 0, 3, 3]
    _check_robot(o, 1, c.restated(), 0.0, "the robot with a plan")
