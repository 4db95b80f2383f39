"""FleetHomotopyClassPlanner with robot classes and the _per_class wrappers of TebBatchSolver - what needs no device: what is one per
call must agree over the classes (the ValueError names the class and the field), and the wrappers check their lengths before they
enter the library, as tests/test_fleet_configs.py holds the class-map wrappers to."""
import copy
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import fleet_class_tick_cases as CT  # noqa: E402
import fleet_config_cases as FC  # noqa: E402

from teb_local_planner_amd import planner  # noqa: E402
from teb_local_planner_amd.config import TebConfig  # noqa: E402


def _classes():
    cfgs = FC.point_classes()
    cfgs[1].hcp.switching_blocking_period = 2.0        # what the tick takes per class may differ
    cfgs[2].trajectory.force_reinit_new_goal_dist = 0.5
    return cfgs


def _set(path, value):
    def change(c):
        obj = c
        for name in path[:-1]:
            obj = getattr(obj, name)
        setattr(obj, path[-1], value)
    return change


ONE_PER_CALL = [
    ("simple_exploration", _set(("hcp", "simple_exploration"), True)),
    ("roadmap_graph_no_samples", _set(("hcp", "roadmap_graph_no_samples"), 7)),
    ("roadmap_graph_area_width", _set(("hcp", "roadmap_graph_area_width"), 3.5)),
    ("obstacle_heading_threshold", _set(("hcp", "obstacle_heading_threshold"), 0.2)),
    ("h_signature_prescaler", _set(("hcp", "h_signature_prescaler"), 0.7)),
    ("h_signature_threshold", _set(("hcp", "h_signature_threshold"), 0.3)),
    ("max_number_plans_in_current_class", _set(("hcp", "max_number_plans_in_current_class"), 2)),
    ("viapoints_all_candidates", _set(("hcp", "viapoints_all_candidates"), False)),
    ("allow_init_with_backwards_motion", _set(("trajectory", "allow_init_with_backwards_motion"), True)),
    ("global_plan_overwrite_orientation", _set(("trajectory", "global_plan_overwrite_orientation"), False)),
    ("delete_detours_backwards", _set(("hcp", "delete_detours_backwards"), False)),
    ("max_number_classes", _set(("hcp", "max_number_classes"), 2)),
    ("no_inner_iterations", _set(("optim", "no_inner_iterations"), 3)),
    ("no_outer_iterations", _set(("optim", "no_outer_iterations"), 2)),
    ("optimization_activate", _set(("optim", "optimization_activate"), False)),
    ("xy_goal_tolerance", _set(("goal_tolerance", "xy_goal_tolerance"), 0.35)),
]


def test_every_field_of_hcp_params_is_among_the_cases():
    from teb_local_planner_amd import _abi
    a, b = TebConfig().hcp_params(), TebConfig().hcp_params()
    assert all(getattr(a, k) == getattr(b, k) for k, _ in _abi.HcpParams._fields_)
    # the planner compares EVERY field of the block, whatever the cases above change
    cfgs = _classes()
    seen = {name for name, _, _ in planner.FleetHomotopyClassPlanner._one_per_call(cfgs[0], cfgs[1])}
    assert {k for k, _ in _abi.HcpParams._fields_} <= seen
    assert {"delete_detours_backwards", "max_number_classes", "no_inner_iterations", "no_outer_iterations", "optimization_activate",
            "xy_goal_tolerance"} <= seen


@pytest.mark.parametrize("field,change", ONE_PER_CALL, ids=[f for f, _ in ONE_PER_CALL])
@pytest.mark.parametrize("k", [1, 2])
def test_what_is_one_per_call_must_agree_over_the_classes(field, change, k):
    cfgs = _classes()
    before = copy.deepcopy(cfgs[k])
    change(cfgs[k])
    moved = [name for name, u, v in planner.FleetHomotopyClassPlanner._one_per_call(before, cfgs[k]) if u != v]
    assert field in moved, "the case changes nothing"
    with pytest.raises(ValueError) as e:
        planner.FleetHomotopyClassPlanner(cfgs[0], 6, robot_cfgs=cfgs, class_of_robot=FC.POINTS_CLASS_OF)
    assert "class %d" % k in str(e.value) and field in str(e.value), str(e.value)


def test_the_other_refusals_of_the_planner_come_before_the_handle():
    cfgs = _classes()
    P = planner.FleetHomotopyClassPlanner
    with pytest.raises(ValueError, match="come together"):
        P(cfgs[0], 6, robot_cfgs=cfgs)
    with pytest.raises(ValueError, match="come together"):
        P(cfgs[0], 6, class_of_robot=FC.POINTS_CLASS_OF)
    with pytest.raises(ValueError, match="5 class entries for 6 robots"):
        P(cfgs[0], 6, robot_cfgs=cfgs, class_of_robot=[0] * 5)
    with pytest.raises(ValueError, match="does not fit"):
        P(cfgs[0], 6, robot_cfgs=cfgs, class_of_robot=[0, 1, 2, 3, 0, 0])
    cfgs[2].hcp.selection_dropping_probability = 0.1
    with pytest.raises(ValueError) as e:
        P(cfgs[0], 6, robot_cfgs=cfgs, class_of_robot=FC.POINTS_CLASS_OF)
    assert "class 2" in str(e.value) and "selection_dropping_probability" in str(e.value)
    # costmap_obstacles_behind_robot_dist: one per call unless plan() is given one - checked where the costmaps arrive
    cfgs = _classes()
    cfgs[1].obstacles.costmap_obstacles_behind_robot_dist = 0.7
    fp = object.__new__(P)
    fp.n_robots, fp.robot_cfgs, fp.class_of_robot, fp.cfg_, fp._shared = 6, cfgs, FC.POINTS_CLASS_OF, cfgs[0], cfgs[0]

    class Refuses:   # the solver must not be reached
        def __getattr__(self, name):
            if name == "set_config":
                return lambda cfg: None
            raise AssertionError("the handle was reached: " + name)
    fp.solver = Refuses()
    with pytest.raises(ValueError) as e:
        fp.plan([(0, 0, 0)] * 6, [(1, 0, 0)] * 6, costmaps_per_robot=[None] * 6)
    assert "class 1" in str(e.value) and "costmap_obstacles_behind_robot_dist" in str(e.value)
    # one value, or one per class
    assert fp._of_class(0.25, 1) == 0.25 and fp._of_class([0.2, 0.3, 0.4], 1) == 0.3
    tri, rect = [(0.4, 0.0), (-0.2, 0.25), (-0.2, -0.25)], [(-0.3, -0.25), (0.9, -0.25), (0.9, 0.25), (-0.3, 0.25)]
    assert fp._of_class(tri, 2, 2) == tri and fp._of_class([tri, rect, tri], 1, 2) == rect
    with pytest.raises(ValueError, match="2 entries for 3 classes"):
        fp._of_class([0.2, 0.3], 0)
    assert fp.cfg_of(1) is cfgs[FC.POINTS_CLASS_OF[1]]
    assert "homogeneous" not in P.__doc__.split("heterogeneous")[0]


def _unbound_solver(n_scenes):
    s = object.__new__(planner.TebBatchSolver)
    s._h = None
    s.cfg = TebConfig()
    s._n_scenes = n_scenes
    s.count = 0
    return s


def test_wrappers_check_lengths_before_the_library_is_entered():
    s = _unbound_solver(8)
    st, gl = np.zeros((8, 3)), np.ones((8, 3))
    with pytest.raises(ValueError, match="starts"):
        s.explore_candidates_per_class(st[:-1], gl)
    with pytest.raises(ValueError, match="goals"):
        s.explore_candidates_per_class(st, gl[:5])
    with pytest.raises(ValueError, match="required"):
        s.explore_candidates_per_class(None, gl)
    with pytest.raises(ValueError, match="start velocities"):
        s.explore_candidates_per_class(st, gl, start_vels=np.zeros((3, 3)))
    with pytest.raises(ValueError, match="best"):
        s.explore_candidates_per_class(st, gl, best=[-1] * 9)
    with pytest.raises(ValueError, match="initial plans"):
        s.explore_candidates_per_class(st, gl, initial_plans=[None] * 7)
    with pytest.raises(ValueError, match="starts"):
        s.update_and_prune_per_class(st[:-1], gl)
    with pytest.raises(ValueError, match="values per scene"):
        s.update_and_prune_per_class(st, np.ones((8, 2)))
    with pytest.raises(ValueError, match="start velocity flags"):
        s.update_and_prune_per_class(st, gl, st, [1] * 7)
    specs = CT.feasibility_specs()
    with pytest.raises(ValueError, match="bands"):
        s.is_trajectory_feasible_per_class([0] * 7, specs, CT.FEAS_SPEC_OF)
    with pytest.raises(ValueError, match="required"):
        s.is_trajectory_feasible_per_class(None, specs, CT.FEAS_SPEC_OF)
    with pytest.raises(ValueError, match="at least one spec"):
        s.is_trajectory_feasible_per_class([0] * 8, [], None)
    with pytest.raises(ValueError, match="spec entries"):
        s.is_trajectory_feasible_per_class([0] * 8, specs, CT.FEAS_SPEC_OF[:-1])
    with pytest.raises(ValueError, match="does not fit the 3 specs"):
        s.is_trajectory_feasible_per_class([0] * 8, specs, [0, 1, 2, 3, 0, 0, 0, 0])
    with pytest.raises(ValueError, match="does not fit the 3 specs"):
        s.is_trajectory_feasible_per_class([0] * 8, specs, [0, 1, 2, -1, 0, 0, 0, 0])
