"""Heterogeneous fleets - a configuration and a footprint per robot class (include/teb_amd.h: teb_amd_set_scene_configs) - the part that
needs no device: the three calls are declared, exported and bound; the Python wrappers check their lengths before they enter the
library; the header states the class map in its fleet section; and the fixtures of tests/fleet_config_cases.py hold what
tests/test_gpu_fleet_configs.py relies on, checked scene by scene with the CPU oracle under the scene's class configuration."""
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import fleet_config_cases as FC  # noqa: E402
import sensitivity  # noqa: E402

from teb_local_planner_amd import _abi, planner  # noqa: E402
from teb_local_planner_amd.config import TebConfig  # noqa: E402

ROOT = os.path.dirname(HERE)
CALLS = ("teb_amd_set_scene_configs", "teb_amd_clear_scene_configs", "teb_amd_get_scene_configs")
THREADS = min(os.cpu_count() or 1, 16)


def _declared(header):
    src = open(os.path.join(ROOT, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return set(re.findall(r"\b(teb_amd_[a-z0-9_]+)\s*\(", src))


def test_calls_are_declared_exported_and_bound():
    L = planner.lib()
    assert set(CALLS) <= _declared("teb_amd.h")
    for n in CALLS:
        assert hasattr(L, n), "libteb_amd.so does not export %s" % n
        assert getattr(L, n).argtypes, "no ctypes signature for %s" % n
    assert len(L.teb_amd_set_scene_configs.argtypes) == 5
    assert len(L.teb_amd_clear_scene_configs.argtypes) == 1
    assert len(L.teb_amd_get_scene_configs.argtypes) == 4
    assert L.teb_amd_abi_version() == 3   # additive
    for name in ("set_scene_configs", "clear_scene_configs", "scene_configs"):
        assert callable(getattr(planner.TebBatchSolver, name))


def test_header_states_the_class_map_in_its_fleet_section():
    src = open(os.path.join(ROOT, "include", "teb_amd.h")).read()
    fleet = src[src.index("Fleet batches: the bands of many scenes"):]
    assert "Configuration and footprint stay per handle (a homogeneous fleet)" not in src
    for m in re.finditer(r"homogeneous fleet", src):   # only ever with the qualification
        assert "class map" in src[max(0, m.start() - 400):m.end() + 400]
    for what in CALLS + ("jacobian_mode", "include_dynamic_obstacles", "TEB_AMD_ERR_UNSUPPORTED", "teb_amd_is_trajectory_feasible_per_scene keeps its one footprint"):
        assert what in fleet, what
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "teb_amd_set_scene_configs" in design


def _unbound_solver(n_scenes):
    """a TebBatchSolver without a handle: the wrappers have to raise before they touch it"""
    s = object.__new__(planner.TebBatchSolver)
    s._h = None
    s.cfg = TebConfig()
    s._n_scenes = n_scenes
    s.count = 0
    return s


def test_wrappers_check_lengths_before_the_library_is_entered():
    cfgs = FC.point_classes()
    s = _unbound_solver(6)
    with pytest.raises(ValueError, match="5 class entries for 6 scenes"):
        s.set_scene_configs(cfgs, [0, 1, 2, 0, 1])
    with pytest.raises(ValueError, match="7 class entries for 6 scenes"):
        s.set_scene_configs(cfgs, [0] * 7)
    with pytest.raises(ValueError, match="at least one class"):
        s.set_scene_configs([], [0] * 6)
    with pytest.raises(ValueError, match="3 classes"):
        s.set_scene_configs(cfgs, [0, 1, 2, 3, 0, 0])
    with pytest.raises(ValueError, match="3 classes"):
        s.set_scene_configs(cfgs, [0, 1, 2, -1, 0, 0])
    with pytest.raises(ValueError, match="class entries"):
        s.set_scene_configs(cfgs, [[0, 1, 2], [0, 1, 2]])
    p = _abi.pack_scene_configs(cfgs, FC.POINTS_CLASS_OF, 6)
    assert (p.n_classes, p.n_scenes) == (3, 6) and p.class_of_scene.dtype == np.int32
    for k, c in enumerate(cfgs):
        assert bytes(p.configs[k]) == bytes(c.to_c())
    # TebFleetPlanner: its own checks come before the handle is made
    with pytest.raises(ValueError, match="come together"):
        planner.TebFleetPlanner(cfgs[0], 6, robot_cfgs=cfgs)
    with pytest.raises(ValueError, match="5 class entries for 6 robots"):
        planner.TebFleetPlanner(cfgs[0], 6, robot_cfgs=cfgs, class_of_robot=[0] * 5)
    with pytest.raises(ValueError, match="does not fit"):
        planner.TebFleetPlanner(cfgs[0], 6, robot_cfgs=cfgs, class_of_robot=[0, 1, 2, 3, 0, 0])
    other = FC.point_classes()
    other[1].optim.no_inner_iterations = 3
    with pytest.raises(ValueError, match="one per launch"):
        planner.TebFleetPlanner(cfgs[0], 6, robot_cfgs=other, class_of_robot=FC.POINTS_CLASS_OF)


def test_classes_differ_where_the_device_tests_need_them_to():
    pts, mix, sides = FC.point_classes(), FC.mixed_classes(), FC.side_classes()
    for c in pts + mix + sides:
        assert c.jacobian_mode == _abi.JACOBIAN_ANALYTIC and c.obstacles.include_dynamic_obstacles
        c.to_c()
    # EVERY condition of the kernel that reads the configuration is taken on both sides by some class
    device = open(os.path.join(ROOT, "teb_local_planner_amd", "csrc", "teb_device.hpp")).read()
    reads_c = {m.group(1) for m in re.finditer(r"#define TEB_PF_EXPR_(\w+) (.*)", device) if re.search(r"\bc\.", m.group(2))}
    assert reads_c == set(FC.SIDES), reads_c ^ set(FC.SIDES)
    for name, side in FC.SIDES.items():
        assert {bool(side(c)) for c in pts + mix + sides} == {False, True}, name
    # the sides set: what the other two leave out, and nothing else off the defaults
    assert [FC.SIDES["DYNAMIC_EDGES"](c) for c in sides] == [False, True] and [FC.SIDES["VELOCITY_EDGES"](c) for c in sides] == [True, False]
    assert all(FC.SIDES["DYNAMIC_EDGES"](c) and FC.SIDES["VELOCITY_EDGES"](c) for c in pts + mix)
    assert sorted(set(FC.SIDES_CLASS_OF)) == [0, 1] and len(FC.SIDES_CLASS_OF) == 6
    # the groups in which the classes of a set differ
    for group in ("kinematics", "velocity limits", "min_obstacle_dist", "weights", "footprint", "resize", "selection"):
        assert len({FC.GROUPS[group](c) for c in pts}) >= 2, group
    for group in ("kinematics", "velocity limits", "min_obstacle_dist", "weights", "footprint", "resize", "selection"):
        assert len({FC.GROUPS[group](c) for c in mix}) >= 2, group
    assert len({FC.GROUPS["footprint"](c) for c in mix}) == 4
    assert [c.robot_model.type for c in mix] == [_abi.FOOTPRINT_POLYGON, _abi.FOOTPRINT_LINE, _abi.FOOTPRINT_TWO_CIRCLES, _abi.FOOTPRINT_POINT]
    assert all(c.robot_model.type in (_abi.FOOTPRINT_POINT, _abi.FOOTPRINT_CIRCULAR) for c in pts)
    # the points classes as the issue words them
    d, f, o = pts
    assert FC.as_bytes(d) == FC.as_bytes(FC._base())
    assert f.robot_model.type == _abi.FOOTPRINT_CIRCULAR and f.obstacles.inflation_dist <= f.obstacles.min_obstacle_dist
    assert f.optim.obstacle_cost_exponent != 1 and f.obstacles.legacy_obstacle_association
    assert o.robot.max_vel_y != 0 and o.robot.acc_lim_y != 0 and o.optim.weight_max_vel_y != 0 and o.optim.weight_shortest_path > 0
    assert o.optim.weight_velocity_obstacle_ratio > 0 and o.trajectory.exact_arc_length
    assert mix[0].robot.min_turning_radius > 0 and mix[0].optim.weight_kinematics_turning_radius == 1
    # the maps: two scenes share a class, one class has one scene; every class is used
    for of, n in ((FC.POINTS_CLASS_OF, 3), (FC.MIXED_CLASS_OF, 4)):
        counts = np.bincount(of, minlength=n)
        assert len(of) == 6 and counts.min() >= 1 and counts.max() >= 2
    assert 1 in np.bincount(FC.MIXED_CLASS_OF)
    # the handle's own configuration differs from every class where a launch that read it would be found out
    for cfgs in (pts, mix, sides):
        h = FC.handle_config_that_differs(cfgs)
        assert all(FC.as_bytes(h) != FC.as_bytes(c) for c in cfgs)
        assert all(h.robot.max_vel_y != c.robot.max_vel_y and h.trajectory.dt_ref != c.trajectory.dt_ref for c in cfgs)


@pytest.mark.parametrize("kind", ["points", "mixed", "sides"])
def test_fixtures_hold_what_the_device_tests_rely_on(oracle, kind):
    cf = FC.CLASSED_FLEETS[kind]()
    f = cf.fleet
    assert f.n_scenes == 6 and 6 <= f.batch.count <= 30 and 16 <= f.batch.n.min() and f.batch.n.max() <= 40
    resized = set()
    for s in range(f.n_scenes):
        sub, idx = f.scene_batch(s)
        assert idx
        cfg = cf.cfg_of_scene(s)
        tol = sensitivity.band_tolerances(oracle, cfg, f.tables[s], f.vias[s], sub, threads=THREADS)
        assert all(t is not None and t <= sensitivity.WELL_CONDITIONED_TOL for t in tol), (kind, s, tol)   # no band ill-conditioned
        out, res = oracle.optimize_batch(cfg, f.tables[s], f.vias[s], sub, threads=THREADS)
        assert (res.status == _abi.TEB_OK).all(), (kind, s, res.status)
        assert out.n.max() <= 90, (kind, s, out.n)   # within the smallest pose capacity the device tests use (96)
        # the class matters: the same scene under class 0's configuration ends elsewhere
        if cf.class_of[s] != 0:
            out0, _ = oracle.optimize_batch(cf.cfgs[0], f.tables[s], f.vias[s], sub, threads=THREADS)
            assert any(out.n[k] != out0.n[k] or not np.array_equal(out.x[k], out0.x[k]) for k in range(len(idx))), (kind, s)
            if (out.n != out0.n).any():
                resized.add(cf.class_of[s])
    assert resized, "no class ends autoResize at other pose counts than class 0"
    if kind == "mixed":
        assert any(len(v) > 0 for v in f.vias) and any(len(t) == 0 for t in f.tables)
        # VIA_POINTS is (sc.nvia > 0 && c.weight_viapoint != 0): the class without the weight holds a scene WITH via-points, so that
        # the condition is false through the configuration and not through the scene alone
        assert any(len(f.vias[s]) > 0 for s in range(f.n_scenes) if cf.cfg_of_scene(s).optim.weight_viapoint == 0)


def test_growing_fixture_outgrows_the_optimistic_layout_in_one_class_only(oracle):
    cf = FC.growing_classed_fleet()
    f = cf.fleet
    assert cf.cfgs[0].trajectory.dt_ref == TebConfig().trajectory.dt_ref and len(cf.cfgs) == 2
    longest = {0: 0, 1: 0}
    for s in range(f.n_scenes):
        sub, _ = f.scene_batch(s)
        out, res = oracle.optimize_batch(cf.cfg_of_scene(s), f.tables[s], f.vias[s], sub, threads=THREADS)
        assert (res.status == _abi.TEB_OK).all()
        longest[cf.class_of[s]] = max(longest[cf.class_of[s]], int(out.n.max()))
    assert longest[1] > 238 >= longest[0] and longest[1] <= 400, longest   # blocks in LDS hold 238 poses (csrc/teb_launch_host.hpp)
