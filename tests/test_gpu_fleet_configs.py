"""Heterogeneous fleets on the MI355X (include/teb_amd.h: teb_amd_set_scene_configs): a configuration and a footprint per robot class,
the bands of all classes in ONE launch.

  * bit identity, the main contract: every band ends with the bits it has in a single-scene handle created with its CLASS's
    configuration that holds only its scene (generic_config_path = 1, multi_cu = -1, speculative_trials = -1, same layout and
    capacities, the fleet's distance path) - the points and the mixed class sets of tests/fleet_config_cases.py, the three layouts;
    the handle's own configuration differs from every class, so a launch that read it is found out; a third set, `sides`, holds the two
    sides of the kernel's conditions that those classes do not take (no obstacle weight, no velocity edges), same cases;
  * the distance path: ONE class with a polygon footprint moves the whole launch to the generic path;
  * one class equal to the handle's configuration gives the bits of the fleet without a map, and so does a permuted class order;
  * the automatic layout whose bands outgrow the optimistic choice in one class only, against the pinned run;
  * oracle parity, independent of the device's single-scene path: oracle.optimize_batch per scene with the scene's class
    configuration - counts identical, states <= 1e-7, cost and chi^2 rel 1e-7, every band checked, none skipped;
  * consumers and selection per class; state and errors; TebFleetPlanner with classes beside one handle per robot."""
import copy
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import fleet_cases  # noqa: E402
import fleet_config_cases as FC  # noqa: E402
import sensitivity  # noqa: E402

from teb_local_planner_amd import _abi, planner  # noqa: E402
from teb_local_planner_amd.config import RobotFootprintModel  # noqa: E402

pytestmark = pytest.mark.gpu

THREADS = min(os.cpu_count() or 1, 16)
LAYOUTS = {"cr": 96, "band": 300, "bandg": 400}   # layout pin -> pose capacity
LAYOUT_NO = {"band": 0, "cr": 1, "bandg": 2}
FIELDS = ("status", "lm_iterations", "lm_trials", "chi2", "cost", "lambda_")
CONTRACT = dict(generic_config_path=True, multi_cu=-1, speculative_trials=-1)


def _optimize(s, cfg):
    """(the iteration counts and the cost scales are arguments of the launch: the classes of the fixtures agree on them)"""
    s.optimize(cfg.optim.no_inner_iterations, cfg.optim.no_outer_iterations, True, cfg.hcp.selection_obst_cost_scale,
               cfg.hcp.selection_viapoint_cost_scale, cfg.hcp.selection_alternative_time_cost)


def _fleet_solver(cf, layout="auto", handle_cfg=None, with_map=True, **opts):
    f = cf.fleet
    mo, mv, mw = f.capacities()
    s = planner.TebBatchSolver(handle_cfg or FC.handle_config_that_differs(cf.cfgs), f.batch.count, f.batch.stride, mo, mv, mw,
                               options=_abi.Options(layout=layout, **opts))
    s.set_scenes(f.tables, f.vias)
    if with_map:
        s.set_scene_configs(cf.cfgs, cf.class_of)
    s.set_band_scenes(f.scene_of)
    s.upload(f.batch)
    return s


def _finish(s, f, commands=False):
    res, out, inst = s.results(), s.download(f.batch.copy()), s.last_instantiation()
    assert not s.debug_overflow_flags().any()
    cmd = s.velocity_commands(list(range(f.batch.count)), 2, 1) if commands else None
    s.close()
    return out, res, inst, cmd


def _run_fleet(cf, layout="auto", commands=False, **kw):
    s = _fleet_solver(cf, layout, **kw)
    _optimize(s, cf.cfgs[0])
    return _finish(s, cf.fleet, commands)


def _run_single_scenes(cf, layout, generic_distance_path, commands=False):
    """One single-scene handle per scene, created with the configuration of the scene's class: [(band indices, out, res, inst, cmd)]"""
    f = cf.fleet
    mo, mv, mw = f.capacities()
    runs = []
    for sc in range(f.n_scenes):
        sub, idx = f.scene_batch(sc)
        assert idx
        cfg = cf.cfg_of_scene(sc)
        s = planner.TebBatchSolver(cfg, f.batch.count, f.batch.stride, mo, mv, mw,
                                   options=_abi.Options(layout=layout, generic_distance_path=generic_distance_path, **CONTRACT))
        s.set_obstacles(f.tables[sc])
        s.set_via_points(f.vias[sc])
        s.upload(sub)
        _optimize(s, cfg)
        res, out, inst = s.results(), s.download(sub.copy()), s.last_instantiation()
        cmd = s.velocity_commands(list(range(len(idx))), 2, 1) if commands else None
        runs.append((idx, out, res, inst, cmd))
        s.close()
    return runs


def _assert_bands_equal(out, res, b, out1, res1, k, label):
    assert int(out.n[b]) == int(out1.n[k]), (label, b, out.n[b], out1.n[k])
    for name, u, v in zip(("x", "y", "theta", "dt"), out.get_teb(b), out1.get_teb(k)):
        np.testing.assert_array_equal(u, v, err_msg="%s: band %d, %s" % (label, b, name))
    for fld in FIELDS:
        np.testing.assert_array_equal(getattr(res, fld)[b], getattr(res1, fld)[k], err_msg="%s: band %d, %s" % (label, b, fld))


def _assert_same_run(a, b, label):
    (out, res), (out1, res1) = a, b
    assert out.count == out1.count
    for k in range(out.count):
        _assert_bands_equal(out, res, k, out1, res1, k, label)


def _assert_fleet_equals_singles(cf, fleet_run, singles, want, label, commands=False):
    out, res, inst, cmd = fleet_run
    assert tuple(inst) == want, (inst, want)
    seen = 0
    for idx, out1, res1, inst1, cmd1 in singles:
        assert tuple(inst1) == want, (inst1, want)   # the single-scene handle ran the same (non-folded) kind
        for k, b in enumerate(idx):
            _assert_bands_equal(out, res, b, out1, res1, k, label)
            if commands:
                assert bool(cmd[0][b]) == bool(cmd1[0][k]) and cmd[0][b], (label, b)
                np.testing.assert_array_equal(cmd[1][b], cmd1[1][k], err_msg="%s: velocity command of band %d" % (label, b))
            seen += 1
    assert seen == cf.fleet.batch.count   # every band is compared, none skipped
    assert (res.status == _abi.TEB_OK).all()


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
@pytest.mark.parametrize("kind", ["points", "mixed", "sides"])
def test_bands_equal_the_single_scene_handle_of_their_class_bit_for_bit(kind, layout):
    stride = LAYOUTS[layout]
    cf = FC.CLASSED_FLEETS[kind](stride)
    assert cf.fleet.n_scenes == 6 and 6 <= cf.fleet.batch.count <= 30
    want = (LAYOUT_NO[layout], 0, 1 if kind == "mixed" else 0)
    commands = layout == "cr"   # the consumers once per class set: every band's command against its single-scene handle's
    fleet_run = _run_fleet(cf, layout, commands)
    singles = _run_single_scenes(cf, layout, generic_distance_path=(kind == "mixed"), commands=commands)
    _assert_fleet_equals_singles(cf, fleet_run, singles, want, "%s/%s" % (kind, layout), commands)
    if commands and kind == "points":
        # the holonomic class: vy != 0 somewhere - with the handle's max_vel_y of another class's band the command differs
        out, res, inst, cmd = fleet_run
        holo = [b for b in range(cf.fleet.batch.count) if cf.cfg_of_band(b).robot.max_vel_y != 0]
        rest = [b for b in range(cf.fleet.batch.count) if cf.cfg_of_band(b).robot.max_vel_y == 0]
        assert holo and rest and (cmd[1][holo, 1] != 0).any() and (cmd[1][rest, 1] == 0).all()
    # the classes matter: the same fleet without the map, under class 0 alone, ends elsewhere
    if layout == "cr":
        out, res = fleet_run[0], fleet_run[1]
        out0, res0, _, _ = _run_fleet(cf, layout, handle_cfg=cf.cfgs[0], with_map=False)
        others = [b for b in range(cf.fleet.batch.count) if cf.class_of[int(cf.fleet.scene_of[b])] != 0]
        assert any(out.n[b] != out0.n[b] or res.chi2[b] != res0.chi2[b] for b in others)


def test_one_polygon_class_moves_the_whole_launch_to_the_generic_path():
    cf = FC.classed_point_fleet(LAYOUTS["cr"], polygon_class=1)
    fleet_run = _run_fleet(cf, "cr")
    # the bands of the point-footprint classes equal their handles with generic_distance_path = 1; so do the polygon class's
    singles = _run_single_scenes(cf, "cr", generic_distance_path=True)
    _assert_fleet_equals_singles(cf, fleet_run, singles, (1, 0, 1), "points fleet with one polygon class")
    # ... and the point-like launch of the same fleet without the polygon is another kind
    assert tuple(_run_fleet(FC.classed_point_fleet(LAYOUTS["cr"]), "cr")[2]) == (1, 0, 0)


@pytest.mark.parametrize("kind", ["points", "mixed"])
def test_one_class_equal_to_the_handles_configuration_changes_nothing(kind):
    cf = FC.classed_point_fleet() if kind == "points" else FC.classed_mixed_fleet()
    f = cf.fleet
    cfg = cf.cfgs[1]   # (off the defaults)
    plain = _run_fleet(cf, "cr", handle_cfg=cfg, with_map=False)
    one = FC.ClassedFleet(f, [cfg], [0] * f.n_scenes)
    mapped = _run_fleet(one, "cr", handle_cfg=cfg)
    _assert_same_run(mapped[:2], plain[:2], "one class equal to the handle's configuration")
    assert tuple(mapped[2]) == tuple(plain[2])
    # the same map with the class order permuted
    a = _run_fleet(cf, "cr")
    perm = list(range(len(cf.cfgs)))[::-1]
    shuffled = FC.ClassedFleet(f, [cf.cfgs[k] for k in perm], [perm.index(k) for k in cf.class_of])
    b = _run_fleet(shuffled, "cr")
    _assert_same_run(a[:2], b[:2], "class order permuted")


def test_automatic_layout_repeat_equals_the_pinned_run():
    cf = FC.growing_classed_fleet()
    out_p, res_p, inst_p, _ = _run_fleet(cf, "bandg")
    out_a, res_a, inst_a, _ = _run_fleet(cf, "auto")
    grown = {k: max(int(out_p.n[b]) for b in range(out_p.count) if cf.class_of[int(cf.fleet.scene_of[b])] == k) for k in (0, 1)}
    print("longest band per class after autoResize:", grown, "instantiations (pinned, automatic):", inst_p, inst_a)
    assert grown[1] > 238 >= grown[0], "only class 1's bands were to outgrow the blocks-in-LDS layout"
    assert tuple(inst_p) == (2, 0, 0) and tuple(inst_a) == (2, 0, 0), (inst_p, inst_a)   # the repeat ran in the handle's own layout
    assert (res_p.status == _abi.TEB_OK).all()
    _assert_same_run((out_a, res_a), (out_p, res_p), "automatic layout against the pinned one")


@pytest.mark.parametrize("kind", ["points", "mixed", "sides"])
def test_oracle_parity_per_scene_with_the_class_configuration(oracle, kind):
    cf = FC.CLASSED_FLEETS[kind]()
    f = cf.fleet
    out, res, _, _ = _run_fleet(cf)
    worst = {"state": 0.0, "cost": 0.0}
    total = 0
    for sc in range(f.n_scenes):
        sub, idx = f.scene_batch(sc)
        ref, rres = oracle.optimize_batch(cf.cfg_of_scene(sc), f.tables[sc], f.vias[sc], sub, threads=THREADS)
        dev = _abi.TebBatchHost(len(idx), f.batch.stride)
        dres = _abi.ResultsHost(len(idx))
        for k, b in enumerate(idx):
            for fld in ("n", "x", "y", "theta", "dt"):
                getattr(dev, fld)[k] = getattr(out, fld)[b]
            for fld in FIELDS:
                getattr(dres, fld)[k] = getattr(res, fld)[b]
        rep = sensitivity.compare_bands(dev, dres, ref, rres, None)
        print("%s scene %d class %d:" % (kind, sc, cf.class_of[sc]), rep)
        assert rep["status_equal"] == rep["bands"] and rep["counts_equal"] == rep["bands"], (kind, sc, rep)
        assert rep["checked"] == rep["bands"] == len(idx) and rep["skipped"] == 0, (kind, sc, rep)
        assert rep["max_state_err"] <= 1e-7 and rep["max_cost_rel"] <= 1e-7, (kind, sc, rep)
        np.testing.assert_allclose(dres.chi2, rres.chi2, rtol=1e-7)
        worst["state"] = max(worst["state"], rep["max_state_err"]); worst["cost"] = max(worst["cost"], rep["max_cost_rel"])
        total += rep["checked"]
    print("%s: %d bands against the oracle, max state err %.2e, max cost rel %.2e" % (kind, total, worst["state"], worst["cost"]))
    assert total == f.batch.count


def test_select_best_per_scene_takes_the_scenes_class(oracle):
    cf = FC.classed_point_fleet()
    f = cf.fleet
    ns = f.n_scenes
    cfgs = copy.deepcopy(cf.cfgs)
    for c, (hyst, prefer) in zip(cfgs, ((1.0, 0.95), (0.4, 1.0), (1.0, 0.3))):   # strong enough to change winners, another way in every class
        c.hcp.selection_cost_hysteresis, c.hcp.selection_prefer_initial_plan = hyst, prefer
    cf = FC.ClassedFleet(f, cfgs, cf.class_of)
    handle_cfg = FC.handle_config_that_differs(cfgs)   # hysteresis 1, preference 1: never changes a winner
    s = _fleet_solver(cf, handle_cfg=handle_cfg)
    _optimize(s, cfgs[0])
    cost = s.results().cost.copy()

    def want(cfg_of, last, init):
        best = np.full(ns, -1, np.int32)
        for sc in range(ns):
            idx = f.bands_of(sc)
            loc = lambda b: idx.index(b) if b in idx else -1
            k, _ = oracle.select_best(cfg_of(sc), cost[idx], last_best=loc(last[sc]), initial_plan=loc(init[sc]))
            best[sc] = idx[k]
        return best

    multi = [sc for sc in range(ns) if len(f.bands_of(sc)) >= 2]
    assert {cf.class_of[sc] for sc in multi} >= {1, 2}
    worst = [f.bands_of(sc)[int(np.argmax(cost[f.bands_of(sc)]))] for sc in range(ns)]   # the most expensive band of every scene
    none = [-1] * ns
    differs = 0
    for last, init in ((none, none), (worst, none), (none, worst), (worst, worst)):
        best, bcost = s.select_best_per_scene(None if last is none else last, None if init is none else init)
        w = want(cf.cfg_of_scene, last, init)
        np.testing.assert_array_equal(best, w)
        differs += int((w != want(lambda sc: handle_cfg, last, init)).any())
        for sc in range(ns):
            c = cf.cfg_of_scene(sc).hcp
            scale = c.selection_cost_hysteresis if best[sc] == last[sc] else (c.selection_prefer_initial_plan if best[sc] == init[sc] else 1.0)
            assert bcost[sc] == cost[best[sc]] * scale
    assert differs >= 2, "the handle's values would have chosen the same bands: the case checks nothing"
    # without the map the handle's values are back
    s.clear_scene_configs()
    best, _ = s.select_best_per_scene(worst, worst)
    np.testing.assert_array_equal(best, want(lambda sc: handle_cfg, worst, worst))
    s.close()


def test_state_and_errors():
    cf = FC.classed_point_fleet()
    f = cf.fleet
    handle_cfg = FC.handle_config_that_differs(cf.cfgs)
    mo, mv, mw = f.capacities()
    s = planner.TebBatchSolver(handle_cfg, f.batch.count + 30, f.batch.stride, mo, mv, mw, options=_abi.Options(layout="cr"))

    def run():
        s.set_band_scenes(f.scene_of)
        s.upload(f.batch)
        _optimize(s, cf.cfgs[0])
        return s.download(f.batch.copy()), s.results()

    def refused(call, what, code=_abi.ERR_INVALID_ARG):
        with pytest.raises(planner.TebAmdError) as e:
            call()
        assert e.value.code == code and what in str(e.value), str(e.value)

    def raw(cfgs, of):   # past the wrapper's own checks, into the library
        packed = _abi.pack_scene_configs(cfgs, [0] * len(of))
        planner._chk(planner.lib().teb_amd_set_scene_configs(s._h, len(cfgs), packed.configs, len(of), _abi._ptr(_abi.i32(of), planner.C.c_int32)),
                     "teb_amd_set_scene_configs")
    # not in fleet mode
    refused(lambda: raw(cf.cfgs, cf.class_of), "no scenes set")
    assert s.scene_configs()[0] == 0
    s.set_scenes(f.tables, f.vias)
    no_map = run()
    s.set_scene_configs(cf.cfgs, cf.class_of)
    n_classes, of = s.scene_configs()
    assert n_classes == 3 and of.tolist() == cf.class_of
    with_map = run()
    assert any(with_map[1].chi2[b] != no_map[1].chi2[b] for b in range(f.batch.count))
    # every refusal leaves the map installed and the handle as it was
    bad_fp = copy.deepcopy(cf.cfgs); bad_fp[2].robot_model = RobotFootprintModel(_abi.FOOTPRINT_LINE, vertices=[(0.0, 0.0)])
    static = copy.deepcopy(cf.cfgs); static[1].obstacles.include_dynamic_obstacles = False
    numeric = copy.deepcopy(cf.cfgs); numeric[2].jacobian_mode = _abi.JACOBIAN_G2O_NUMERIC
    out_of_range = list(cf.class_of); out_of_range[4] = 3
    for call, what in ((lambda: raw(cf.cfgs, cf.class_of[:-1]), "6 scenes are set"),
                       (lambda: raw(cf.cfgs, cf.class_of + [0]), "6 scenes are set"),
                       (lambda: raw(cf.cfgs, out_of_range), "class_of_scene[4] = 3"),
                       (lambda: raw(bad_fp, cf.class_of), "class 2: line footprint"),
                       (lambda: raw(static, cf.class_of), "class 1: include_dynamic_obstacles"),
                       (lambda: raw(numeric, cf.class_of), "class 2: jacobian_mode")):
        refused(call, what)
        assert s.scene_configs()[0] == 3
        _assert_same_run(run(), with_map, "after a refused class map: " + what)
    # teb_amd_set_config changes the handle's configuration and leaves the map alone
    s.set_config(cf.cfgs[2])
    _assert_same_run(run(), with_map, "after set_config under a map")
    s.set_config(handle_cfg)
    # the map survives set_scenes with the same count and derives the new tables' lists per class: against the single-scene handles
    order = [4, 3, 5, 1, 0, 2]   # the scenes of every class exchange their tables and bands: new tables everywhere, each under the class the fixture gave it
    g = fleet_cases.Fleet(f.cfg, [f.tables[k] for k in order], [f.vias[k] for k in order], f.batch, [order.index(int(x)) for x in f.scene_of])
    s.set_scenes(g.tables, g.vias)
    assert s.scene_configs()[0] == 3 and s.scene_configs()[1].tolist() == cf.class_of
    s.set_band_scenes(g.scene_of); s.upload(g.batch); _optimize(s, cf.cfgs[0])
    moved = FC.ClassedFleet(g, cf.cfgs, cf.class_of)
    singles = _run_single_scenes(moved, "cr", generic_distance_path=False)
    _assert_fleet_equals_singles(moved, (s.download(g.batch.copy()), s.results(), s.last_instantiation(), None), singles, (1, 0, 0), "map kept over set_scenes")
    # explore_candidates_per_scene: refused with two classes, runs with one
    starts = [(x, y, 0.0) for x, y in f.origins]; goals = [(x + 3.0, y, 0.0) for x, y in f.origins]
    refused(lambda: s.explore_candidates_per_scene(starts, goals), "more than one class", _abi.ERR_UNSUPPORTED)
    assert s.scene_configs()[0] == 3
    s.set_scene_configs([cf.cfgs[1]], [0] * 6)
    got = s.explore_candidates_per_scene(starts, goals, max_paths=40)
    assert got["n_total"] >= f.batch.count and s.scene_configs()[0] == 1
    # forgotten by a set of another size and by clear_scenes
    s.set_scenes(f.tables[:5], f.vias[:5])
    assert s.scene_configs()[0] == 0
    s.set_scenes(f.tables, f.vias)
    assert s.scene_configs()[0] == 0
    _assert_same_run(run(), no_map, "after the map was forgotten by a set of another size")
    s.set_scene_configs(cf.cfgs, cf.class_of)
    s.clear_scenes()
    assert s.scene_configs()[0] == 0 and s.scene_count() == 0
    s.set_scenes(f.tables, f.vias)
    _assert_same_run(run(), no_map, "after clear_scenes")
    s.set_scene_configs(cf.cfgs, cf.class_of)
    s.clear_scene_configs()
    s.clear_scene_configs()   # (no map: no effect)
    _assert_same_run(run(), no_map, "after clear_scene_configs")
    s.close()


def test_divergence_rule_takes_the_bands_class():
    """teb_amd_has_diverged and teb_amd_get_batch_statistics: divergence_detection_* of the band's class"""
    cf = FC.classed_point_fleet()
    f = cf.fleet
    cfgs = copy.deepcopy(cf.cfgs)
    cfgs[1].recovery.divergence_detection_max_chi_squared = 1e-12   # every band of class 1 counts as diverged
    cf = FC.ClassedFleet(f, cfgs, cf.class_of)
    s = _fleet_solver(cf)
    _optimize(s, cfgs[0])
    available, back = s.batch_statistics()
    for b in range(f.batch.count):
        enabled = cf.cfg_of_band(b).recovery.divergence_detection_enable
        assert bool(available[b]) == bool(enabled), b
        assert bool(s.has_diverged(b)) == bool(enabled and back[b] > 1e-12), b
    assert any(s.has_diverged(b) for b in range(f.batch.count))
    s.close()


def test_commands_follow_a_new_band_scene_map():
    """With a class map a band's command depends on the band -> scene map (max_vel_y and dt_ref of the scene's class): a new map must
    not be answered from the commands cached under the old one, at the same look-ahead."""
    cf = FC.classed_point_fleet()
    f = cf.fleet
    s = _fleet_solver(cf)
    _optimize(s, cf.cfgs[0])
    bands = list(range(f.batch.count))
    before = s.velocity_commands(bands, 2, 1)
    moved = [(int(sc) + 1) % f.n_scenes for sc in f.scene_of]   # every band to a scene of another class
    assert all(cf.class_of[a] != cf.class_of[int(b)] for a, b in zip(moved, f.scene_of))
    s.set_band_scenes(moved)
    after = s.velocity_commands(bands, 2, 1)     # the same look-ahead: the cached commands, if the map did not void them
    s.velocity_commands(bands, 3, 1)             # another look-ahead: computed anew
    again = s.velocity_commands(bands, 2, 1)     # ... and so is this one
    np.testing.assert_array_equal(after[0], again[0])
    np.testing.assert_array_equal(after[1], again[1])
    was_holo = [b for b in bands if cf.cfg_of_band(b).robot.max_vel_y != 0]
    assert (before[1][was_holo, 1] != 0).any() and (again[1][was_holo, 1] == 0).all()   # their new classes have no vy
    s.close()


def test_fleet_planner_with_classes_beside_one_handle_per_robot():
    cfgs = FC.point_classes()
    for c, (la, prevent) in zip(cfgs, ((1, 0), (3, 1), (2, 0))):   # each class its own look-ahead
        c.trajectory.control_look_ahead_poses, c.trajectory.prevent_look_ahead_poses_near_goal = la, prevent
    cfgs[1].trajectory.min_samples, cfgs[2].trajectory.force_reinit_new_goal_dist = 5, 0.5
    cfgs[2].trajectory.max_samples = 200
    R, ticks = 6, 3
    class_of = FC.POINTS_CLASS_OF
    rng = np.random.default_rng(207)
    origin = rng.uniform(-20, 20, (R, 2))
    tables = []
    for r in range(R):
        t = _abi.ObstacleTable()
        for _ in range(int(rng.integers(5, 30))):
            t.add_point(origin[r, 0] + rng.uniform(0.5, 5.5), origin[r, 1] + rng.uniform(-1.5, 1.5))
        t.add_point(origin[r, 0] + 3.0, origin[r, 1] + 0.4, vel=(0.0, -0.1))
        tables.append(t)
    fleet = planner.TebFleetPlanner(FC.handle_config_that_differs(cfgs), R, max_obstacles=sum(len(t) for t in tables), robot_cfgs=cfgs, class_of_robot=class_of)
    assert fleet.max_poses == 501   # the largest max_samples of the classes + 1
    fleet = planner.TebFleetPlanner(FC.handle_config_that_differs(cfgs), R, max_poses=128, max_obstacles=sum(len(t) for t in tables), robot_cfgs=cfgs,
                                    class_of_robot=class_of)
    singles = []
    for r in range(R):
        p = planner.TebOptimalPlanner(cfgs[class_of[r]], tables[r], [], max_poses=128)
        p._solver = planner.TebBatchSolver(p.cfg_, 1, 128, max(len(tables[r]), 1), 1, 1, options=_abi.Options(**CONTRACT))   # the contract's options
        p._resident = False
        singles.append(p)
    goal_shift = rng.uniform(-0.3, 0.3, (R, 2))
    prev = None
    for tick in range(ticks):
        starts = [(origin[r, 0] + 0.25 * tick, origin[r, 1] + 0.02 * tick * (r % 3 - 1), 0.01 * tick) for r in range(R)]
        # robots 2 and 5 (the class with force_reinit_new_goal_dist = 0.5) get a goal 0.7 m away at tick 2: they initialise again, a robot
        # of another class with the same shift (robot 1) warm starts
        far = lambda r: 0.7 if (r in (1, 2, 5) and tick == 2) else 0.0
        goals = [(origin[r, 0] + 6.0 + goal_shift[r, 0] + far(r), origin[r, 1] + goal_shift[r, 1], 0.1 * (r % 3 - 1)) for r in range(R)]
        ok = fleet.plan(starts, goals, prev, tables, [[] for _ in range(R)])
        assert fleet.solver.scene_configs()[0] == 3
        cmds = fleet.getVelocityCommands()
        counts = fleet.pose_counts()
        for r in range(R):
            ok1 = singles[r].plan(starts[r], goals[r], None if prev is None else prev[r])
            c1 = singles[r].getVelocityCommand()
            assert bool(ok[r]) == bool(ok1), (tick, r)
            assert int(counts[r]) == int(singles[r].teb().n[0]), (tick, r, counts[r], singles[r].teb().n[0])
            assert cmds[r] == c1, (tick, r, cmds[r], c1)
            for u, v in zip(fleet.teb().get_teb(r), singles[r].teb().get_teb(0)):
                np.testing.assert_array_equal(u, v)
        prev = [c[1:] for c in cmds]
