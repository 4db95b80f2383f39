"""The whole tick of a heterogeneous fleet on the MI355X (include/teb_amd.h: the _per_class calls) - every robot under the
configuration of its class from updateAllTEBs to the saturated command.

  * exploration: every scene's bands, flags, counts, graph and initial_plan_teb bit for bit those of a single-scene handle created with
    the configuration of the scene's class that ran teb_amd_explore_candidates with dist_to_obst = its min_obstacle_dist - both graphs,
    2-D and 3-D signatures, given samples and the scene's own generator; every scene against the CPU oracle under its class; the result
    does not depend on the round quota; one class equal to the handle's configuration gives the bits of the per-scene call;
  * costs: teb_amd_optimize_batch_per_class leaves the bands teb_amd_optimize_batch leaves, in the three layouts, the cost of every band
    has the bits of its class's single-scene handle launched with its class's triple, and the selection picks what those handles pick;
  * pruning and feasibility per class against the single calls, and every refusal with the handle left as it was;
  * FleetHomotopyClassPlanner with classes, tick after tick, beside one HomotopyClassPlanner per robot created with the robot's class.

The handle's own configuration equals no class. The fixtures (tests/fleet_class_tick_cases.py) are shown to discriminate on the CPU in
tests/test_fleet_class_tick_cases.py."""
import copy
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.path.insert(0, HERE)
import feasibility_cases  # noqa: E402
import fleet_class_tick_cases as CT  # noqa: E402
import fleet_config_cases as FC  # noqa: E402
import fleet_explore_cases as FE  # noqa: E402
import fleet_tick_cases as FT  # noqa: E402
import plan_window_cases as PW  # noqa: E402
from test_gpu_fleet_explore import _state, _compare_all, _renew_fleet, _renew_single, MAX_TEBS, TOL  # noqa: E402
from test_gpu_fleet_configs import LAYOUTS, LAYOUT_NO  # noqa: E402
from test_gpu_fleet_tick import _tick_costmap  # noqa: E402

from teb_local_planner_amd import _abi, planner  # noqa: E402
from teb_local_planner_amd.config import TebConfig  # noqa: E402

pytestmark = pytest.mark.gpu

SINGLE = dict(generic_config_path=True, multi_cu=-1, speculative_trials=-1)   # the fleet contract of include/teb_amd.h


def _same(u, v, what=""):
    u = np.ascontiguousarray(np.asarray(u, np.float64)).view(np.uint64)
    v = np.ascontiguousarray(np.asarray(v, np.float64)).view(np.uint64)
    assert u.shape == v.shape and np.array_equal(u, v), what


# ---- exploration -------------------------------------------------------------------------------------------------------------------
def _explore_fixture(graph, dynamic):
    f = FE.explore_fleet("points", dynamic, keypoint=(graph == "keypoint"), plans_in_class=2, viapoints_all_candidates=False)
    return f, CT.explore_classes(f.cfg)


def _fleet_explorer(f, cfgs, class_of=CT.EXPLORE_CLASS_OF, handle_cfg=None):
    mo, mv, mw = f.capacities()
    s = planner.TebBatchSolver(handle_cfg or CT.explore_handle_config(cfgs), MAX_TEBS, f.batch.stride, mo, mv, mw, options=_abi.Options(**SINGLE))
    s.set_scenes(f.tables, f.vias)
    if cfgs is not None:
        s.set_scene_configs(cfgs, class_of)
    s.set_band_scenes(f.scene_of)
    s.upload(f.batch)
    s.set_optimized_flags([1] * f.batch.count)
    return s


def _single_explorer(f, cfg, sc):
    mo, mv, mw = f.capacities()
    s = planner.TebBatchSolver(cfg, MAX_TEBS, f.batch.stride, mo, mv, mw, options=_abi.Options(**SINGLE))
    s.set_obstacles(f.tables[sc])
    s.set_via_points(f.vias[sc])
    sub, idx = f.scene_batch(sc)
    if idx:
        s.upload(sub)
        s.set_optimized_flags([1] * len(idx))
    return s


def _explore_single(s, f, cfg, sc, best, us=None):
    return s.explore_candidates(f.starts[sc], f.goals[sc], cfg.obstacles.min_obstacle_dist, None, False, best, None if us is None else us[sc],
                                f.max_paths, initial_plan=f.plans[sc])


def _explore_class(s, f, best, us=None):
    return s.explore_candidates_per_class(f.starts, f.goals, None, False, best, us, f.max_paths, params=f.cfg.hcp_params(), initial_plans=f.plans)


@pytest.mark.parametrize("dynamic", [True, False])
@pytest.mark.parametrize("graph", ["keypoint", "roadmap"])
def test_every_scene_explores_under_its_class_bit_for_bit_and_against_the_oracle(oracle, graph, dynamic):
    f, cfgs = _explore_fixture(graph, dynamic)
    us = FE.unit_samples(f)
    sf = _fleet_explorer(f, cfgs)
    before = sf.count
    r = _explore_class(sf, f, _renew_fleet(sf, f), us)
    assert r["n_total"] > before
    singles, results = [], []
    for sc in range(f.n_scenes):
        cfg = cfgs[CT.EXPLORE_CLASS_OF[sc]]
        s1 = _single_explorer(f, cfg, sc)
        results.append(_explore_single(s1, f, cfg, sc, _renew_single(s1, f, sc), us))
        singles.append(s1)
    _compare_all(sf, f, r, singles, results)
    # ... and against the CPU oracle under the scene's class, independent of the device's single-scene path
    scene_of = sf.band_scenes()
    fb, fve, _, _ = _state(sf, f.batch.stride)
    for sc in range(f.n_scenes):
        n_tebs, o = CT.explore_on_host(oracle, f, cfgs[CT.EXPLORE_CLASS_OF[sc]], sc, us)
        mine = np.nonzero(scene_of == sc)[0]
        assert r["n_bands"][sc] == o["n_total"] == len(mine), sc
        assert r["initial_plan_teb"][sc] == o["initial_plan_teb"] and r["n_vertices"][sc] == len(o["vertices"]), sc
        V, A = sf.exploration_graph_per_scene(sc)
        if len(o["vertices"]):
            assert np.abs(V - o["vertices"]).max() <= TOL
            want = np.zeros_like(A)
            for i, row in enumerate(o["adjacency"]):
                want[i, row] = 1
            np.testing.assert_array_equal(A, want, err_msg="graph of scene %d" % sc)
        for k, bnd in enumerate(mine):
            for u, v in zip(fb.get_teb(int(bnd)), o["batch"].get_teb(k)):
                assert len(u) == len(v) and np.abs(u - v).max(initial=0) <= TOL, (sc, k)
        if f.vias[sc]:
            np.testing.assert_array_equal(fve[mine], o["via_enabled"][:o["n_total"]], err_msg="via-point flags of scene %d" % sc)
    for s1 in singles:
        s1.close()
    sf.close()


def test_every_scene_draws_from_its_own_generator_under_its_class():
    f, cfgs = _explore_fixture("roadmap", True)
    sf = _fleet_explorer(f, cfgs)
    new_best = _renew_fleet(sf, f)
    singles = [_single_explorer(f, cfgs[CT.EXPLORE_CLASS_OF[sc]], sc) for sc in range(f.n_scenes)]
    bests = [_renew_single(s1, f, sc) for sc, s1 in enumerate(singles)]
    r = _explore_class(sf, f, new_best)
    results = [_explore_single(s1, f, cfgs[CT.EXPLORE_CLASS_OF[sc]], sc, bests[sc]) for sc, s1 in enumerate(singles)]
    _compare_all(sf, f, r, singles, results)
    for s1 in singles:
        s1.close()
    sf.close()


def test_exploration_per_class_does_not_depend_on_the_paths_per_round():
    f, cfgs = _explore_fixture("roadmap", True)
    us = FE.unit_samples(f)
    seen = {}
    for q in (0, 1, 64):
        sf = _fleet_explorer(f, cfgs)
        sf.debug_set_explore_quota(q)
        r = _explore_class(sf, f, _renew_fleet(sf, f), us)
        scene_of = sf.band_scenes()
        fb, fve, fvs, fvg = _state(sf, f.batch.stride)
        per_scene = []
        for sc in range(f.n_scenes):
            mine = np.nonzero(scene_of == sc)[0]
            per_scene.append(([fb.get_teb(int(b)) for b in mine], fve[mine], fvs[mine], fvg[mine], sf.exploration_graph_per_scene(sc)))
        seen[q] = (r, per_scene)
        sf.close()
    r0, p0 = seen[0]
    for q in (1, 64):
        r, p = seen[q]
        for key in ("n_total", "n_bands", "n_vertices", "n_paths", "initial_plan_teb"):
            np.testing.assert_array_equal(r[key], r0[key], err_msg="%s with %d paths per round" % (key, q))
        for sc in range(f.n_scenes):
            assert len(p[sc][0]) == len(p0[sc][0])
            for u, v in zip(p[sc][0], p0[sc][0]):
                for a, b in zip(u, v):
                    np.testing.assert_array_equal(a, b)
            for k in (1, 2, 3):
                np.testing.assert_array_equal(p[sc][k], p0[sc][k])
            np.testing.assert_array_equal(p[sc][4][0], p0[sc][4][0])
            np.testing.assert_array_equal(p[sc][4][1], p0[sc][4][1])


def test_one_class_equal_to_the_handle_gives_the_bits_of_the_per_scene_call():
    f, cfgs = _explore_fixture("keypoint", True)
    us = FE.unit_samples(f)
    cfg = cfgs[1]
    runs = []
    for mode in ("per_class with a map of one class", "per_class without a map", "per_scene"):
        sf = _fleet_explorer(f, [cfg] if mode.endswith("one class") else None, [0] * f.n_scenes, handle_cfg=cfg)
        best = _renew_fleet(sf, f)
        if mode == "per_scene":
            r = sf.explore_candidates_per_scene(f.starts, f.goals, cfg.obstacles.min_obstacle_dist, None, False, best, us, f.max_paths,
                                                initial_plans=f.plans)
        else:
            r = _explore_class(sf, f, best, us)
        runs.append((r, _state(sf, f.batch.stride), sf.band_scenes(), [sf.exploration_graph_per_scene(sc) for sc in range(f.n_scenes)]))
        sf.close()
    r0, st0, so0, g0 = runs[2]
    assert r0["n_total"] > f.batch.count
    for (r, st, so, g), mode in zip(runs[:2], ("map of one class", "no map")):
        for key in ("n_total", "n_bands", "n_vertices", "n_paths", "initial_plan_teb"):
            np.testing.assert_array_equal(r[key], r0[key], err_msg=mode)
        np.testing.assert_array_equal(so, so0)
        for k in range(r0["n_total"]):
            for u, v in zip(st[0].get_teb(k), st0[0].get_teb(k)):
                np.testing.assert_array_equal(u, v, err_msg="%s: band %d" % (mode, k))
        for a, b in zip(st[1:], st0[1:]):
            np.testing.assert_array_equal(a, b, err_msg=mode)
        for (V, A), (V0, A0) in zip(g, g0):
            np.testing.assert_array_equal(V, V0); np.testing.assert_array_equal(A, A0)


def test_exploration_refusals():
    f, cfgs = _explore_fixture("keypoint", True)
    L = planner.lib()
    p = f.cfg.hcp_params()
    D = lambda a: _abi._ptr(np.ascontiguousarray(a, np.float64), C.c_double)
    one = _single_explorer(f, cfgs[0], FE.BEST)
    nt = C.c_int32(0)
    rc = L.teb_amd_explore_candidates_per_class(one._h, C.byref(p), D(f.starts), D(f.goals), None, 0, None, None, 0, C.byref(nt), None, None, None, None,
                                                None, None, None, None)
    assert rc == _abi.ERR_INVALID_ARG and b"teb_amd_set_scenes" in L.teb_amd_last_error()
    one.close()
    sf = _fleet_explorer(f, cfgs)
    with pytest.raises(planner.TebAmdError) as e:   # the per-scene call keeps refusing more than one class
        sf.explore_candidates_per_scene(f.starts, f.goals, 0.2, None, False, f.best, None, f.max_paths, initial_plans=f.plans)
    assert e.value.code == _abi.ERR_UNSUPPORTED
    wrong = f.best.copy(); wrong[FE.FULL] = f.bands_of(FE.BEST)[0]
    with pytest.raises(planner.TebAmdError) as e:
        _explore_class(sf, f, wrong)
    assert e.value.code == _abi.ERR_INVALID_ARG and "teb_amd_explore_candidates_per_class" in str(e.value) and "not a band of scene" in str(e.value)
    assert sf.count == f.batch.count
    np.testing.assert_array_equal(sf.band_scenes(), f.scene_of)
    sf.close()


# ---- costs -------------------------------------------------------------------------------------------------------------------------
RESULT_FIELDS = ("status", "lm_iterations", "lm_trials", "chi2", "lambda_")


def _cost_solver(cf, layout):
    f = cf.fleet
    mo, mv, mw = f.capacities()
    s = planner.TebBatchSolver(FC.handle_config_that_differs(cf.cfgs), f.batch.count, f.batch.stride, mo, mv, mw, options=_abi.Options(layout=layout))
    s.set_scenes(f.tables, f.vias)
    s.set_scene_configs(cf.cfgs, cf.class_of)
    s.set_band_scenes(f.scene_of)
    s.upload(f.batch)
    return s


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_costs_take_the_triple_of_the_bands_class(layout):
    cf = CT.cost_classed_fleet(LAYOUTS[layout])
    f = cf.fleet
    o = cf.cfgs[0].optim
    plain = _cost_solver(cf, layout)
    plain.optimize(o.no_inner_iterations, o.no_outer_iterations, True, 1.7, 0.6, True)   # any triple
    want_out, want_res = plain.download(f.batch.copy()), plain.results()
    plain.close()
    s = _cost_solver(cf, layout)
    s.optimize_per_class(o.no_inner_iterations, o.no_outer_iterations, True)
    out, res = s.download(f.batch.copy()), s.results()
    assert tuple(s.last_instantiation()) == (LAYOUT_NO[layout], 0, 1)
    assert (res.status == _abi.TEB_OK).all()
    np.testing.assert_array_equal(out.n, want_out.n)
    for b in range(f.batch.count):
        for u, v in zip(out.get_teb(b), want_out.get_teb(b)):
            _same(u, v, "band %d" % b)
    for fld in RESULT_FIELDS:
        np.testing.assert_array_equal(getattr(res, fld), getattr(want_res, fld), err_msg=fld)
    best, best_cost = s.select_best_per_scene()
    mo, mv, mw = f.capacities()
    seen = 0
    differs = set()
    for sc in range(f.n_scenes):
        sub, idx = f.scene_batch(sc)
        cfg = cf.cfg_of_scene(sc)
        one = planner.TebBatchSolver(cfg, f.batch.count, f.batch.stride, mo, mv, mw, options=_abi.Options(layout=layout, generic_distance_path=True, **SINGLE))
        one.set_obstacles(f.tables[sc]); one.set_via_points(f.vias[sc])
        one.upload(sub)
        one.optimize(o.no_inner_iterations, o.no_outer_iterations, True, cfg.hcp.selection_obst_cost_scale, cfg.hcp.selection_viapoint_cost_scale,
                     cfg.hcp.selection_alternative_time_cost)
        res1 = one.results()
        for k, b in enumerate(idx):
            _same(res.cost[b], res1.cost[k], "cost of band %d (scene %d, class %d)" % (b, sc, cf.class_of[sc]))
            if not np.array_equal(res.cost[b], want_res.cost[b]):
                differs.add(cf.class_of[sc])
            seen += 1
        b1, c1 = one.select_best()
        assert best[sc] == idx[b1], sc
        _same(best_cost[sc], c1, "selected cost of scene %d" % sc)
        one.close()
    assert seen == f.batch.count
    assert differs == set(range(len(cf.cfgs))), differs   # (the plain run's triple is no class's)
    # without costs nothing is written to them, as for teb_amd_optimize_batch
    s.upload(f.batch)
    s.optimize_per_class(o.no_inner_iterations, o.no_outer_iterations, False)
    assert (s.results().status == _abi.TEB_OK).all()
    s.close()


def test_optimize_per_class_refusals():
    cf = CT.cost_classed_fleet(96)
    f = cf.fleet
    L = planner.lib()
    s = _cost_solver(cf, "cr")
    assert L.teb_amd_optimize_batch_per_class(s._h, -1, 1, 1) == _abi.ERR_INVALID_ARG
    s.set_band_scenes(np.where(f.scene_of == f.n_scenes - 1, f.n_scenes, f.scene_of))
    assert L.teb_amd_optimize_batch_per_class(s._h, 1, 1, 1) == _abi.ERR_INVALID_ARG and b"maps to scene" in L.teb_amd_last_error()
    got = s.download(f.batch.copy())
    _same(got.x, f.batch.x, "nothing ran")
    s.clear_scenes()
    assert L.teb_amd_optimize_batch_per_class(s._h, 1, 1, 1) == _abi.ERR_INVALID_ARG and b"teb_amd_set_scenes" in L.teb_amd_last_error()
    s.close()


# ---- pruning -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_map", [True, False])
def test_every_band_is_pruned_with_min_samples_of_its_class(oracle, with_map):
    f = FT.prune_fleet()
    cfgs = CT.prune_classes(f.cfg)
    handle = copy.deepcopy(f.cfg)
    handle.trajectory.min_samples = 5 if with_map else 8
    a = planner.TebBatchSolver(handle, f.batch.count, f.batch.stride, 4, 4, 4)
    a.set_scenes([_abi.ObstacleTable() for _ in FT.PRUNE_COUNTS])
    if with_map:
        a.set_scene_configs(cfgs, CT.PRUNE_CLASS_OF)
    a.set_band_scenes(f.scene_of)
    a.upload(f.batch)
    b = planner.TebBatchSolver(f.cfg, f.batch.count, f.batch.stride, 4, 4, 4)
    b.upload(f.batch)
    a.update_and_prune_per_class(f.starts, f.goals, f.vels, f.mask)
    changed = 0
    for k in range(f.batch.count):
        sc = int(f.scene_of[k])
        ms = cfgs[CT.PRUNE_CLASS_OF[sc]].trajectory.min_samples if with_map else 8
        b.update_and_prune(f.starts[sc], f.goals[sc], ms, b=k)
        if f.mask[sc]:
            b.set_velocity_start(f.vels[sc], True, b=k)
    ba, bb = a.download(f.batch.copy()), b.download(f.batch.copy())
    np.testing.assert_array_equal(ba.n, bb.n)
    for k in range(f.batch.count):
        sc = int(f.scene_of[k])
        ms = cfgs[CT.PRUNE_CLASS_OF[sc]].trajectory.min_samples if with_map else 8
        want = oracle.update_and_prune(*f.batch.get_teb(k), f.starts[sc], f.goals[sc], ms)
        other = oracle.update_and_prune(*f.batch.get_teb(k), f.starts[sc], f.goals[sc], 3 if ms == 8 else 8)
        changed += len(want[0]) != len(other[0])
        for u, v, w in zip(ba.get_teb(k), bb.get_teb(k), want):
            _same(u, v, "band %d against the per-band call" % k); _same(u, w, "band %d against the oracle" % k)
    assert changed >= 1
    np.testing.assert_array_equal(a.band_flags()[1], b.band_flags()[1])
    L = planner.lib()
    a.clear_scenes()
    assert L.teb_amd_update_and_prune_per_class(a._h, None, None, None, None) == _abi.ERR_INVALID_ARG and b"teb_amd_set_scenes" in L.teb_amd_last_error()
    a.close(); b.close()


# ---- feasibility -------------------------------------------------------------------------------------------------------------------
def _feas_solver(f, cfgs=None, class_of=None):
    s = planner.TebBatchSolver(TebConfig(), f.batch.count, f.batch.stride, 4, 4, 4)
    s.set_scenes([_abi.ObstacleTable() for _ in f.grids])
    if cfgs is not None:
        s.set_scene_configs(cfgs, class_of)
    s.set_band_scenes(f.scene_of)
    s.upload(f.batch)
    s.set_costmaps(f.grids)
    return s


def test_feasibility_with_a_spec_per_scene(oracle):
    f = FT.feasibility_fleet()
    specs = CT.feasibility_specs()
    ns = len(f.grids)
    s = _feas_solver(f)
    use = f.bands.copy()
    use[4] = -3
    ok, first = s.is_trajectory_feasible_per_class(use, specs, CT.FEAS_SPEC_OF)
    differs = set()
    for k in range(ns):
        if use[k] < 0:
            assert (ok[k], first[k]) == (-1, -1)
            continue
        args = CT.spec_args(specs[CT.FEAS_SPEC_OF[k]])
        want = oracle.is_trajectory_feasible(f.batch, int(use[k]), f.grids[k], *args)
        assert (bool(ok[k]), int(first[k])) == want, k
        one = planner.TebBatchSolver(TebConfig(), 1, f.batch.stride, 4, 4, 4)
        one.upload(f.singles[k])
        one.set_costmap(f.grids[k].cells, f.grids[k].resolution, f.grids[k].origin_x, f.grids[k].origin_y)
        assert one.is_trajectory_feasible(0, *args) == want, k
        one.close()
        if want != oracle.is_trajectory_feasible(f.batch, int(use[k]), f.grids[k], *CT.spec_args(specs[0])):
            differs.add(CT.FEAS_SPEC_OF[k])
    assert differs, "no scene tells its spec from spec 0"
    # one spec for every scene is the per-scene call
    for q in specs:
        a = s.is_trajectory_feasible_per_class(f.bands, [q], [0] * ns)
        b = s.is_trajectory_feasible_per_scene(f.bands, *CT.spec_args(q))
        np.testing.assert_array_equal(a[0], b[0]); np.testing.assert_array_equal(a[1], b[1])
        c = s.is_trajectory_feasible_per_class(f.bands, [q])   # no map on the handle: the one spec
        np.testing.assert_array_equal(a[0], c[0]); np.testing.assert_array_equal(a[1], c[1])
    # 64 vertices per spec: the staged array is longer than one footprint
    ring = [(0.3 * np.cos(t), 0.3 * np.sin(t)) for t in np.linspace(0, 2 * np.pi, 64, endpoint=False)]
    big = [dict(specs[0], footprint=ring), dict(specs[1], footprint=ring[::-1]), specs[2]]
    ok, first = s.is_trajectory_feasible_per_class(f.bands, big, CT.FEAS_SPEC_OF)
    for k in range(ns):
        assert (bool(ok[k]), int(first[k])) == oracle.is_trajectory_feasible(f.batch, int(f.bands[k]), f.grids[k], *CT.spec_args(big[CT.FEAS_SPEC_OF[k]])), k
    s.close()
    # spec_of_scene NULL: the class of the scene
    cfgs = [TebConfig(), TebConfig(), TebConfig()]
    s = _feas_solver(f, cfgs, CT.FEAS_SPEC_OF)
    a = s.is_trajectory_feasible_per_class(f.bands, specs)
    b = s.is_trajectory_feasible_per_class(f.bands, specs, CT.FEAS_SPEC_OF)
    np.testing.assert_array_equal(a[0], b[0]); np.testing.assert_array_equal(a[1], b[1])
    with pytest.raises(planner.TebAmdError) as e:
        s.is_trajectory_feasible_per_class(f.bands, specs[:2])
    assert e.value.code == _abi.ERR_INVALID_ARG and "one spec per class" in str(e.value)
    s.close()


def test_feasibility_per_class_refuses_what_it_cannot_answer():
    f = FT.feasibility_fleet()
    specs = CT.feasibility_specs()
    s = _feas_solver(f)
    L = planner.lib()

    def refused(bands, specs_, of=CT.FEAS_SPEC_OF, code=_abi.ERR_INVALID_ARG, word=""):
        with pytest.raises(planner.TebAmdError) as e:
            s.is_trajectory_feasible_per_class(bands, specs_, of)
        assert e.value.code == code and word in str(e.value), str(e.value)

    other = f.bands.copy(); other[2] = f.bands[3]
    refused(other, specs, word="not a band of scene")
    beyond = f.bands.copy(); beyond[0] = f.batch.count
    refused(beyond, specs)
    refused(f.bands, [specs[0], dict(specs[1], inscribed_radius=0.0), specs[2]], word="spec 1")
    refused(f.bands, [specs[0], specs[1], dict(specs[2], min_resolution_collision_check_angular=-1.0)], word="spec 2")
    refused(f.bands, [dict(specs[0], footprint=[(0.0, 0.0)] * 65), specs[1], specs[2]], word="spec 0")
    refused(f.bands, specs, None, word="one spec per class")                    # three specs, no map: one class
    refused(f.bands, [specs[0], dict(specs[1], inscribed_radius=1e-12), specs[2]], code=_abi.ERR_CAPACITY)   # the sample limit of the single call
    # a spec_of_scene entry outside the specs: the wrapper refuses it, and so does the library
    with pytest.raises(ValueError, match="does not fit"):
        s.is_trajectory_feasible_per_class(f.bands, specs, [0, 1, 2, 3, 0, 0, 0, 0])
    arr = (planner.FeasibilitySpec * 1)()
    fx = _abi.f64([0.0]); ok = np.zeros(8, np.int32)
    arr[0] = planner.FeasibilitySpec(1, _abi._ptr(fx, C.c_double), _abi._ptr(fx, C.c_double), 0.2, 0.3, -1, -1.0)
    of = _abi.i32([0, 0, 0, 1, 0, 0, 0, 0]); bands = _abi.i32(f.bands)
    rc = L.teb_amd_is_trajectory_feasible_per_class(s._h, _abi._ptr(bands, C.c_int32), 1, arr, _abi._ptr(of, C.c_int32), _abi._ptr(ok, C.c_int32), None)
    assert rc == _abi.ERR_INVALID_ARG and b"spec_of_scene[3]" in L.teb_amd_last_error()
    s.set_costmaps(f.grids[:-1])
    refused(f.bands, specs, word="costmap set")
    s.set_costmaps(f.grids)
    ok, _ = s.is_trajectory_feasible_per_class(f.bands, specs, CT.FEAS_SPEC_OF)   # the handle is as it was
    assert set(ok) <= {0, 1}
    s.clear_scenes()
    s._n_scenes = len(f.grids)
    refused(f.bands, specs, word="teb_amd_set_scenes")
    s.close()


# ---- the whole tick ----------------------------------------------------------------------------------------------------------------
def _tick_classes():
    """a slow robot that keeps far from obstacles, a fast one that passes close and looks two poses ahead, a default one"""
    out = []
    for k in range(3):
        c = TebConfig()
        c.hcp.max_number_classes = 4
        c.optim.no_inner_iterations = 3; c.optim.no_outer_iterations = 2
        c.recovery.divergence_detection_enable = True
        c.recovery.divergence_detection_max_chi_squared = 2.0
        c.robot.max_vel_trans = c.robot.max_vel_x
        out.append(c)
    a, b, _ = out
    a.robot.max_vel_x, a.robot.max_vel_theta, a.robot.acc_lim_x = 0.3, 0.25, 0.4
    a.robot.max_vel_trans = 0.3
    a.obstacles.min_obstacle_dist, a.obstacles.inflation_dist = 0.35, 0.5
    a.trajectory.min_samples, a.trajectory.force_reinit_new_goal_dist = 6, 0.5
    a.hcp.selection_obst_cost_scale, a.hcp.selection_alternative_time_cost = 3.0, True
    a.hcp.switching_blocking_period = 5.0
    a.recovery.divergence_detection_max_chi_squared = 0.5
    b.robot.max_vel_x, b.robot.max_vel_theta, b.robot.acc_lim_x = 0.8, 0.6, 0.9
    b.robot.max_vel_trans = 0.8
    b.obstacles.min_obstacle_dist = 0.15
    b.trajectory.control_look_ahead_poses, b.trajectory.prevent_look_ahead_poses_near_goal = 2, 1
    b.trajectory.feasibility_check_no_poses = 8
    b.trajectory.min_resolution_collision_check_angular = 0.3
    b.hcp.selection_viapoint_cost_scale, b.hcp.selection_cost_hysteresis = 0.5, 0.8
    return out


@pytest.mark.parametrize("route", ["points", "polygons"])
def test_whole_ticks_of_a_mixed_fleet_beside_one_planner_per_robot(route):
    R = 4
    class_of = [0, 1, 2, 1]
    cfgs = _tick_classes()
    rng = np.random.default_rng(515)
    origins = [(-7.0, 3.0), (11.0, -4.0), (2.5, 9.0), (-12.0, -8.0)]
    grids = [_tick_costmap(rng, ox, oy) for ox, oy in origins]
    customs = [None, FT.custom_pointlike(origins[1][0] + 1.0, origins[1][1] + 3.0), None, None]
    tables = [c if c is not None else _abi.ObstacleTable() for c in customs]
    starts = [(ox + 0.6, oy + 3.0, 0.0) for ox, oy in origins]
    goals = [(ox + 5.0, oy + 3.0 + 0.2 * r, 0.0) for r, (ox, oy) in enumerate(origins)]
    vels = [(0.0, 0.0, 0.0)] * R
    dist = cfgs[0].obstacles.costmap_obstacles_behind_robot_dist
    tiles = None if route == "points" else [8, 1, 8, 4]   # the tile size is per robot
    cap, vcap = 64, 64
    fleet = planner.FleetHomotopyClassPlanner(FC.handle_config_that_differs(cfgs), R, max_tebs=4 * R, max_poses=96, max_obstacles=R * cap,
                                              max_obstacle_vertices=R * vcap, max_via_points=4, options=_abi.Options(**SINGLE), robot_cfgs=cfgs,
                                              class_of_robot=class_of)
    ones = []
    for r in range(R):
        cfg = cfgs[class_of[r]]
        hp = planner.HomotopyClassPlanner(cfg, _abi.ObstacleTable(), [], None, max_tebs=4, max_poses=96)
        hp.solver.close()
        hp.solver = planner.TebBatchSolver(cfg, 4, 96, cap, vcap, 4, options=_abi.Options(**SINGLE))
        hp.solver.set_via_points([])
        ones.append(hp)
    # per class: the last tick's footprint of class 1 is wide - bands near a blob become infeasible
    footprints = [[feasibility_cases.FOOTPRINTS["tri"], feasibility_cases.FOOTPRINTS["rect"], feasibility_cases.FOOTPRINTS["point1"]],
                  [feasibility_cases.FOOTPRINTS["rect"], feasibility_cases.FOOTPRINTS["tri"], feasibility_cases.FOOTPRINTS["tri"]],
                  [feasibility_cases.FOOTPRINTS["tri"], [(-0.3, -0.9), (0.9, -0.9), (0.9, 0.9), (-0.3, 0.9)], feasibility_cases.FOOTPRINTS["rect"]]]
    radii = [0.25, 0.2, 0.3]
    infeasible_seen = False
    for tick in range(3):
        best = fleet.plan(starts, goals, vels, tables, None, now=float(tick + 1), costmaps_per_robot=grids, costmap_tile_cells=tiles)
        for r, hp in enumerate(ones):
            g = grids[r]
            hp.solver.set_costmap(g.cells, g.resolution, g.origin_x, g.origin_y)
            if tiles is None:
                n = hp.solver.set_obstacles_from_costmap(starts[r], dist, customs[r])[0]
            else:
                n = len(hp.solver.set_obstacles_from_costmap_polygons(starts[r], dist, tiles[r], customs[r]))
            assert 1 <= n <= cap - 3
            hp.plan(starts[r], goals[r], vels[r])
        bands = fleet.bands()
        cost = fleet.results().cost
        for r, hp in enumerate(ones):
            mine, want = fleet.bands_of(r), hp.bands()
            assert len(mine) == len(want) >= 1, (tick, r)
            for k, b in enumerate(mine):
                for u, v in zip(bands[b], want[k]):
                    _same(u, v, "tick %d robot %d band %d" % (tick, r, k))
            _same(cost[mine], hp.results().cost[:len(want)], "tick %d costs of robot %d" % (tick, r))
            assert best[r] == mine[hp.best_teb_], (tick, r)
        assert fleet.hasDiverged() == [hp.solver.has_diverged(hp.best_teb_) for hp in ones], tick
        t_of = [cfgs[class_of[r]].trajectory for r in range(R)]
        held = [len(fleet.bands_of(r)) for r in range(R)]
        verdict = fleet.isTrajectoryFeasible(footprints[tick], radii, 0.0, [c.trajectory.feasibility_check_no_poses for c in cfgs],
                                             [c.trajectory.feasibility_check_lookahead_distance for c in cfgs])
        want_verdict = [hp.isTrajectoryFeasible(grids[r], footprints[tick][class_of[r]], radii[class_of[r]], 0.0, t_of[r].feasibility_check_no_poses,
                                                t_of[r].feasibility_check_lookahead_distance) for r, hp in enumerate(ones)]
        assert verdict == want_verdict, tick
        bands = fleet.bands()
        for r, hp in enumerate(ones):                                          # the checks removed the same bands on both sides
            mine, want = fleet.bands_of(r), hp.bands()
            assert len(mine) == len(want), (tick, r)
            infeasible_seen = infeasible_seen or len(mine) < held[r]              # an infeasible best band was removed
            for k, b in enumerate(mine):
                for u, v in zip(bands[b], want[k]):
                    _same(u, v, "after the check: tick %d robot %d band %d" % (tick, r, k))
            assert (fleet.best_teb_[r] < 0) == (hp.best_teb_ < 0)
            if hp.best_teb_ >= 0:
                assert fleet.best_teb_[r] == mine[hp.best_teb_]
        cmds = fleet.getVelocityCommands()
        for r, hp in enumerate(ones):
            w = hp.getVelocityCommand()
            assert cmds[r][0] == w[0]
            _same(np.array(cmds[r][1:]), np.array(w[1:]), "command of robot %d" % r)
        nxt, nv = [], []
        for r in range(R):
            if fleet.best_teb_[r] >= 0:
                x, y, th, _ = bands[int(fleet.best_teb_[r])]
                nxt.append((float(x[1]), float(y[1]), float(th[1]))); nv.append(cmds[r][1:])
            else:
                nxt.append(starts[r]); nv.append((0.0, 0.0, 0.0))
        starts, vels = nxt, nv
    assert infeasible_seen, "no best band was infeasible: the wide footprint never met a blob"
    for hp in ones:
        hp.solver.close()
    fleet.solver.close()


def test_compute_velocity_commands_saturates_with_each_class_limits():
    """computeVelocityCommands over setPlans: the mixed fleet beside one single-robot FleetHomotopyClassPlanner per robot created with the
    robot's class - the same status, the same saturated command."""
    from test_gpu_fleet_adapter import _grids, _plans, _pose_on, PARAMS, FOOTPRINT
    grids = _grids()
    plans = _plans(grids)
    R = 3
    class_of = [1, 0, 2]
    cfgs = _tick_classes()
    for c in cfgs:
        c.hcp.max_number_classes = 3
        c.recovery.divergence_detection_enable = False   # (the tight chi^2 bounds of the tick test would end the first tick here)
    opts = dict(max_poses=96, max_obstacle_vertices=8, max_via_points=16, options=_abi.Options(**SINGLE))
    fleet = planner.FleetHomotopyClassPlanner(FC.handle_config_that_differs(cfgs), R, max_tebs=3 * R, max_obstacles=R * 256, robot_cfgs=cfgs,
                                              class_of_robot=class_of, **opts)
    fleet.setPlans(plans)
    ones = []
    for r in range(R):
        one = planner.FleetHomotopyClassPlanner(cfgs[class_of[r]], 1, max_tebs=3, max_obstacles=256, **opts)
        one.setPlans([plans[r]])
        ones.append(one)
    wp = _abi.PlanWindowParams(**dict(PW.DEFAULTS, **PARAMS))
    for tick in range(2):
        poses = [_pose_on(plans[r], 8 * tick + r, 0.05 * r) for r in range(R)]
        vels = [(0.1 * tick, 0.0, 0.02 * r) for r in range(R)]
        status, cmd = fleet.computeVelocityCommands(poses, vels, grids, FOOTPRINT, 0.2, window_params=wp, now=float(tick + 1))
        for r, one in enumerate(ones):
            st1, cmd1 = one.computeVelocityCommands([poses[r]], [vels[r]], [grids[r]], FOOTPRINT, 0.2, window_params=wp, now=float(tick + 1))
            assert status[r] == st1[0] == fleet.SUCCESS, (tick, r, status, st1, {k: v for k, v in fleet.last_tick.items() if k != "windows"})
            _same(cmd[r], cmd1[0], "tick %d command of robot %d" % (tick, r))
            rb = cfgs[class_of[r]].robot
            assert abs(cmd[r][0]) <= rb.max_vel_x and abs(cmd[r][2]) <= rb.max_vel_theta
    for one in ones:
        one.solver.close()
    fleet.solver.close()
