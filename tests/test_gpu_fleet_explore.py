"""Candidate exploration per scene of a fleet batch on the MI355X (include/teb_amd.h: teb_amd_explore_candidates_per_scene,
teb_amd_get_exploration_graph_per_scene, teb_amd_compact_bands_per_scene) - exploreEquivalenceClassesAndInitTebs of every robot of a
fleet on one handle.

  * bit identity: the bands of every scene, in band order, equal the batch of a single-scene handle that holds only that scene, held the
    same bands and ran the single-scene sequence (signatures, class filter, detours, compact, explore) - bands, flags, start velocity,
    counts, graph; both graphs, 2-D and 3-D signatures, point and mixed obstacles, given samples and each scene's own generator;
  * the result does not depend on the number of paths a scene contributes to a round;
  * every scene against the CPU oracle, independent of the device's single-scene path;
  * teb_amd_compact_bands_per_scene against teb_amd_compact_bands on the single-scene handles; state and errors;
  * FleetHomotopyClassPlanner tick after tick beside one HomotopyClassPlanner per robot.

The fixtures (tests/fleet_explore_cases.py) and what the tests rely on are checked on the CPU in tests/test_fleet_explore.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.path.insert(0, HERE)
import fleet_explore_cases as FE  # noqa: E402
from test_reference_pinning import renew_on_host, kept_via_flags  # noqa: E402

from teb_local_planner_amd import _abi, planner  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = 1e-12   # of tests/test_gpu_candidates.py
SINGLE = dict(generic_config_path=True, multi_cu=-1, speculative_trials=-1)   # the fleet contract of include/teb_amd.h
MAX_TEBS = FE.N_SCENES * 4   # sum over the scenes of max(bands, max_number_classes): the capacity rule, met exactly


def _fleet_solver(f, max_tebs=MAX_TEBS, before_scenes=None):
    mo, mv, mw = f.capacities()
    s = planner.TebBatchSolver(f.cfg, max_tebs, f.batch.stride, mo, mv, mw, options=_abi.Options(**SINGLE))
    if before_scenes:
        before_scenes(s)
    s.set_scenes(f.tables, f.vias)
    s.set_band_scenes(f.scene_of)
    s.upload(f.batch)
    s.set_optimized_flags([1] * f.batch.count)
    return s


def _single_solver(f, sc, max_tebs=MAX_TEBS):
    """the reference handle of scene sc: same capacities, the options of the fleet contract, the scene's table, via-points and bands"""
    mo, mv, mw = f.capacities()
    s = planner.TebBatchSolver(f.cfg, max_tebs, f.batch.stride, mo, mv, mw, options=_abi.Options(**SINGLE))
    s.set_obstacles(f.tables[sc])
    s.set_via_points(f.vias[sc])
    sub, idx = f.scene_batch(sc)
    if idx:
        s.upload(sub)
        s.set_optimized_flags([1] * len(idx))
    return s


def _renew_fleet(s, f):
    h = f.cfg.hcp
    s.h_signatures_per_scene(h.h_signature_prescaler, values=False)
    keep, _, _ = s.filter_equivalence_classes_per_scene(h.h_signature_threshold, f.best, h.max_number_plans_in_current_class)
    keep = s.filter_detours_per_scene(keep, f.best)
    return s.compact_bands_per_scene(keep, f.best)[1]


def _renew_single(s, f, sc):
    h = f.cfg.hcp
    if s.count == 0:
        return -1
    best = f.scene_case(sc)["best"]
    s.h_signatures(h.h_signature_prescaler, values=False)
    keep, _, _ = s.filter_equivalence_classes(h.h_signature_threshold, best, h.max_number_plans_in_current_class)
    keep = s.filter_detours(keep, best)
    return s.compact_bands(keep, best)[1]


def _explore_fleet(s, f, best, us=None):
    return s.explore_candidates_per_scene(f.starts, f.goals, f.dist_to_obst, None, False, best, us, f.max_paths, initial_plans=f.plans)


def _explore_single(s, f, sc, best, us=None):
    return s.explore_candidates(f.starts[sc], f.goals[sc], f.dist_to_obst, None, False, best, None if us is None else us[sc], f.max_paths,
                                initial_plan=f.plans[sc])


def _state(s, stride):
    """everything a band carries that the exploration writes: (host batch, via_en, has_vs, has_vg)"""
    b = _abi.TebBatchHost(max(s.count, 1), stride)
    if s.count:
        s.download(b)
    return (b,) + tuple(s.band_flags()) if s.count else (b, np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.int32))


def _assert_scene_equals_single(sf, fstate, scene_of, r, sc, s1, r1, stride):
    mine = np.nonzero(scene_of == sc)[0]
    what = "scene %d" % sc
    assert r["n_bands"][sc] == len(mine) == r1["n_total"] == s1.count, what
    assert r["n_vertices"][sc] == r1["n_vertices"] and r["n_paths"][sc] == r1["n_paths"], what
    assert r["initial_plan_teb"][sc] == r1["initial_plan_teb"], what
    V, A = sf.exploration_graph_per_scene(sc)
    V1, A1 = s1.exploration_graph()
    assert len(V) == r["n_vertices"][sc]
    np.testing.assert_array_equal(V, V1, err_msg=what)
    np.testing.assert_array_equal(A, A1, err_msg=what)
    fb, fve, fvs, fvg = fstate
    ob, ove, ovs, ovg = _state(s1, stride)
    for k, b in enumerate(mine):
        for u, v in zip(fb.get_teb(int(b)), ob.get_teb(k)):
            np.testing.assert_array_equal(u, v, err_msg="%s, band %d (its %d.)" % (what, b, k))
        np.testing.assert_array_equal(fb.vel_start[b], ob.vel_start[k])
        assert (fve[b], fvs[b], fvg[b]) == (ove[k], ovs[k], ovg[k]), (what, k)


def _compare_all(sf, f, r, singles, results):
    scene_of = sf.band_scenes()
    assert r["n_total"] == sf.count == len(scene_of) == sum(r["n_bands"])
    fstate = _state(sf, f.batch.stride)
    for sc in range(f.n_scenes):   # every scene, none skipped
        _assert_scene_equals_single(sf, fstate, scene_of, r, sc, singles[sc], results[sc], f.batch.stride)


CASES = [(k, d, g, 15) for k in ("points", "mixed") for d in (True, False) for g in ("keypoint", "roadmap")] + \
        [("points", True, "roadmap", 13), ("points", False, "roadmap", 14)]


@pytest.mark.parametrize("kind,dynamic,graph,samples", CASES)
def test_every_scene_equals_its_single_scene_handle_bit_for_bit(kind, dynamic, graph, samples):
    f = FE.explore_fleet(kind, dynamic, keypoint=(graph == "keypoint"), no_samples=samples, plans_in_class=2,
                         viapoints_all_candidates=(samples != 15 or kind == "points"))
    us = FE.unit_samples(f)
    sf = _fleet_solver(f)
    new_best = _renew_fleet(sf, f)
    before = sf.count
    r = _explore_fleet(sf, f, new_best, us)
    assert r["n_total"] > before
    singles, results = [], []
    for sc in range(f.n_scenes):
        s1 = _single_solver(f, sc)
        b1 = _renew_single(s1, f, sc)
        results.append(_explore_single(s1, f, sc, b1, us))
        singles.append(s1)
    _compare_all(sf, f, r, singles, results)
    # the map on the device is the map on the host: one optimise launch over the new batch runs every band against its scene
    assert (sf.band_scenes()[before:] < f.n_scenes).all()
    for s1 in singles:
        s1.close()
    sf.close()


@pytest.mark.parametrize("dynamic", [True, False])
def test_every_scene_draws_from_its_own_generator(dynamic):
    """no unit samples: two consecutive calls; the second continues every scene's generator, and the scene that was full in the first
    call - it returned before its graph and drew nothing - starts from a fresh one, like its single-scene handle"""
    f = FE.explore_fleet("points", dynamic, keypoint=False, plans_in_class=2)
    sf = _fleet_solver(f)
    new_best = _renew_fleet(sf, f)
    singles = [_single_solver(f, sc) for sc in range(f.n_scenes)]
    bests = [_renew_single(s1, f, sc) for sc, s1 in enumerate(singles)]
    r = _explore_fleet(sf, f, new_best)
    results = [_explore_single(s1, f, sc, bests[sc]) for sc, s1 in enumerate(singles)]
    assert r["n_vertices"][FE.FULL] == 0 and r["n_vertices"][FE.PLAIN] == f.cfg.hcp.roadmap_graph_no_samples + 2
    _compare_all(sf, f, r, singles, results)
    first = sf.exploration_graph_per_scene(FE.PLAIN)[0]
    # tebs_.clear() everywhere, then again: now every scene but the two at their goal reaches its graph
    sf.compact_bands_per_scene(np.zeros(sf.count, np.int32), None)
    for s1 in singles:
        if s1.count:
            s1.compact_bands(np.zeros(s1.count, np.int32))
    r = _explore_fleet(sf, f, None)
    results = [_explore_single(s1, f, sc, -1) for sc, s1 in enumerate(singles)]
    assert r["n_vertices"][FE.FULL] == f.cfg.hcp.roadmap_graph_no_samples + 2
    assert not np.array_equal(first, sf.exploration_graph_per_scene(FE.PLAIN)[0])   # the continuation, not the same samples again
    _compare_all(sf, f, r, singles, results)
    for s1 in singles:
        s1.close()
    sf.close()


@pytest.mark.parametrize("graph", ["keypoint", "roadmap"])
def test_result_does_not_depend_on_the_paths_per_round(graph):
    f = FE.explore_fleet("points", True, keypoint=(graph == "keypoint"), plans_in_class=2)
    us = FE.unit_samples(f)
    seen = {}
    for q in (0, 1, 3, 64):
        sf = _fleet_solver(f)
        sf.debug_set_explore_quota(q)
        r = _explore_fleet(sf, f, _renew_fleet(sf, f), us)
        scene_of = sf.band_scenes()
        fb, fve, fvs, fvg = _state(sf, f.batch.stride)
        per_scene = []
        for sc in range(f.n_scenes):
            mine = np.nonzero(scene_of == sc)[0]
            per_scene.append(([fb.get_teb(int(b)) for b in mine], fve[mine], fvs[mine], fvg[mine], sf.exploration_graph_per_scene(sc)))
        seen[q] = (r, per_scene)
        sf.close()
    r0, p0 = seen[0]
    assert r0["n_paths"].max() > 2 * FE.QUOTA or graph == "keypoint"
    for q in (1, 3, 64):
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


@pytest.mark.parametrize("kind,dynamic,graph", [(k, d, g) for k in ("points", "mixed") for d in (True, False) for g in ("keypoint", "roadmap")])
def test_every_scene_against_the_oracle(oracle, kind, dynamic, graph):
    f = FE.explore_fleet(kind, dynamic, keypoint=(graph == "keypoint"), plans_in_class=2, viapoints_all_candidates=(kind == "mixed"))
    us = FE.unit_samples(f)
    sf = _fleet_solver(f)
    r = _explore_fleet(sf, f, _renew_fleet(sf, f), us)
    scene_of = sf.band_scenes()
    fb, fve, _, _ = _state(sf, f.batch.stride)
    total = 0
    for sc in range(f.n_scenes):
        case = f.scene_case(sc)
        b, n_tebs, best = renew_on_host(oracle, case, slots=8)
        o = oracle.explore_candidates(f.cfg, f.tables[sc], b, n_tebs, best, case["start"], case["goal"], unit_samples=us[sc], max_paths=f.max_paths,
                                      dist_to_obst=f.dist_to_obst, initial_plan=case["initial_plan"], via_enabled=kept_via_flags(oracle, case, b.count))
        mine = np.nonzero(scene_of == sc)[0]
        assert r["n_bands"][sc] == o["n_total"] == len(mine), sc
        assert r["initial_plan_teb"][sc] == o["initial_plan_teb"], sc
        assert r["n_vertices"][sc] == len(o["vertices"]), sc
        if o["n_total"] > n_tebs:
            assert r["n_paths"][sc] <= o["n_paths"] or o["n_paths"] == 0   # the relation of tests/test_gpu_candidates.py
        V, A = sf.exploration_graph_per_scene(sc)
        if len(o["vertices"]):
            assert np.abs(V - o["vertices"]).max() <= TOL
            want = np.zeros_like(A)
            for i, row in enumerate(o["adjacency"]):
                want[i, row] = 1
            np.testing.assert_array_equal(A, want)
        for k, bnd in enumerate(mine):
            for u, v in zip(fb.get_teb(int(bnd)), o["batch"].get_teb(k)):
                assert len(u) == len(v) and np.abs(u - v).max(initial=0) <= TOL, (sc, k)
        if f.vias[sc]:
            np.testing.assert_array_equal(fve[mine], o["via_enabled"][:o["n_total"]])
        total += o["n_total"]
    assert r["n_total"] == total
    sf.close()


def _compact_case(f, keep, best):
    """per-scene compaction on the fleet handle beside compact_bands on the handles of the scenes"""
    f.batch.vel_start[:] = np.arange(3 * f.batch.count).reshape(-1, 3) * 0.01   # attributes travel with their band
    f.batch.has_vel_start[:] = 1
    sf = _fleet_solver(f)
    nk, nb = sf.compact_bands_per_scene(keep, best)
    assert nk == int(np.count_nonzero(keep)) == sf.count
    scene_of = sf.band_scenes()
    fb = _state(sf, f.batch.stride)[0]
    for sc in range(f.n_scenes):
        idx = f.bands_of(sc)
        mine = np.nonzero(scene_of == sc)[0]
        if not idx:
            assert len(mine) == 0 and nb[sc] == -1
            continue
        s1 = _single_solver(f, sc)
        b1 = -1 if best is None or best[sc] < 0 else idx.index(int(best[sc]))
        nk1, nb1 = s1.compact_bands(np.asarray(keep)[idx], b1)
        assert nk1 == len(mine), sc
        assert (nb[sc] == -1) == (nb1 == -1) and (nb1 == -1 or mine[nb1] == nb[sc]), (sc, nb[sc], nb1)
        ob = _state(s1, f.batch.stride)[0]
        for k, b in enumerate(mine):
            for u, v in zip(fb.get_teb(int(b)), ob.get_teb(k)):
                np.testing.assert_array_equal(u, v, err_msg="scene %d band %d" % (sc, k))
            np.testing.assert_array_equal(fb.vel_start[b], ob.vel_start[k])
        s1.close()
    sf.close()
    return nk, nb, scene_of


def test_compact_bands_per_scene_equals_compact_bands_scene_by_scene():
    f = FE.explore_fleet("points", True)
    B = f.batch.count
    full, bst = f.bands_of(FE.FULL), f.bands_of(FE.BEST)
    best = np.full(f.n_scenes, -1, np.int32)
    best[FE.FULL] = full[2]      # in the middle of its scene
    best[FE.BEST] = bst[0]       # first already
    keep = np.ones(B, np.int32)
    keep[full[1]] = 0
    keep[f.bands_of(FE.PLAN_NEW)] = 0    # a scene that loses all its bands
    nk, nb, scene_of = _compact_case(f, keep, best)
    assert nb[FE.FULL] >= 0 and nb[FE.BEST] >= 0 and (scene_of == FE.PLAN_NEW).sum() == 0
    assert scene_of[nb[FE.FULL]] == FE.FULL and nb[FE.FULL] == np.nonzero(scene_of == FE.FULL)[0][0]
    # the kept bands move to the front in band order with the two best bands exchanged with their scene's first: the map follows
    order = list(range(B))
    for sc in (FE.FULL, FE.BEST):
        a, b = f.bands_of(sc)[0], int(best[sc])
        order[a], order[b] = order[b], order[a]
    np.testing.assert_array_equal(scene_of, [f.scene_of[b] for b in order if keep[b]])
    # a best band that is dropped; no best at all; the identity
    keep2 = np.ones(B, np.int32); keep2[full[2]] = 0
    assert _compact_case(FE.explore_fleet("points", True), keep2, best)[1][FE.FULL] == -1
    nk, nb, scene_of = _compact_case(FE.explore_fleet("points", True), keep, None)
    assert (nb == -1).all()
    nk, nb, scene_of = _compact_case(FE.explore_fleet("points", True), np.ones(B, np.int32), None)
    assert nk == B
    np.testing.assert_array_equal(scene_of, f.scene_of)


def test_state_and_errors():
    f = FE.explore_fleet("points", True, keypoint=False)
    L = planner.lib()
    p = f.cfg.hcp_params()
    D = lambda a: _abi._ptr(np.ascontiguousarray(a, np.float64), C.c_double)
    st, gl = np.ascontiguousarray(f.starts), np.ascontiguousarray(f.goals)
    # single-scene mode: refused, and the message names the call that sets scenes
    one = _single_solver(f, FE.BEST)
    nt = C.c_int32(0)
    rc = L.teb_amd_explore_candidates_per_scene(one._h, C.byref(p), D(st), D(gl), 0.2, None, 0, None, None, 0, C.byref(nt), None, None, None, None, None, None, None, None)
    assert rc == _abi.ERR_INVALID_ARG and b"teb_amd_set_scenes" in L.teb_amd_last_error()
    assert L.teb_amd_compact_bands_per_scene(one._h, _abi._ptr(np.ones(3, np.int32), C.c_int32), None, None, None) == _abi.ERR_INVALID_ARG
    assert b"teb_amd_set_scenes" in L.teb_amd_last_error()
    assert L.teb_amd_get_exploration_graph_per_scene(one._h, 0, None, None, None, 0, C.byref(nt)) == _abi.ERR_INVALID_ARG
    assert b"teb_amd_set_scenes" in L.teb_amd_last_error()
    # the capacity rule: one slot short, nothing changes
    sf = _fleet_solver(f, max_tebs=MAX_TEBS - 1)
    before = _state(sf, f.batch.stride)
    with pytest.raises(planner.TebAmdError) as e:
        _explore_fleet(sf, f, f.best)
    assert e.value.code == _abi.ERR_CAPACITY
    after = _state(sf, f.batch.stride)
    assert sf.count == f.batch.count
    np.testing.assert_array_equal(sf.band_scenes(), f.scene_of)
    for k in range(f.batch.count):
        for u, v in zip(before[0].get_teb(k), after[0].get_teb(k)):
            np.testing.assert_array_equal(u, v)
    # (the per-scene signatures stay as they were: none were computed, so the filter still asks for them)
    sf.close()
    # best of another scene
    sf = _fleet_solver(f, before_scenes=lambda s: (s.set_obstacles(f.tables[FE.PLAIN]), s.set_via_points([])))
    wrong = f.best.copy(); wrong[FE.FULL] = f.bands_of(FE.BEST)[0]
    with pytest.raises(planner.TebAmdError) as e:
        _explore_fleet(sf, f, wrong)
    assert e.value.code == _abi.ERR_INVALID_ARG and "not a band of scene" in str(e.value)
    with pytest.raises(planner.TebAmdError) as e:
        sf.compact_bands_per_scene(np.ones(sf.count, np.int32), wrong)
    assert e.value.code == _abi.ERR_INVALID_ARG
    assert sf.count == f.batch.count
    # the call changes the bands: the per-scene class filter asks for new signatures
    sf.h_signatures_per_scene(f.cfg.hcp.h_signature_prescaler, values=False)
    sf.filter_equivalence_classes_per_scene(0.1, f.best)
    r = _explore_fleet(sf, f, f.best)
    assert r["n_total"] > f.batch.count
    with pytest.raises(planner.TebAmdError) as e:
        sf.filter_equivalence_classes_per_scene(0.1, None)
    assert "first" in str(e.value)
    # after clear_scenes the single scene explores as on a fresh handle: its generator was not advanced, no class remembered
    sf.compact_bands_per_scene(np.zeros(sf.count, np.int32), None)
    sf.clear_scenes()
    fresh = planner.TebBatchSolver(f.cfg, MAX_TEBS, f.batch.stride, *f.capacities(), options=_abi.Options(**SINGLE))
    fresh.set_obstacles(f.tables[FE.PLAIN]); fresh.set_via_points([])
    got = [s.explore_candidates(f.starts[FE.PLAIN], f.goals[FE.PLAIN], f.dist_to_obst, max_paths=f.max_paths) for s in (sf, fresh)]
    assert got[0] == got[1] and got[0]["n_total"] >= 1 and got[0]["n_vertices"] == f.cfg.hcp.roadmap_graph_no_samples + 2
    (V0, A0), (V1, A1) = sf.exploration_graph(), fresh.exploration_graph()
    np.testing.assert_array_equal(V0, V1); np.testing.assert_array_equal(A0, A1)
    a, b = _state(sf, f.batch.stride)[0], _state(fresh, f.batch.stride)[0]
    for k in range(sf.count):
        for u, v in zip(a.get_teb(k), b.get_teb(k)):
            np.testing.assert_array_equal(u, v)
    for s in (one, sf, fresh):
        s.close()


def test_whole_ticks_beside_one_planner_per_robot():
    """FleetHomotopyClassPlanner with four robots, three ticks with starts that advance along the best band and a fourth with a goal jump
    for one robot only, beside four HomotopyClassPlanner on handles of the fleet contract driven through the same steps: bands, costs
    and the best band of every robot bit for bit."""
    f = FE.explore_fleet("points", True, keypoint=True)
    robots = [FE.PLAIN, FE.PLAN_OLD, FE.PLAN_NEW, FE.EMPTY]
    cfg = f.cfg
    cfg.optim.no_inner_iterations = 3; cfg.optim.no_outer_iterations = 2
    tables = [f.tables[s] for s in robots]; vias = [f.vias[s] for s in robots]
    mo, mv, mw = f.capacities()
    fleet = planner.FleetHomotopyClassPlanner(cfg, 4, max_tebs=16, max_poses=96, max_obstacles=mo, max_obstacle_vertices=mv, max_via_points=mw,
                                              options=_abi.Options(**SINGLE))
    ones = []
    for r in range(4):
        hp = planner.HomotopyClassPlanner(cfg, tables[r], vias[r], None, max_tebs=16, max_poses=96)
        hp.solver.close()
        hp.solver = planner.TebBatchSolver(cfg, 16, 96, mo, mv, mw, options=_abi.Options(**SINGLE))
        hp.solver.set_obstacles(tables[r]); hp.solver.set_via_points(vias[r])
        ones.append(hp)
    starts = [tuple(f.starts[s]) for s in robots]
    goals = [tuple(f.goals[s]) for s in robots]
    vels = [(0.0, 0.0, 0.0)] * 4
    for tick in range(4):
        if tick == 3:   # a goal jump for robot 1 only: its bands are dropped, the others warm-start
            goals[1] = (goals[1][0] + 1.5, goals[1][1] + 0.5, goals[1][2])
        best = fleet.plan(starts, goals, vels, tables, vias, now=float(tick + 1))
        bands = fleet.bands()
        cost = fleet.results().cost
        for r in range(4):
            hp = ones[r]
            hp.plan(starts[r], goals[r], vels[r])
            mine = fleet.bands_of(r)
            want = hp.bands()
            assert len(mine) == len(want) >= 1, (tick, r)
            if tick == 3 and r == 1:
                assert all(abs(w[0][-1] - goals[1][0]) < 1e-9 for w in want)
            for k, b in enumerate(mine):
                for u, v in zip(bands[b], want[k]):
                    np.testing.assert_array_equal(u, v, err_msg="tick %d robot %d band %d" % (tick, r, k))
            np.testing.assert_array_equal(cost[mine], hp.results().cost[:len(want)])
            assert best[r] == mine[hp.best_teb_], (tick, r)
            assert (fleet.initial_plan_teb_[r] < 0) == (hp.initial_plan_teb_ < 0)
        cmds = fleet.getVelocityCommands()
        assert all(c[0] for c in cmds)
        x, y, th, _ = zip(*[bands[int(b)] for b in best])
        starts = [(float(x[r][1]), float(y[r][1]), float(th[r][1])) for r in range(4)]
        vels = [(c[1], c[2], c[3]) for c in cmds]
    for hp in ones:
        hp.solver.close()
    fleet.solver.close()
