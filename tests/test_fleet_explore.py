"""Candidate exploration per scene of a fleet batch, the part that needs no device: the three calls and the debug hook are declared,
exported and bound; the Python wrappers check their lengths before they enter the library; and the fixtures of
tests/fleet_explore_cases.py hold what tests/test_gpu_fleet_explore.py relies on - checked scene by scene with the CPU oracle
(oracle.explore_candidates, bit-equal to the reference's graph search on such cases: tests/test_reference_pinning.py)."""
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.path.insert(0, HERE)
import fleet_explore_cases as FE  # noqa: E402
from test_reference_pinning import renew_on_host, kept_via_flags  # noqa: E402

from teb_local_planner_amd import _abi, planner  # noqa: E402

ROOT = os.path.dirname(HERE)
CALLS = ("teb_amd_explore_candidates_per_scene", "teb_amd_get_exploration_graph_per_scene", "teb_amd_compact_bands_per_scene", "teb_amd_get_band_scenes")
HOOK = "teb_amd_debug_set_explore_quota"
MARGIN = 1e-6


def _declared(header):
    src = open(os.path.join(ROOT, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return set(re.findall(r"\b(teb_amd_[a-z0-9_]+)\s*\(", src))


def test_calls_and_hook_are_declared_exported_and_bound():
    L = planner.lib()
    assert set(CALLS) <= _declared("teb_amd.h") and HOOK in _declared("teb_amd_debug.h")
    for n in CALLS + (HOOK,):
        assert hasattr(L, n), "libteb_amd.so does not export %s" % n
        assert getattr(L, n).argtypes, "no ctypes signature for %s" % n
    assert len(L.teb_amd_explore_candidates_per_scene.argtypes) == 19
    assert len(L.teb_amd_get_exploration_graph_per_scene.argtypes) == 7
    assert len(L.teb_amd_compact_bands_per_scene.argtypes) == 5
    assert L.teb_amd_abi_version() == 3   # additive


def test_header_points_the_refused_call_at_the_per_scene_one():
    src = open(os.path.join(ROOT, "include", "teb_amd.h")).read()
    assert "does not exist yet" not in src
    assert re.search(r"teb_amd_explore_candidates \(teb_amd_explore_candidates_per_scene takes its place\)", src)


def _unbound_solver(n_scenes):
    """a TebBatchSolver without a handle: the wrappers have to raise before they touch it"""
    s = object.__new__(planner.TebBatchSolver)
    s._h = None
    s.cfg = FE.explore_fleet().cfg
    s._n_scenes = n_scenes
    s.count = 0
    return s


def test_wrappers_check_lengths_before_the_library_is_entered():
    f = FE.explore_fleet()
    s = _unbound_solver(f.n_scenes)
    ok = dict(starts=f.starts, goals=f.goals)
    with pytest.raises(ValueError, match="starts"):
        s.explore_candidates_per_scene(f.starts[:-1], f.goals)
    with pytest.raises(ValueError, match="goals"):
        s.explore_candidates_per_scene(f.starts, list(f.goals) + [f.goals[0]])
    with pytest.raises(ValueError, match="start velocities"):
        s.explore_candidates_per_scene(start_vels=np.zeros((3, 3)), **ok)
    with pytest.raises(ValueError, match="best"):
        s.explore_candidates_per_scene(best=[-1] * (f.n_scenes + 1), **ok)
    with pytest.raises(ValueError, match="unit sample"):
        s.explore_candidates_per_scene(unit_samples=FE.unit_samples(f)[1:], **ok)
    with pytest.raises(ValueError, match="values per scene"):
        s.explore_candidates_per_scene(unit_samples=FE.unit_samples(f)[:, :-2], **ok)
    with pytest.raises(ValueError, match="initial plans"):
        s.explore_candidates_per_scene(initial_plans=f.plans[:-1], **ok)
    with pytest.raises(ValueError, match="best"):
        s.compact_bands_per_scene(np.ones(4, np.int32), best=[0, 1])
    fp = object.__new__(planner.FleetHomotopyClassPlanner)
    fp.n_robots = 4
    with pytest.raises(ValueError, match="robots"):
        fp.plan([(0, 0, 0)] * 3, [(1, 0, 0)] * 4, None, [None] * 4)
    cfg = FE.explore_fleet().cfg
    cfg.hcp.selection_dropping_probability = 0.1
    with pytest.raises(NotImplementedError):
        planner.FleetHomotopyClassPlanner(cfg, 2)


GRAPHS = [("keypoint", 15), ("roadmap", 13), ("roadmap", 14), ("roadmap", 15)]


def _explore_on_host(oracle, f, s, us):
    case = f.scene_case(s)
    b, n_tebs, best = renew_on_host(oracle, case, slots=8)
    o = oracle.explore_candidates(f.cfg, f.tables[s], b, n_tebs, best, case["start"], case["goal"], unit_samples=us[s], max_paths=f.max_paths,
                                  dist_to_obst=f.dist_to_obst, initial_plan=case["initial_plan"], via_enabled=kept_via_flags(oracle, case, b.count))
    return case, n_tebs, best, o


def _paths(adjacency, limit):
    """GraphSearchInterface::DepthFirst in the reference's order: the first `limit` start-goal paths"""
    goal, out = len(adjacency) - 1, []

    def rec(visited):
        if len(out) >= limit:
            return
        back = visited[-1]
        if goal in adjacency[back]:
            out.append(visited + [goal])
        for w in adjacency[back]:
            if w in visited or w == goal:
                continue
            rec(visited + [w])
    rec([0])
    return out[:limit]


def _margin(mode, thr, a, b):
    """distance of the decision a.isEqual(b) from h_signature_threshold (h_signature.h:196-204, 360-377)"""
    if mode == 2:
        return np.abs(np.abs(np.asarray(b) - np.asarray(a)) - thr).min()
    return min(np.abs(np.abs(a) - thr).min(initial=1.0), np.abs(np.abs(b) - thr).min(initial=1.0))


@pytest.mark.parametrize("kind", ["points", "mixed"])
@pytest.mark.parametrize("dynamic", [True, False])
@pytest.mark.parametrize("graph,samples", GRAPHS)
def test_fixtures_hold_what_the_device_tests_rely_on(oracle, kind, dynamic, graph, samples):
    f = FE.explore_fleet(kind, dynamic, keypoint=(graph == "keypoint"), no_samples=samples, plans_in_class=2)
    us = FE.unit_samples(f)
    mode = 3 if dynamic else 2
    h = f.cfg.hcp
    assert f.n_scenes == 8 and len(f.tables[-1]) == 0 and max(len(t) for t in f.tables) <= 30 and f.batch.n.max() <= 40
    assert (np.diff(f.scene_of) < 0).any()   # interleaved, unsorted
    if kind == "mixed":
        assert {_abi.OBST_POINT, _abi.OBST_CIRCULAR, _abi.OBST_LINE, _abi.OBST_PILL, _abi.OBST_POLYGON} <= set(int(t) for tab in f.tables for t in tab.type)
    gained, examined, N = {}, {}, {}
    for s in range(f.n_scenes):
        case, n_tebs, best, o = _explore_on_host(oracle, f, s, us)
        gained[s], examined[s], N[s] = o["n_total"] - n_tebs, o["n_paths"], len(o["vertices"])
        # every class decision among the existing bands and the examined candidates keeps MARGIN from the threshold
        sigs = []
        if n_tebs:
            kept = _abi.TebBatchHost(n_tebs, f.batch.stride)
            for k in range(n_tebs):
                kept.set_teb(k, *o["batch"].get_teb(k))
            sigs += list(oracle.h_signatures(f.cfg, f.tables[s], kept, mode, h.h_signature_prescaler))
        c = f.cfg
        for path in _paths(o["adjacency"], o["n_paths"]):
            px, py = o["vertices"][path, 0], o["vertices"][path, 1]
            band = oracle.init_trajectory_path(px, py, c.robot.max_vel_x, c.robot.max_vel_theta, c.robot.acc_lim_x, case["start"][2], case["goal"][2],
                                               c.trajectory.min_samples, c.trajectory.allow_init_with_backwards_motion)
            one = _abi.TebBatchHost(1, 64)
            one.set_teb(0, *band)
            sigs.append(oracle.h_signatures(f.cfg, f.tables[s], one, mode, h.h_signature_prescaler)[0])
        for i in range(len(sigs)):
            for j in range(i):
                if len(sigs[i]):
                    assert _margin(mode, h.h_signature_threshold, sigs[i], sigs[j]) >= MARGIN, (s, i, j)
    # what is stated about the scenes
    assert gained[FE.FULL] == 0 and N[FE.FULL] == 0 and len(f.bands_of(FE.FULL)) == h.max_number_classes
    assert gained[FE.LINE] == 1 and N[FE.LINE] == 0 and gained[FE.AT_GOAL] == 0 and N[FE.AT_GOAL] == 0
    assert sum(g >= 2 for g in gained.values()) >= 2, gained
    assert gained[FE.PLAN_NEW] >= 1
    if graph == "keypoint":
        for s, n in FE.KEYPOINT_VERTICES.items():
            assert N[s] == n, (s, N[s])
        assert gained[FE.EMPTY] == 1 and examined[FE.EMPTY] == 1
    else:
        assert all(N[s] == samples + 2 for s in (FE.PLAIN, FE.BEST, FE.PLAN_NEW, FE.PLAN_OLD, FE.EMPTY))
        # one class, cut by max_paths inside its fourth round of QUOTA paths while other scenes finish in their first
        assert gained[FE.EMPTY] == 1 and examined[FE.EMPTY] == f.max_paths > 2 * FE.QUOTA
        assert any(0 < examined[s] <= FE.QUOTA for s in (FE.PLAIN, FE.BEST, FE.PLAN_NEW, FE.PLAN_OLD))


@pytest.mark.parametrize("plans_in_class,kept", [(1, 2), (2, 3)])
def test_best_scene_keeps_two_plans_of_the_best_class_when_allowed(oracle, plans_in_class, kept):
    f = FE.explore_fleet(plans_in_class=plans_in_class)
    _, n_tebs, best = renew_on_host(oracle, f.scene_case(FE.BEST), slots=8)
    assert (n_tebs, best) == (kept, 0)


@pytest.mark.parametrize("all_candidates", [True, False])
def test_plan_scenes_cover_the_via_point_rule(oracle, all_candidates):
    f = FE.explore_fleet(viapoints_all_candidates=all_candidates, keypoint=True)
    us = FE.unit_samples(f)
    _, n_new, _, o_new = _explore_on_host(oracle, f, FE.PLAN_NEW, us)
    _, n_old, _, o_old = _explore_on_host(oracle, f, FE.PLAN_OLD, us)
    assert o_new["initial_plan_teb"] == n_new == 1      # the plan's class is new: its band is appended after the kept one
    assert o_old["initial_plan_teb"] == 0 and n_old == 1   # present already: the existing band stands for it
    ve_new, ve_old = o_new["via_enabled"][:o_new["n_total"]], o_old["via_enabled"][:o_old["n_total"]]
    if all_candidates:
        assert ve_new.all() and ve_old.all()
    else:
        assert list(ve_new[:2]) == [0, 1] and ve_old[0] == 1 and not ve_old[1:].any()
