"""The whole tick per robot class (include/teb_amd.h: teb_amd_explore_candidates_per_class, teb_amd_update_and_prune_per_class,
teb_amd_optimize_batch_per_class, teb_amd_is_trajectory_feasible_per_class) - the part that needs no device: the four calls are declared,
exported and bound; header and DESIGN.md state them; and the fixtures of tests/fleet_class_tick_cases.py discriminate - with the CPU
oracle, every class that is not class 0 owns a scene (a band, a spec) whose result under its own configuration differs from the result
under class 0's, so a launch that read ONE class for the whole fleet is found out by tests/test_gpu_fleet_class_tick.py."""
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.path.insert(0, HERE)
import fleet_class_tick_cases as CT  # noqa: E402
import fleet_explore_cases as FE  # noqa: E402
import fleet_tick_cases as FT  # noqa: E402

from teb_local_planner_amd import _abi, planner  # noqa: E402

ROOT = os.path.dirname(HERE)
CALLS = {"teb_amd_explore_candidates_per_class": 18, "teb_amd_update_and_prune_per_class": 5, "teb_amd_optimize_batch_per_class": 4,
         "teb_amd_is_trajectory_feasible_per_class": 7}
THREADS = min(os.cpu_count() or 1, 16)


def test_calls_are_declared_exported_and_bound():
    src = open(os.path.join(ROOT, "include", "teb_amd.h")).read()
    declared = set(re.findall(r"\b(teb_amd_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", src, flags=re.S)))
    assert set(CALLS) <= declared
    assert "teb_amd_feasibility_spec_t" in src
    L = planner.lib()
    for name, nargs in CALLS.items():
        assert hasattr(L, name), "libteb_amd.so does not export %s" % name
        assert len(getattr(L, name).argtypes) == nargs, name
    # each is its sibling without the arguments that stand for a configuration field
    assert len(L.teb_amd_explore_candidates_per_scene.argtypes) == CALLS["teb_amd_explore_candidates_per_class"] + 1    # dist_to_obst
    assert len(L.teb_amd_update_and_prune_per_scene.argtypes) == CALLS["teb_amd_update_and_prune_per_class"] + 1       # min_samples
    assert len(L.teb_amd_optimize_batch.argtypes or [0] * 7) == CALLS["teb_amd_optimize_batch_per_class"] + 3           # the cost triple
    assert L.teb_amd_abi_version() == 3   # additive
    for name in ("explore_candidates_per_class", "update_and_prune_per_class", "optimize_per_class", "is_trajectory_feasible_per_class"):
        assert callable(getattr(planner.TebBatchSolver, name))
    # valid only while scenes are set: a null handle is refused before anything else
    assert L.teb_amd_optimize_batch_per_class(None, 1, 1, 1) == _abi.ERR_INVALID_ARG
    assert L.teb_amd_update_and_prune_per_class(None, None, None, None, None) == _abi.ERR_INVALID_ARG


def test_header_and_design_state_the_calls():
    src = open(os.path.join(ROOT, "include", "teb_amd.h")).read()
    fleet = src[src.index("Fleet batches: the bands of many scenes"):]
    for name in CALLS:
        assert name in fleet, name
    assert "teb_amd_is_trajectory_feasible_per_scene keeps its one footprint" in fleet   # still true
    assert "teb_amd_explore_candidates_per_class takes its place" in fleet
    assert "the library cannot check this" not in src
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for name in CALLS:
        assert name in design, name
    # section 8 no longer lists the four limits as open
    assert "exploration, pruning, feasibility and band costs per class" not in design[design.index("## 8"):] or \
        "closed" in design[design.index("## 8"):]
    assert "homogeneous fleet on ONE handle" not in (planner.FleetHomotopyClassPlanner.__doc__ or "")


# ---- exploration -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dynamic", [True, False])
@pytest.mark.parametrize("graph", ["keypoint", "roadmap"])
def test_exploration_fixture_discriminates_the_classes(oracle, graph, dynamic):
    f = FE.explore_fleet("points", dynamic, keypoint=(graph == "keypoint"), plans_in_class=2, viapoints_all_candidates=False)
    us = FE.unit_samples(f)
    cfgs = CT.explore_classes(f.cfg)
    assert len(cfgs) == 3 and sorted(set(CT.EXPLORE_CLASS_OF)) == [0, 1, 2] and len(CT.EXPLORE_CLASS_OF) == f.n_scenes
    assert [c.obstacles.min_obstacle_dist for c in cfgs] == [FE.DIST_TO_OBST, 0.35, 0.1]
    for field in (lambda c: c.robot.max_vel_x, lambda c: c.robot.max_vel_theta, lambda c: c.robot.acc_lim_x):
        assert len({field(c) for c in cfgs}) == 3
    assert [c.trajectory.min_samples for c in cfgs] == [3, 3, 12] and [c.optim.weight_viapoint > 0 for c in cfgs] == [True, True, False]
    assert CT.EXPLORE_CLASS_OF[FE.PLAN_NEW] == 2 and f.vias[FE.PLAN_NEW] and f.plans[FE.PLAN_NEW] is not None
    handle = CT.explore_handle_config(cfgs)
    for c in cfgs:   # a launch that read the handle's configuration would be found out as well
        assert handle.obstacles.min_obstacle_dist != c.obstacles.min_obstacle_dist and handle.robot.max_vel_x != c.robot.max_vel_x
        assert handle.trajectory.min_samples != c.trajectory.min_samples and handle.optim.weight_viapoint != c.optim.weight_viapoint
        assert handle.robot.acc_lim_x != c.robot.acc_lim_x and handle.robot.max_vel_theta != c.robot.max_vel_theta
    own, differs = {}, {1: [], 2: []}
    for s in range(f.n_scenes):
        k = CT.EXPLORE_CLASS_OF[s]
        own[s] = CT.explore_on_host(oracle, f, cfgs[k], s, us)
        if k != 0:
            _, under0 = CT.explore_on_host(oracle, f, cfgs[0], s, us)
            if not CT.same_exploration(own[s][1], under0):
                differs[k].append(s)
    assert differs[1] and differs[2], differs
    # every scene kind still reaches what its name says
    n0 = {s: own[s][0] for s in own}
    o = {s: own[s][1] for s in own}
    assert o[FE.PLAIN]["n_total"] >= 3 and n0[FE.PLAIN] == 0                                  # gains several classes
    assert o[FE.FULL]["n_total"] == n0[FE.FULL] == 4 and len(o[FE.FULL]["vertices"]) == 0     # full: untouched, draws nothing
    assert n0[FE.LINE] == 0 and o[FE.LINE]["n_total"] == 1 and len(o[FE.LINE]["vertices"]) == 0   # the line band
    assert o[FE.AT_GOAL]["n_total"] == n0[FE.AT_GOAL] == 1                                    # at its goal with a band: nothing
    assert n0[FE.BEST] == 3                                                                   # both `up` bands survive the filter
    assert o[FE.PLAN_NEW]["initial_plan_teb"] == 1 and o[FE.PLAN_NEW]["n_total"] == 2         # the plan is a new class
    assert o[FE.PLAN_OLD]["initial_plan_teb"] == 0 and o[FE.PLAN_OLD]["n_total"] > n0[FE.PLAN_OLD] == 1   # its class is present
    assert o[FE.EMPTY]["n_total"] == 1 and o[FE.EMPTY]["n_paths"] == (1 if graph == "keypoint" else f.max_paths)
    # min_samples: the line band and the short paths of the class with 12 are padded to 12 poses, those of the others are not
    assert int(o[FE.LINE]["batch"].n[0]) == 12 and all(int(n) == 12 for n in o[FE.PLAIN]["batch"].n[:o[FE.PLAIN]["n_total"]])
    assert int(o[FE.EMPTY]["batch"].n[0]) == 3
    # weight_viapoint: with the weight the band of the initial plan alone follows the via-points; without it no flag moves
    np.testing.assert_array_equal(o[FE.PLAN_NEW]["via_enabled"][:2], [1, 0])
    np.testing.assert_array_equal(CT.explore_on_host(oracle, f, cfgs[0], FE.PLAN_NEW, us)[1]["via_enabled"][:2], [0, 1])
    assert o[FE.PLAN_OLD]["via_enabled"][0] == 1 and not o[FE.PLAN_OLD]["via_enabled"][1:o[FE.PLAN_OLD]["n_total"]].any()


# ---- costs -------------------------------------------------------------------------------------------------------------------------
def test_cost_fixture_discriminates_the_classes(oracle):
    cf = CT.cost_classed_fleet()
    f = cf.fleet
    triples = [(c.hcp.selection_obst_cost_scale, c.hcp.selection_viapoint_cost_scale, bool(c.hcp.selection_alternative_time_cost)) for c in cf.cfgs]
    assert len(set(triples)) >= 3 and any(t[2] for t in triples)
    t0 = triples[0]
    seen = set()
    via_scaled = False
    for s in range(f.n_scenes):
        k = cf.class_of[s]
        if k == 0:
            continue
        cfg = cf.cfg_of_scene(s)
        sub, idx = f.scene_batch(s)
        _, own = oracle.optimize_batch(cfg, f.tables[s], f.vias[s], sub, threads=THREADS)
        _, as0 = oracle.optimize_batch(cfg, f.tables[s], f.vias[s], sub, obst_cost_scale=t0[0], viapoint_cost_scale=t0[1], alternative_time_cost=t0[2],
                                       threads=THREADS)
        assert (own.status == _abi.TEB_OK).all()
        if (own.cost != as0.cost).any():
            seen.add(k)
        if triples[k][1] != 1 and f.vias[s] and cfg.optim.weight_viapoint != 0:
            _, unscaled = oracle.optimize_batch(cfg, f.tables[s], f.vias[s], sub, viapoint_cost_scale=1.0, threads=THREADS)
            via_scaled = via_scaled or bool((own.cost != unscaled.cost).any())
    assert seen == set(range(1, len(cf.cfgs))), seen
    assert via_scaled, "no scene with via-points under a class with selection_viapoint_cost_scale != 1"


# ---- feasibility -------------------------------------------------------------------------------------------------------------------
def test_feasibility_fixture_discriminates_the_specs(oracle):
    f = FT.feasibility_fleet()
    specs = CT.feasibility_specs()
    assert len(specs) == 3 and [len(q["footprint"]) for q in specs] == [4, 3, 1]
    assert CT.spec_args(specs[0])[1:] == FT.FEAS_PARAMS[0] and CT.spec_args(specs[1])[1:] == FT.FEAS_PARAMS[1]
    assert len(CT.FEAS_SPEC_OF) == len(f.grids) and sorted(set(CT.FEAS_SPEC_OF)) == [0, 1, 2]
    differs = set()
    for s, k in enumerate(CT.FEAS_SPEC_OF):
        own = oracle.is_trajectory_feasible(f.batch, int(f.bands[s]), f.grids[s], *CT.spec_args(specs[k]))
        under0 = oracle.is_trajectory_feasible(f.batch, int(f.bands[s]), f.grids[s], *CT.spec_args(specs[0]))
        if own != under0:
            differs.add(k)
    assert differs == {1, 2}, differs


# ---- pruning -----------------------------------------------------------------------------------------------------------------------
def test_prune_fixture_discriminates_the_classes(oracle):
    f = FT.prune_fleet()
    cfgs = CT.prune_classes(f.cfg)
    assert [c.trajectory.min_samples for c in cfgs] == [3, 8] and len(CT.PRUNE_CLASS_OF) == len(FT.PRUNE_COUNTS)
    short = [n for s, poses in enumerate(FT.PRUNE_POSES) if CT.PRUNE_CLASS_OF[s] == 1 for n in poses if 3 <= n <= 6]
    assert short, "no band of 3 to 6 poses under the class with the larger min_samples"
    differs = 0
    for b in range(f.batch.count):
        s = int(f.scene_of[b])
        if CT.PRUNE_CLASS_OF[s] != 1:
            continue
        own = oracle.update_and_prune(*f.batch.get_teb(b), f.starts[s], f.goals[s], 8)
        under0 = oracle.update_and_prune(*f.batch.get_teb(b), f.starts[s], f.goals[s], 3)
        differs += len(own[0]) != len(under0[0])
    assert differs >= 1, "min_samples never changes what updateAndPruneTEB deletes"
