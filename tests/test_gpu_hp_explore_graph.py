"""The exploration graph of the device (graph_vertices on the host, graph_edges_kernel / graph_edges_fleet_kernel: csrc/teb_graph.hpp,
csrc/teb_hcp_host.hpp) against the fixtures of tests/golden/make_hp_explore_graph.py: the op-by-op fp64 restatement of createGraph,
checked at 80 digits and against the reference planner's own binary, on scenes built ON the thresholds of every decision
(tests/explore_graph_cases.py; what the cases cover is asserted on the CPU in tests/test_hp_explore_graph.py).

This file reads only the fixtures. Every case runs through explore_candidates + exploration_graph on a single-scene handle with the
fixture's unit samples, and through explore_candidates_per_scene + exploration_graph_per_scene as a scene set of one with the handle's
own generator; the two fleets run their four scenes in one launch beside the single-scene handles:
  * adjacency: byte-equal;
  * key-point vertices, and roadmap vertices whose frame is exact in libm (start -> goal along +x): bit-equal;
  * roadmap vertices of the one oblique frame (host libm): <= 4 ulp, the observed distance printed; the fixture says that every decision
    of that case is separated by >= 1e-9 or exact;
  * n_vertices, and n_paths under the case's bound; one case under two bounds of the enumeration: the same graph.
"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import hp_explore_graph as HG  # noqa: E402  (unpack, ulp_distance, the class ids: no mpmath needed)

from teb_local_planner_amd import _abi, planner  # noqa: E402
from teb_local_planner_amd.config import TebConfig  # noqa: E402

pytestmark = pytest.mark.gpu

FAMILIES = ["fwd", "head", "front", "disc", "seg", "lanes", "table", "fleet"]
SINGLE = dict(generic_config_path=True, multi_cu=-1, speculative_trials=-1)   # the fleet contract of include/teb_amd.h
ULP_BOUND = 4
_FIX = {}


def _family(fam):
    if fam not in _FIX:
        _FIX[fam] = HG.unpack(np.load(os.path.join(HERE, "golden", "hp_explore_graph_%s.npz" % fam)))
    return _FIX[fam]


def _names():
    return [(fam, n) for fam in FAMILIES for n in _family(fam)]


def _table(fx):
    ob = _abi.ObstacleTable()
    for o, ty in enumerate(fx["ob_type"]):
        ax, ay, bx, by, r = (float(v) for v in fx["ob_rows"][o])
        verts = None
        if ty == _abi.OBST_POLYGON:
            verts = [tuple(v) for v in fx["ob_verts"][fx["ob_voff"][o]:fx["ob_voff"][o + 1]]]
        ob._add(int(ty), ax, ay, bx, by, r, verts=verts)
    return ob


def _config(fx, max_classes=None):
    keypoint, dist_to_obst, thr, no_samples, width, scale, tol, mc, mp = fx["params"]
    cfg = TebConfig()
    h = cfg.hcp
    h.simple_exploration = bool(keypoint)
    h.obstacle_heading_threshold = float(thr)
    h.roadmap_graph_no_samples = int(no_samples)
    h.roadmap_graph_area_width = float(width)
    h.roadmap_graph_area_length_scale = float(scale)
    h.max_number_classes = int(mc) if max_classes is None else max_classes
    cfg.goal_tolerance.xy_goal_tolerance = float(tol)
    return cfg, float(dist_to_obst), int(mp)


def _solver(cfg, tables, max_tebs):
    mo = max(sum(len(t) for t in tables), 1)
    mv = max(sum(len(t.vert_x) for t in tables), 1)
    return planner.TebBatchSolver(cfg, max_tebs, 256, mo, mv, 1, options=_abi.Options(**SINGLE))


def _check(name, fx, V, A, n_vertices, n_paths, max_paths, what):
    N = len(fx["vertices"])
    assert n_vertices == N == len(V), (name, what)
    assert n_paths <= max_paths, (name, what, n_paths)
    if N == 0:
        return
    np.testing.assert_array_equal(A, fx["adjacency"], err_msg="%s, %s: adjacency" % (name, what))
    if int(fx["libm_exact"][0]):
        np.testing.assert_array_equal(V, fx["vertices"], err_msg="%s, %s: vertices" % (name, what))
    else:
        assert not (fx["rec_class"] == HG.RUNG).any() and (fx["rec_margin"][fx["rec_class"] == HG.SEPARATED] >= HG.REL).all(), name
        d = int(HG.ulp_distance(V, fx["vertices"]).max())
        print("%s, %s: roadmap vertices within %d ulp of the fixture (bound %d)" % (name, what, d, ULP_BOUND))
        assert d <= ULP_BOUND, (name, what, d)


def _single(name, fx, max_classes=None, max_paths=None, units=True):
    cfg, dist_to_obst, mp = _config(fx, max_classes)
    mp = mp if max_paths is None else max_paths
    ob = _table(fx)
    s = _solver(cfg, [ob], max(cfg.hcp.max_number_classes, 1))
    s.set_obstacles(ob)
    s.set_via_points([])
    us = fx["units"] if units and len(fx["units"]) else None
    r = s.explore_candidates(list(fx["start"]), list(fx["goal"]), dist_to_obst=dist_to_obst, unit_samples=us, max_paths=mp)
    V, A = s.exploration_graph()
    s.close()
    return r, V, A, mp


@pytest.mark.parametrize("fam,name", _names())
def test_every_case_single_scene_and_as_a_scene_set_of_one(fam, name):
    fx = _family(fam)[name]
    r, V, A, mp = _single(name, fx)
    _check(name, fx, V, A, r["n_vertices"], r["n_paths"], mp, "single scene")
    # the per-scene forms, the samples from the handle's own generator
    cfg, dist_to_obst, mp = _config(fx)
    ob = _table(fx)
    s = _solver(cfg, [ob], max(cfg.hcp.max_number_classes, 1))
    s.set_scenes([ob], [[]])
    rf = s.explore_candidates_per_scene([list(fx["start"])], [list(fx["goal"])], dist_to_obst, None, False, None, None, mp)
    Vf, Af = s.exploration_graph_per_scene(0)
    s.close()
    _check(name, fx, Vf, Af, int(rf["n_vertices"][0]), int(rf["n_paths"][0]), mp, "scene set of one")
    np.testing.assert_array_equal(Vf, V)
    np.testing.assert_array_equal(Af, A)


@pytest.mark.parametrize("fleet", ["fleetk", "fleetr"])
def test_four_scenes_in_one_launch_equal_their_single_scene_handles(fleet):
    raw = np.load(os.path.join(HERE, "golden", "hp_explore_graph_fleet.npz"))
    members = [str(m) for m in raw["fleet_" + fleet]]
    fxs = [_family("fleet")[m] for m in members]
    for fx in fxs[1:]:   # one launch shares the parameters (but not start, goal, table, samples)
        np.testing.assert_array_equal(fx["params"], fxs[0]["params"])
    cfg, dist_to_obst, mp = _config(fxs[0])
    tables = [_table(fx) for fx in fxs]
    ns = len(members)
    s = _solver(cfg, tables, ns * max(cfg.hcp.max_number_classes, 1))
    s.set_scenes(tables, [[] for _ in range(ns)])
    width = 2 * int(fxs[0]["params"][3])
    us = None
    if width:   # a scene that returns before its graph draws nothing: its row is never read
        us = np.stack([fx["units"] if len(fx["units"]) == width else np.zeros(width) for fx in fxs])
    r = s.explore_candidates_per_scene([list(fx["start"]) for fx in fxs], [list(fx["goal"]) for fx in fxs], dist_to_obst, None, False, None, us, mp)
    graphs = [s.exploration_graph_per_scene(k) for k in range(ns)]
    s.close()
    sizes = []
    for k, (m, fx) in enumerate(zip(members, fxs)):
        V, A = graphs[k]
        _check(m, fx, V, A, int(r["n_vertices"][k]), int(r["n_paths"][k]), mp, "scene %d of %s" % (k, fleet))
        r1, V1, A1, _ = _single(m, fx)
        assert r1["n_vertices"] == r["n_vertices"][k] and r1["n_paths"] == r["n_paths"][k] and r1["n_total"] == r["n_bands"][k], m
        np.testing.assert_array_equal(V, V1)
        np.testing.assert_array_equal(A, A1)
        sizes.append((len(V), len(fx["ob_type"])))
    if fleet == "fleetk":
        assert sizes == [(2, 0), (18, 8), (6, 130), (0, 1)]
    else:   # one set of vertices, three tables: a record that read its neighbour's table would give its neighbour's adjacency
        assert [n for n, _ in sizes] == [17, 17, 17, 0]
        for a in range(3):
            np.testing.assert_array_equal(graphs[a][0], graphs[0][0])
            for b in range(a):
                assert not np.array_equal(graphs[a][1], graphs[b][1])


def test_the_graph_does_not_depend_on_the_bounds_of_the_enumeration():
    fx = _family("lanes")["lanes_n16_keypoint"]
    seen = [_single("lanes_n16_keypoint", fx, max_classes=mc, max_paths=mp) for mc, mp in ((1, 8), (3, 64))]
    assert seen[0][0]["n_paths"] <= 8 and seen[1][0]["n_paths"] <= 64 and seen[1][0]["n_total"] > seen[0][0]["n_total"]
    for r, V, A, mp in seen:
        _check("lanes_n16_keypoint", fx, V, A, r["n_vertices"], r["n_paths"], mp, "bounds %d" % mp)
