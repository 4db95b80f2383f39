"""PINS the oracle against the reference's OWN code (oracle/_ref/libteb_ref.so = /root/reference's headers and
src/{obstacles,timed_elastic_band}.cpp compiled in place against stand-in Eigen/g2o/ROS/Boost headers):

  * every computeError() of the 15 edge classes (+ penalties.h, misc.h fast_sigmoid, pose_se2.h) on the oracle's own graph,
  * the two live analytic Jacobians of the reference (EdgeKinematicsDiffDrive, EdgeTimeOptimal),
  * all 5 footprints x 5 obstacle types distances, static and spatio-temporal, and the obstacle centroids,
  * TimedElasticBand::autoResize (incl. the reference's three unit tests run on the reference implementation),
  * the TebConfig() constructor defaults.

  * src/optimal_planner.cpp itself — buildGraph / AddEdges* (edge list, order, vertices, weights, association incl. the legacy
    variant, dynamic-obstacle time stamps), optimizeGraph, computeCurrentCost, the optimizeTEB outer loop — compiled in place and
    driven through a recording stand-in for g2o::SparseOptimizer (oracle/ref_shim/shim_g2o.h): graph records, central-difference
    Jacobians over the reference's computeError, final state / pose count / cost after the full outer x inner loop, all BIT-equal.

Not pinnable (external libg2o absent): the LM iteration, the central-difference scheme and the linear solver are restated in
shim_g2o.h from g2o's sources as described in SURVEY.md Appendix B — by the same author as the oracle's, so the agreement of
those three parts shows consistency, not independent confirmation.
When libteb_ref.so is not available (no /root/reference, no prebuilt file) the same checks run against the committed
golden vectors that tests/golden/make_ref_golden.py produced from it.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
from teb_local_planner_amd import scenes, _abi  # noqa: E402
from teb_local_planner_amd.config import TebConfig  # noqa: E402

sys.path.insert(0, os.path.join(HERE, "golden"))
import make_ref_golden as G  # noqa: E402
import ref_replay  # noqa: E402


def _ref():
    from oracle import ref_py
    if os.environ.get("TEB_REF_GOLDEN_ONLY") or not ref_py.available():
        return None
    try:
        ref_py.lib()
    except Exception:
        return None
    return ref_py


def _ref_results(name):
    """Live reference if it can be loaded, else the committed golden vectors."""
    r = _ref()
    if r is not None:
        return G.compute(name, r), "live"
    g = np.load(os.path.join(HERE, "golden", "ref_%s.npz" % name))
    return {k: g[k] for k in g.files}, "golden"


@pytest.mark.parametrize("name", sorted(G.EDGE_CASES))
def test_edge_residuals_match_reference_classes(oracle, name):
    ref, src = _ref_results(name)
    cfg, obst, via, batch = G.EDGE_CASES[name]()
    k0 = 0
    types_seen = set()
    for b in range(batch.count):
        cfg.jacobian_mode = _abi.JACOBIAN_ANALYTIC
        ir, dr = oracle.edges(cfg, obst, via, batch, b, G.WEIGHT_MULTIPLIER)
        E = len(ir)
        err_ref = ref["err"][k0:k0 + E]; jac_ref = ref["jac"][k0:k0 + E]; jv = ref["jac_valid"][k0:k0 + E]
        np.testing.assert_array_equal(ref["types"][k0:k0 + E], ir[:, 0])
        # residuals: same arithmetic on the same CPU -> bit-identical (allow 2 ulp for libm / evaluation-order freedom)
        np.testing.assert_allclose(dr[:, 0:3], err_ref, rtol=4e-16, atol=1e-300)
        J = dr[:, 8:41].reshape(E, 3, 11)
        sel = jv != 0
        assert sel.any()
        np.testing.assert_allclose(J[sel], jac_ref[sel], rtol=4e-16, atol=0)
        types_seen |= set(ir[:, 0].tolist())
        k0 += E
    assert k0 == len(ref["err"])
    assert types_seen >= G.EXPECTED_TYPES[name], (name, types_seen)


def test_every_edge_class_is_covered():
    seen = set()
    for v in G.EXPECTED_TYPES.values():
        seen |= v
    assert seen == set(range(18))   # all 18 edge kinds of the reference (15 classes + start/goal variants)


@pytest.mark.parametrize("footprint", ["point", "circular", "two_circles", "line", "polygon"])
def test_distances_and_centroids_match_reference(oracle, footprint):
    ref, src = _ref_results("dist_" + footprint)
    cfg, obst, q = G.distance_case(footprint)
    for mode, key in ((None, "d_static"), (q["t"], "d_st")):
        for k in range(len(q["oi"])):
            d, _ = oracle.distance(cfg, obst, int(q["oi"][k]), q["x"][k], q["y"][k], q["th"][k], None if mode is None else mode[k])
            assert abs(d - ref[key][k]) <= 4e-16 * max(1.0, abs(d)), (footprint, k, d, ref[key][k])
    for i in range(len(obst)):
        cx, cy = oracle.centroid(obst, i)
        sel = np.where(q["oi"] == i)[0]
        if len(sel):
            assert cx == ref["cx"][sel[0]] and cy == ref["cy"][sel[0]]


def test_autoresize_matches_reference_implementation(oracle):
    ref, src = _ref_results("autoresize")
    cases = G.autoresize_cases()
    for k, (x, y, th, dt, args) in enumerate(cases):
        X, Y, T, D = oracle.autoresize(x, y, th, dt, *args)
        n = int(ref["n"][k])
        assert len(X) == n
        o = int(ref["off"][k])
        np.testing.assert_array_equal(X, ref["x"][o:o + n]); np.testing.assert_array_equal(Y, ref["y"][o:o + n])
        np.testing.assert_allclose(T, ref["th"][o:o + n], rtol=0, atol=4e-16)
        np.testing.assert_array_equal(D, ref["dt"][o:o + n - 1])


def test_reference_unit_tests_on_reference_implementation():
    """test/teb_basics.cpp:5-67 executed on the reference's TimedElasticBand itself (its recorded outputs without oracle/_ref)."""
    r = ref_replay.reference("unit_tests", 0, _ref())
    dt = 0.1; hyst = dt / 3.
    for last, mid in ((dt + 2 * hyst, None), (dt - 2 * hyst, None), (dt - 2 * hyst, dt + 2 * hyst)):
        d = np.full(10, dt); d[9] = last
        if mid is not None:
            d[5] = mid
        X, Y, T, D = r.autoresize(np.arange(11.0), np.zeros(11), np.zeros(11), d, dt, hyst, 3, 100, False)
        assert np.all(D <= dt + hyst + 1e-3) and np.all(dt - hyst - 1e-3 <= D)


def test_config_defaults_match_reference_constructor():
    ref, src = _ref_results("config")
    mine = TebConfig().to_c()
    from teb_local_planner_amd import planner
    libc = _abi.Config()
    planner.lib().teb_amd_config_default(C.byref(libc))
    for k, (name, _) in enumerate([f for f in _abi.Config._fields_ if not f[0].startswith("footprint") and f[0] != "jacobian_mode"]):
        if name in ("divergence_detection_enable", "divergence_detection_max_chi_squared"):
            continue   # no constructor default in the reference (teb_config.h: only the ROS loaders set them)
        assert getattr(mine, name) == ref["values"][k], name
        assert getattr(libc, name) == ref["values"][k], name


# ---- src/optimal_planner.cpp compiled in place: graph construction and the whole optimizeTEB --------------------------------------

def _oracle_graph_as_ref_records(ir, dr):
    """teb_oracle_edges records -> (type, dim, vertex-id list) in the reference's vertex numbering (pose i: 2i, dt i: 2i+1)."""
    out = []
    for k in range(len(ir)):
        t, npose, p0, p1, p2, nd, d0, d1, dim = [int(v) for v in ir[k][:9]]
        out.append((t, dim, [2 * p for p in (p0, p1, p2)[:npose]] + [2 * d + 1 for d in (d0, d1)[:nd]]))
    return out


@pytest.mark.parametrize("name", sorted(G.PLANNER_CASES))
def test_graph_matches_reference_buildGraph(oracle, name):
    ref, src = _ref_results("graph_" + name)
    cfg, obst, via, batch = G.PLANNER_CASES[name]()
    cfg.jacobian_mode = _abi.JACOBIAN_G2O_NUMERIC
    k0 = 0
    for b in range(min(batch.count, G.MAX_TEBS)):
        ir, dr = oracle.edges(cfg, obst, via, batch, b, G.WEIGHT_MULTIPLIER)
        E = int(ref["count"][b])
        assert len(ir) == E, (name, b)
        rir = ref["irec"][k0:k0 + E]; rdr = ref["drec"][k0:k0 + E]
        n = int(batch.n[b])
        fixed = {0, 2 * (n - 1)}
        for k, (t, dim, verts) in enumerate(_oracle_graph_as_ref_records(ir, dr)):
            assert t == rir[k][0] and dim == rir[k][1] and verts == list(rir[k][3:3 + rir[k][2]]), (name, b, k, ir[k], rir[k])
            np.testing.assert_array_equal(dr[k, :dim], rdr[k, :dim])             # residuals
            np.testing.assert_array_equal(dr[k, 3:3 + dim], rdr[k, 3:3 + dim])   # information = weights (x weight_multiplier)
            Jo = dr[k, 8:41].reshape(3, 11); Jr = rdr[k, 6:48].reshape(3, 14)[:, :11]
            npose = int(ir[k][1])
            for v in range(npose):   # columns of fixed vertices are never linearised by g2o
                if verts[v] in fixed:
                    Jo[:, 3 * v:3 * v + 3] = 0
            np.testing.assert_array_equal(Jo, Jr)
        k0 += E


@pytest.mark.parametrize("name", sorted(G.PLANNER_CASES))
def test_optimizeTEB_matches_reference_optimal_planner(oracle, name):
    """Whole TebOptimalPlanner::optimizeTEB (no_outer x no_inner iterations, autoResize, graph rebuilds, weight adaptation,
    computeCurrentCost): the reference's own src/optimal_planner.cpp vs the oracle in g2o-numeric Jacobian mode. Bit-equal."""
    ref, src = _ref_results("opt_" + name)
    cfg, obst, via, batch = G.PLANNER_CASES[name]()
    cfg.jacobian_mode = _abi.JACOBIAN_G2O_NUMERIC
    nb, res = oracle.optimize_batch(cfg, obst, via, batch, compute_cost=True)
    for b in range(min(batch.count, G.MAX_TEBS)):
        x, y, th, dt = nb.get_teb(b)
        n = int(ref["n"][b])
        assert len(x) == n, (name, b)
        assert bool(ref["success"][b]) == (res.status[b] == _abi.TEB_OK)
        np.testing.assert_array_equal(x, ref["state"][b, 0, :n]); np.testing.assert_array_equal(y, ref["state"][b, 1, :n])
        np.testing.assert_array_equal(th, ref["state"][b, 2, :n]); np.testing.assert_array_equal(dt, ref["state"][b, 3, :n - 1])
        assert res.cost[b] == ref["cost"][b], (name, b, res.cost[b], ref["cost"][b])


def test_reference_default_start_and_goal_velocity_are_fixed_at_zero(oracle):
    """TebOptimalPlanner::initialize() sets vel_start_.first = vel_goal_.first = true with zero twists (src/optimal_planner.cpp:94-102):
    the reference's graph of a freshly initialised planner has an EdgeAccelerationStart and an EdgeAccelerationGoal. The batch
    defaults (and NULL flag arrays in the C-ABI) mean the same."""
    cfg, obst, via, batch = scenes.scene_c1()
    assert batch.has_vel_start[0] == 1 and batch.has_vel_goal[0] == 1
    ir, _ = oracle.edges(cfg, obst, via, batch, 0, 1.0)
    assert (ir[:, 0] == 7).sum() == 1 and (ir[:, 0] == 8).sum() == 1
    r = _ref()
    if r is not None:
        rir, _ = r.build_graph(cfg, obst, via, batch, 0, 1.0)
        assert (rir[:, 0] == 7).sum() == 1 and (rir[:, 0] == 8).sum() == 1


# ---- producers and consumers of the strip, pinned on the reference's TimedElasticBand / planner ------

def _same_band(a, b):
    assert len(a[0]) == len(b[0])
    for u, v in zip(a, b):
        np.testing.assert_array_equal(u, v)


def test_f1_initTrajectoryToGoal_line_matches_reference(oracle):
    ref, src = _ref_results("f1_init_line")
    for k, c in enumerate(G.init_line_cases()):
        _same_band(oracle.init_trajectory_line(*c), G.unpack(ref, k))


def test_f1_initTrajectoryToGoal_plan_matches_reference(oracle):
    ref, src = _ref_results("f1_init_plan")
    o = 0
    for k, c in enumerate(G.init_plan_cases()):
        seen = ref["yaw_seen"][o:o + len(c[0])]; o += len(c[0])   # the plan reaches the reference as quaternions
        np.testing.assert_allclose(seen, c[2], rtol=0, atol=1e-15)
        _same_band(oracle.init_trajectory_plan(c[0], c[1], seen, *c[3:]), G.unpack(ref, k))


def test_f1_initTrajectoryToGoal_path_template_matches_reference(oracle):
    ref, src = _ref_results("f1_init_path")
    for k, c in enumerate(G.init_path_cases()):
        _same_band(oracle.init_trajectory_path(*c), G.unpack(ref, k))


def test_f1_updateAndPruneTEB_matches_reference(oracle):
    ref, src = _ref_results("f1_prune")
    pruned = 0
    for k, c in enumerate(G.prune_cases()):
        out = oracle.update_and_prune(*c)
        _same_band(out, G.unpack(ref, k))
        pruned += len(out[0]) < len(c[0])
    assert pruned >= 5


def test_f2_velocity_command_profile_and_trajectory_match_reference(oracle):
    ref, src = _ref_results("f2_consumers")
    po = to = 0
    for k, c in enumerate(G.consumer_cases()):
        r = oracle.consumers(*c)
        n = int(c[1].n[c[2]])
        assert r["ok"] == bool(ref["ok"][k])
        np.testing.assert_array_equal(r["cmd"], ref["cmd"][k])
        np.testing.assert_array_equal(r["profile"], ref["profile"][po:po + n + 1]); po += n + 1
        t = ref["trajectory"][to:to + n]; to += n
        np.testing.assert_array_equal(r["trajectory"][:, [0, 1, 3, 4, 5, 6]], t[:, [0, 1, 3, 4, 5, 6]])
        np.testing.assert_allclose(r["trajectory"][:, 2], t[:, 2], rtol=0, atol=1e-15)   # yaw went through a quaternion in the reference


# ---- SURVEY section 8(f) row f3, arithmetic core: H-signatures (h_signature.h) ------------------------------------------------------

def _class_list(equal, valid):
    """renewAndAnalyzeOldTebs without a best TEB, driven by the REFERENCE's isEqual / isValid results."""
    cls, keep = [], np.zeros(len(valid), np.int32)
    for b in range(len(valid)):
        if valid[b] and not any(equal[b, c] for c in cls):
            cls.append(b); keep[b] = 1
    return keep


@pytest.mark.parametrize("mode", [2, 3])
def test_f3_h_signatures_and_equivalence_match_reference(oracle, mode):
    ref, src = _ref_results("f3_hsig_%dd" % mode)
    classes_seen = 0
    for cname, cfg, obst, batch in G.h_signature_cases():
        sig = oracle.h_signatures(cfg, obst, batch, mode, 1.0)
        np.testing.assert_array_equal(sig, ref[cname + "_sig"])          # long double (2-D) / double (3-D) like the reference: bit-equal
        keep, valid, reas = oracle.filter_equivalence_classes(mode, sig, 0.1, -1, 1)
        np.testing.assert_array_equal(valid, ref[cname + "_valid"])
        np.testing.assert_array_equal(reas, ref[cname + "_reasonable"])
        np.testing.assert_array_equal(keep, _class_list(ref[cname + "_equal"], ref[cname + "_valid"]))
        classes_seen = max(classes_seen, int(keep.sum()))
    assert classes_seen >= 3


@pytest.mark.parametrize("seed", range(40))
def test_f1_f2_randomized_strip_functions_are_bit_equal_to_reference_code(oracle, seed):
    """Random start / goal / plan / path / pruning / read-out inputs: the oracle's initTrajectoryToGoal x3, updateAndPruneTEB,
    getVelocityCommand / Profile / FullTrajectory against the reference's own code (its recorded outputs without oracle/_ref)."""
    from random_strip_cases import random_strip_case, band_for_readout
    r = ref_replay.reference("f1_f2", seed, _ref())
    c = random_strip_case(seed)
    _same_band(oracle.init_trajectory_line(*c["line"]), r.init_trajectory_line(*c["line"]))
    ref_band, yaw_seen = r.init_trajectory_plan(*c["plan"])
    px, py, _, *rest = c["plan"]
    _same_band(oracle.init_trajectory_plan(px, py, yaw_seen, *rest), ref_band)      # yaw as read back from the pose messages
    _same_band(oracle.init_trajectory_path(*c["path"]), r.init_trajectory_path(*c["path"]))
    b = band_for_readout(oracle, c)
    band = b.get_teb(0)
    if len(band[0]) >= c["prune"][2]:
        _same_band(oracle.update_and_prune(*band, *c["prune"]), r.update_and_prune(*band, *c["prune"]))
    la, prevent, _, _ = c["consumer"]
    want = r.consumers(c["cfg"], b, 0, la, prevent)
    got = oracle.consumers(c["cfg"], b, 0, la, prevent)
    assert got["ok"] == want["ok"]
    np.testing.assert_array_equal(got["cmd"], want["cmd"]); np.testing.assert_array_equal(got["profile"], want["profile"])
    np.testing.assert_array_equal(got["trajectory"][:, [0, 1, 3, 4, 5, 6]], want["trajectory"][:, [0, 1, 3, 4, 5, 6]])
    np.testing.assert_allclose(got["trajectory"][:, 2], want["trajectory"][:, 2], rtol=0, atol=1e-15)   # yaw went through a quaternion in the reference


# ---- SURVEY section 8(f) row f3, candidate generation: graph_search.cpp + addAndInitNewTeb -----------------------------------------

def renew_on_host(oracle, case, slots=None):
    """renewAndAnalyzeOldTebs on the existing bands with the oracle's signature / filter functions: (batch with `slots` slots holding the
    kept bands in the reference's order, n_tebs, best)."""
    cfg, obst, batch, best = case["cfg"], case["obst"], case["batch"], case["best"]
    slots = slots or cfg.hcp.max_number_classes + (batch.count if batch is not None else 0)
    stride = batch.stride if batch is not None else 256
    out = _abi.TebBatchHost(slots, stride)
    if batch is None:
        return out, 0, -1
    mode = 3 if cfg.obstacles.include_dynamic_obstacles else 2
    sig = oracle.h_signatures(cfg, obst, batch, mode, cfg.hcp.h_signature_prescaler)
    keep, _, _ = oracle.filter_equivalence_classes(mode, sig, cfg.hcp.h_signature_threshold, best, cfg.hcp.max_number_plans_in_current_class)
    if cfg.hcp.delete_detours_backwards:
        opt = case.get("optimized") or [1] * batch.count
        keep = oracle.filter_detours(cfg, batch, keep, best, opt)
    order = list(range(batch.count))
    if best >= 0:
        order[0], order[best] = order[best], order[0]
    kept = [b for b in order if keep[b]]
    for k, b in enumerate(kept):
        out.set_teb(k, *batch.get_teb(b))
    return out, len(kept), (0 if best >= 0 and keep[best] else -1)


def kept_via_flags(oracle, case, slots):
    """via-point flags of the existing bands after renewAndAnalyzeOldTebs (they travel with their band), padded to `slots`."""
    if not case.get("via"):
        return None
    flags = np.zeros(slots, np.int32)
    if case["batch"] is not None:
        given = case.get("via_enabled") or [1] * case["batch"].count
        kept, n_tebs, _ = renew_on_host(oracle, case)
        for k in range(n_tebs):
            for j in range(case["batch"].count):
                a, c = kept.get_teb(k), case["batch"].get_teb(j)
                if len(a[0]) == len(c[0]) and np.array_equal(a[1], c[1]) and np.array_equal(a[3], c[3]):
                    flags[k] = given[j]
    return flags


def plan_as_seen(case, ref):
    """The initial plan with the yaw angles the reference reads back from the pose messages (yaw -> quaternion -> tf::getYaw)."""
    if case.get("initial_plan") is None:
        return None
    px, py, _ = case["initial_plan"]
    return px, py, ref["plan_yaw_seen"]


def stale_signature(oracle, case, key="stale_band"):
    """Signature of case[key] (the class of a best / initial-plan band that no longer exists), or None."""
    if case.get(key) is None:
        return None
    cfg = case["cfg"]
    b = _abi.TebBatchHost(1, 256)
    b.set_teb(0, *case[key])
    return oracle.h_signatures(cfg, case["obst"], b, 3 if cfg.obstacles.include_dynamic_obstacles else 2, cfg.hcp.h_signature_prescaler)[0]


@pytest.mark.parametrize("name", sorted(G.explore_cases()))
def test_f3_candidate_generation_matches_reference_graph_search(oracle, name):
    """createGraph (both graph types), DepthFirst and addAndInitNewTeb: vertices, edges and every resulting band bit-equal to the
    reference's own src/graph_search.cpp / homotopy_class_planner.hpp run on the same inputs."""
    case = G.explore_cases()[name]
    r = _ref()
    ref = G.explore_reference(r, case) if r is not None else None
    if ref is None:
        g = np.load(os.path.join(HERE, "golden", "ref_f3_explore.npz"))
        ref = {k[len(name) + 2:]: g[k] for k in g.files if k.startswith(name + "__")}
    b, n_tebs, best = renew_on_host(oracle, case)
    o = oracle.explore_candidates(case["cfg"], case["obst"], b, n_tebs, best, case["start"], case["goal"], skip_draws=case.get("skip_draws", 0),
                                  dist_to_obst=case.get("dist_to_obst"), stale_best_sig=stale_signature(oracle, case),
                                  initial_plan=plan_as_seen(case, ref), stale_initial_sig=stale_signature(oracle, case, "stale_initial_band"),
                                  via_enabled=kept_via_flags(oracle, case, b.count))
    assert o["n_total"] == int(ref["n_total"])
    assert o["initial_plan_teb"] == int(ref["initial_plan_teb"])
    if case.get("via"):
        np.testing.assert_array_equal(o["via_enabled"][:o["n_total"]], ref["via_enabled"])
    np.testing.assert_array_equal(o["vertices"], ref["vertices"])
    N = len(o["vertices"])
    adj = np.zeros((N, N), np.uint8)
    for i, row in enumerate(o["adjacency"]):
        adj[i, row] = 1
    np.testing.assert_array_equal(adj, ref["adjacency"])
    for k in range(o["n_total"]):
        for a, e in zip(o["batch"].get_teb(k), G.unpack(ref, k)):
            np.testing.assert_array_equal(a, e)


def test_f3_candidate_cases_cover_both_graphs_and_find_several_classes(oracle):
    seen = {}
    for name, case in G.explore_cases().items():
        b, n_tebs, best = renew_on_host(oracle, case)
        o = oracle.explore_candidates(case["cfg"], case["obst"], b, n_tebs, best, case["start"], case["goal"], skip_draws=case.get("skip_draws", 0),
                                  dist_to_obst=case.get("dist_to_obst"))
        seen[name] = (n_tebs, o["n_total"], o["n_paths"])
    assert seen["keypoint_12_obstacles"][1] >= 5 and seen["roadmap_points_3d"][1] >= 3
    assert seen["goal_reached_line_init"] == (0, 1, 0) and seen["already_full"][1] == seen["already_full"][0] == 2
    assert seen["roadmap_existing_tebs_best"][0] == 4          # 5 bands in 3 classes, 2 allowed in the best band's class
    assert seen["max_two_classes"][1] == 2
    assert seen["stale_best_class_2d"][1] == 3 and seen["stale_best_class_3d"][1] == 3     # without the left-over class: 3 classes ...
    for name in ("stale_best_class_2d", "stale_best_class_3d"):                            # ... with it: two more plans in that class
        case = G.explore_cases()[name]
        b, n_tebs, best = renew_on_host(oracle, case)
        o = oracle.explore_candidates(case["cfg"], case["obst"], b, n_tebs, best, case["start"], case["goal"],
                                      stale_best_sig=stale_signature(oracle, case))
        assert o["n_total"] == 5
    # deletePlansDetouringBackwards: the backwards start (1), the 5x longer plan (2) and the not-optimised plan (3) go, each by its own rule
    case = G.explore_cases()["detours_existing_tebs"]
    ones = np.ones(6, np.int32)
    np.testing.assert_array_equal(oracle.filter_detours(case["cfg"], case["batch"], ones, 0, case["optimized"]), [1, 0, 0, 0, 1, 1])
    np.testing.assert_array_equal(oracle.filter_detours(case["cfg"], case["batch"], ones, 0, [1] * 6), [1, 0, 0, 1, 1, 1])
    np.testing.assert_array_equal(oracle.filter_detours(case["cfg"], case["batch"], ones, -1, [1] * 6), ones)          # no best band yet
    np.testing.assert_array_equal(oracle.filter_detours(G.explore_cases()["detours_best_too_short"]["cfg"], case["batch"], ones, 0, [1] * 6), ones)


@pytest.mark.parametrize("seed", range(40))
def test_f3_randomized_candidate_generation_is_bit_equal_to_reference_code(oracle, seed):
    """Random scenes (every obstacle class, both graphs, random parameters, optional initial plan): graph, bands, getInitialPlanTEB index
    and via-point flags of the oracle against the reference's own code run on the same inputs (its recorded outputs without oracle/_ref)."""
    from random_explore_cases import random_explore_case
    r = ref_replay.reference("f3_explore", seed, _ref())
    case = random_explore_case(seed)
    ref = G.explore_reference(r, case)
    b, n_tebs, best = renew_on_host(oracle, case, slots=16)
    o = oracle.explore_candidates(case["cfg"], case["obst"], b, n_tebs, best, case["start"], case["goal"], dist_to_obst=case.get("dist_to_obst"),
                                  initial_plan=plan_as_seen(case, ref), via_enabled=kept_via_flags(oracle, case, b.count), max_paths=20000)
    if o["n_paths"] >= 20000:
        pytest.skip("path enumeration bounded")
    assert o["n_total"] == int(ref["n_total"]) and o["initial_plan_teb"] == int(ref["initial_plan_teb"])
    np.testing.assert_array_equal(o["vertices"], ref["vertices"])
    N = len(o["vertices"])
    adj = np.zeros((N, N), np.uint8)
    for i, row in enumerate(o["adjacency"]):
        adj[i, row] = 1
    np.testing.assert_array_equal(adj, ref["adjacency"])
    for k in range(o["n_total"]):
        for a, e in zip(o["batch"].get_teb(k), G.unpack(ref, k)):
            np.testing.assert_array_equal(a, e)
    if case.get("via"):
        np.testing.assert_array_equal(o["via_enabled"][:o["n_total"]], ref["via_enabled"])


@pytest.mark.parametrize("seed", range(0, 80, 4))
@pytest.mark.parametrize("mode", [2, 3])
def test_f3_randomized_h_signatures_are_bit_equal_to_reference_code(oracle, mode, seed):
    """Random scenes of the optimiser tests (every obstacle class, moving obstacles, ragged bands): both signature classes, isValid,
    isReasonable and the pairwise isEqual of the reference against the oracle's values and class list (its recorded outputs without
    oracle/_ref)."""
    from random_cases import random_case
    r = ref_replay.reference("f3_hsig", "%d_%d" % (mode, seed), _ref())
    cfg, obst, via, batch = random_case(seed)
    want = r.h_signatures(cfg, obst, batch, mode, 1.0, 0.1)
    sig = oracle.h_signatures(cfg, obst, batch, mode, 1.0)
    np.testing.assert_array_equal(sig, want["sig"])
    keep, valid, reas = oracle.filter_equivalence_classes(mode, sig, 0.1, -1, 1)
    np.testing.assert_array_equal(valid, want["valid"]); np.testing.assert_array_equal(reas, want["reasonable"])
    np.testing.assert_array_equal(keep, _class_list(want["equal"], want["valid"]))


# ---- randomised pin: every option toggled at random, whole optimizeTEB, oracle vs the reference's src/optimal_planner.cpp ----------
@pytest.mark.parametrize("seed", range(40))
def test_randomized_optimizeTEB_is_bit_equal_to_reference_code(oracle, seed):
    r = ref_replay.reference("optimize_teb", seed, _ref())      # (its recorded outputs without oracle/_ref)
    sys.path.insert(0, HERE)
    from random_cases import random_case
    cfg, obst, via, batch = random_case(seed)
    cfg.jacobian_mode = _abi.JACOBIAN_G2O_NUMERIC
    nb, res = oracle.optimize_batch(cfg, obst, via, batch, compute_cost=True)
    for b in range(batch.count):
        ref = r.optimize_teb(cfg, obst, via, batch, b)
        x, y, th, dt = nb.get_teb(b)
        assert len(x) == len(ref["x"]) and ref["success"] == (res.status[b] == _abi.TEB_OK), (seed, b)
        np.testing.assert_array_equal(x, ref["x"]); np.testing.assert_array_equal(y, ref["y"])
        np.testing.assert_array_equal(th, ref["theta"]); np.testing.assert_array_equal(dt, ref["dt"])
        assert res.cost[b] == ref["cost"], (seed, b, res.cost[b], ref["cost"])
