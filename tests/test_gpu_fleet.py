"""Fleet batches on the MI355X (include/teb_amd.h: teb_amd_set_scenes): the bands of many scenes in ONE launch.

  * bit identity, the main contract: every band of a fleet launch ends with the bits it has in a single-scene handle holding only its
    scene (generic_config_path = 1, multi_cu = -1, speculative_trials = -1, same layout, same capacities) - points and mixed fleets,
    the three layouts; and the automatic layout whose bands outgrow the optimistic choice against the pinned run;
  * oracle parity, independent of the device's single-scene path: 64 point scenes x 4 bands and the mixed fleet against
    oracle.optimize_batch per scene - counts identical, states <= 1e-7, cost and chi^2 rel 1e-7 (the tolerances of
    tests/test_gpu_measured_configs.py), every band checked, none skipped;
  * selection per scene against oracle.select_best; state and errors (the refused single-scene calls, the distributed collectives
    among them; compact_bands); TebFleetPlanner beside eight TebOptimalPlanner objects."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import fleet_cases  # noqa: E402
import sensitivity  # noqa: E402

from teb_local_planner_amd import _abi, planner  # noqa: E402

pytestmark = pytest.mark.gpu

THREADS = min(os.cpu_count() or 1, 16)
LAYOUTS = {"cr": 96, "band": 300, "bandg": 400}   # layout pin -> pose capacity
FIELDS = ("status", "lm_iterations", "lm_trials", "chi2", "cost", "lambda_")


def _optimize(s, cfg):
    s.optimize(cfg.optim.no_inner_iterations, cfg.optim.no_outer_iterations, True, cfg.hcp.selection_obst_cost_scale,
               cfg.hcp.selection_viapoint_cost_scale, cfg.hcp.selection_alternative_time_cost)


def _fleet_solver(f, layout="auto", cfg=None, **opts):
    mo, mv, mw = f.capacities()
    s = planner.TebBatchSolver(cfg or f.cfg, f.batch.count, f.batch.stride, mo, mv, mw, options=_abi.Options(layout=layout, **opts))
    s.set_scenes(f.tables, f.vias)
    s.set_band_scenes(f.scene_of)
    s.upload(f.batch)
    return s


def _run_fleet(f, layout="auto", cfg=None):
    s = _fleet_solver(f, layout, cfg)
    _optimize(s, cfg or f.cfg)
    res, out, inst = s.results(), s.download(f.batch.copy()), s.last_instantiation()
    assert not s.debug_overflow_flags().any()
    s.close()
    return out, res, inst


def _run_single_scenes(f, layout, cfg=None):
    """One single-scene handle per scene: [(band indices, out, res)]"""
    mo, mv, mw = f.capacities()
    runs = []
    for sc in range(f.n_scenes):
        sub, idx = f.scene_batch(sc)
        if not idx:
            continue
        s = planner.TebBatchSolver(cfg or f.cfg, f.batch.count, f.batch.stride, mo, mv, mw,
                                   options=_abi.Options(layout=layout, generic_config_path=True, multi_cu=-1, speculative_trials=-1))
        s.set_obstacles(f.tables[sc])
        s.set_via_points(f.vias[sc])
        s.upload(sub)
        _optimize(s, cfg or f.cfg)
        runs.append((idx, s.download(sub.copy()), s.results(), s.last_instantiation()))
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
    for k in range(out.count):
        _assert_bands_equal(out, res, k, out1, res1, k, label)


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
@pytest.mark.parametrize("kind", ["points", "mixed"])
def test_fleet_bands_equal_single_scene_handles_bit_for_bit(kind, layout):
    stride = LAYOUTS[layout]
    f = fleet_cases.point_fleet(101, stride=stride) if kind == "points" else fleet_cases.oracle_mixed_fleet(stride=stride)
    assert f.n_scenes == 6 and 6 <= f.batch.count <= 30
    out, res, inst = _run_fleet(f, layout)
    want = ({"band": 0, "cr": 1, "bandg": 2}[layout], 0, 0 if kind == "points" else 1)
    assert tuple(inst) == want, inst
    seen = 0
    for idx, out1, res1, inst1 in _run_single_scenes(f, layout):
        assert tuple(inst1) == want, (inst1, want)   # the single-scene handle ran the same (non-folded) kind
        for k, b in enumerate(idx):
            _assert_bands_equal(out, res, b, out1, res1, k, "%s/%s" % (kind, layout))
            seen += 1
    assert seen == f.batch.count
    assert (res.status == _abi.TEB_OK).all()


@pytest.mark.parametrize("empty", [0, 2])
def test_empty_scene_first_and_last_equal_single_scene_handles_bit_for_bit(empty):
    """The scene without obstacles at a pinned place: first (every later segment starts after an empty one) and last (its segment starts
    where the rows of the scene set end - what the padding of the set's store is for). The other two scenes hold polygons, so the
    offsets and vertices of a scene are found at its own segment."""
    f = fleet_cases.mixed_fleet(102, n_scenes=3, stride=LAYOUTS["cr"], empty=empty)
    assert f.n_scenes == 3 and len(f.tables[empty]) == 0 and f.bands_of(empty)
    with_polygons = [sc for sc in range(3) if len(f.tables[sc]) > 0 and (np.asarray(f.tables[sc].type) == _abi.OBST_POLYGON).any()]
    assert len(with_polygons) >= 2, with_polygons
    out, res, inst = _run_fleet(f, "cr")
    assert tuple(inst) == (1, 0, 1), inst
    seen = 0
    for idx, out1, res1, inst1 in _run_single_scenes(f, "cr"):
        assert tuple(inst1) == (1, 0, 1), inst1
        for k, b in enumerate(idx):
            _assert_bands_equal(out, res, b, out1, res1, k, "empty scene %d" % empty)
            seen += 1
    assert seen == f.batch.count
    assert (res.status == _abi.TEB_OK).all()


def _growing_fleet():
    """Bands that start short enough for the optimistic blocks-in-LDS layout of a 400-pose handle (whose own layout is the band in HBM)
    and that autoResize grows past it: 100 poses 0.08 m apart are 0.2 s apart at max_vel_x, dt_ref = 0.1 splits every interval and the
    detours round the obstacles add more. The CPU oracle ends these bands at 246 .. 341 poses."""
    f = fleet_cases.point_fleet(103, stride=400, poses=100, obstacles=(20, 60), spacing=0.08, amplitude=0.3)
    f.cfg.trajectory.dt_ref = 0.1
    f.cfg.trajectory.dt_hysteresis = 0.02
    return f


def test_automatic_layout_repeat_equals_the_pinned_run():
    f = _growing_fleet()
    out_p, res_p, inst_p = _run_fleet(f, "bandg")
    out_a, res_a, inst_a = _run_fleet(f, "auto")
    print("pose counts after autoResize:", out_p.n.tolist(), "instantiations (pinned, automatic):", inst_p, inst_a)
    assert int(out_p.n.max()) > 238, "no band outgrew the blocks-in-LDS layout: the repeat path was not taken"
    assert tuple(inst_p) == (2, 0, 0) and tuple(inst_a) == (2, 0, 0), (inst_p, inst_a)   # the repeat ran in the handle's own layout
    assert (res_p.status == _abi.TEB_OK).all()
    _assert_same_run((out_a, res_a), (out_p, res_p), "automatic layout against the pinned one")


def _oracle_parity(oracle, f, label):
    out, res, _ = _run_fleet(f)
    worst = {"state": 0.0, "cost": 0.0}
    total = 0
    for sc in range(f.n_scenes):
        sub, idx = f.scene_batch(sc)
        if not idx:
            continue
        ref, rres = oracle.optimize_batch(f.cfg, f.tables[sc], f.vias[sc], sub, threads=THREADS)
        dev = _abi.TebBatchHost(len(idx), f.batch.stride)
        dres = _abi.ResultsHost(len(idx))
        for k, b in enumerate(idx):
            for fld in ("n", "x", "y", "theta", "dt"):
                getattr(dev, fld)[k] = getattr(out, fld)[b]
            for fld in FIELDS:
                getattr(dres, fld)[k] = getattr(res, fld)[b]
        rep = sensitivity.compare_bands(dev, dres, ref, rres, None)
        assert rep["status_equal"] == rep["bands"] and rep["counts_equal"] == rep["bands"], (label, sc, rep)
        assert rep["checked"] == rep["bands"] == len(idx) and rep["skipped"] == 0, (label, sc, rep)
        assert rep["max_state_err"] <= 1e-7 and rep["max_cost_rel"] <= 1e-7, (label, sc, rep)
        np.testing.assert_allclose(dres.chi2, rres.chi2, rtol=1e-7)
        worst["state"] = max(worst["state"], rep["max_state_err"]); worst["cost"] = max(worst["cost"], rep["max_cost_rel"])
        total += rep["checked"]
    print("%s: %d bands of %d scenes against the oracle, max state err %.2e, max cost rel %.2e" % (label, total, f.n_scenes, worst["state"], worst["cost"]))
    assert total == f.batch.count


def test_oracle_parity_64_point_scenes_x_4_bands(oracle):
    f = fleet_cases.oracle_point_fleet()
    assert f.n_scenes == 64 and f.batch.count == 256 and all(len(t) == 60 for t in f.tables) and (f.batch.n == 100).all()
    _oracle_parity(oracle, f, "64 x 4 point fleet")


def test_oracle_parity_mixed_fleet(oracle):
    _oracle_parity(oracle, fleet_cases.oracle_mixed_fleet(), "mixed fleet")


def test_select_best_per_scene_equals_the_oracle_rule(oracle):
    f = fleet_cases.point_fleet(104, n_scenes=7, empty_tail=True)   # scene 7 has no band
    ns = f.n_scenes
    # a tie: every band of one scene (with two bands at least) is the same band, so all of them end with the same cost
    tie_scene = next(sc for sc in range(ns) if len(f.bands_of(sc)) >= 2)
    tied = f.bands_of(tie_scene)
    for b in tied[1:]:
        for fld in ("n", "x", "y", "theta", "dt"):
            getattr(f.batch, fld)[b] = getattr(f.batch, fld)[tied[0]]
    s = _fleet_solver(f)
    _optimize(s, f.cfg)
    cost = s.results().cost.copy()
    assert (cost[tied] == cost[tied[0]]).all()

    def want(last, init):
        best = np.full(ns, -1, np.int32)
        for sc in range(ns):
            idx = f.bands_of(sc)
            if not idx:
                continue
            loc = lambda b: idx.index(b) if b in idx else -1
            k, _ = oracle.select_best(f.cfg, cost[idx], last_best=loc(last[sc]), initial_plan=loc(init[sc]))
            best[sc] = idx[k]
        return best

    none = [-1] * ns
    first = [f.bands_of(sc)[0] if f.bands_of(sc) else -1 for sc in range(ns)]
    lastb = [f.bands_of(sc)[-1] if f.bands_of(sc) else -1 for sc in range(ns)]
    f.cfg.hcp.selection_cost_hysteresis, f.cfg.hcp.selection_prefer_initial_plan = 0.5, 0.6   # strong enough to change winners
    s.set_config(f.cfg)
    changed = 0
    for last, init in ((none, none), (lastb, none), (none, lastb), (first, lastb), (lastb, first)):
        best, bcost = s.select_best_per_scene(None if last is none else last, None if init is none else init)
        w = want(last, init)
        np.testing.assert_array_equal(best, w)
        changed += int((w != want(none, none)).any())
        for sc in range(ns):
            if best[sc] >= 0:
                scale = 0.5 if best[sc] == last[sc] else (0.6 if best[sc] == init[sc] else 1.0)
                assert bcost[sc] == cost[best[sc]] * scale
    assert changed >= 2, "hysteresis / initial-plan preference never changed a winner: the case checks nothing"
    best, _ = s.select_best_per_scene()
    assert best[ns - 1] == -1             # the scene without bands
    assert best[tie_scene] == min(tied)   # lowest band index on ties
    s.close()


def test_state_and_errors():
    f = fleet_cases.mixed_fleet(105)
    cfg = f.cfg
    mo, mv, mw = f.capacities()
    s = planner.TebBatchSolver(cfg, f.batch.count, f.batch.stride, mo, mv, mw, options=_abi.Options(generic_config_path=True, multi_cu=-1, speculative_trials=-1))
    # the single-scene run made before set_scenes
    s.set_obstacles(f.tables[0]); s.set_via_points(f.vias[0]); s.upload(f.batch)
    assert s.scene_count() == 0
    _optimize(s, cfg)
    single = (s.download(f.batch.copy()), s.results())
    # fleet run
    s.set_scenes(f.tables, f.vias); s.set_band_scenes(f.scene_of); s.upload(f.batch)
    assert s.scene_count() == f.n_scenes
    _optimize(s, cfg)
    fleet = (s.download(f.batch.copy()), s.results())
    # capacity errors leave the previous set installed
    big = _abi.ObstacleTable()
    for k in range(mo + 1):
        big.add_point(float(k), 0.0)
    for tables, vias, what in (([big], [[]], "max_obstacles"), (f.tables, [[(0.0, 0.0)] * (mw + 1)] + [[]] * (f.n_scenes - 1), "max_via_points"),
                               (f.tables + [f.tables[0]] * (f.batch.count), None, "")):
        with pytest.raises(planner.TebAmdError) as e:
            s.set_scenes(tables, vias)
        assert e.value.code == _abi.ERR_CAPACITY and what in str(e.value), str(e.value)
    poly = _abi.ObstacleTable()
    for k in range(mv // 3 + 1):
        poly.add_polygon([(k, 0.0), (k + 0.5, 0.0), (k + 0.5, 0.5)])
    if len(poly) <= mo:
        with pytest.raises(planner.TebAmdError) as e:
            s.set_scenes([poly])
        assert e.value.code == _abi.ERR_CAPACITY and "max_obstacle_vertices" in str(e.value)
    assert s.scene_count() == f.n_scenes
    s.upload(f.batch)
    _optimize(s, cfg)
    _assert_same_run((s.download(f.batch.copy()), s.results()), fleet, "after refused scene sets")
    # a band that maps to a scene >= n_scenes; the numeric Jacobian mode
    bad = f.scene_of.copy(); bad[0] = f.n_scenes
    s.set_band_scenes(bad)
    with pytest.raises(planner.TebAmdError) as e:
        _optimize(s, cfg)
    assert e.value.code == _abi.ERR_INVALID_ARG and "scene" in str(e.value)
    s.set_band_scenes(f.scene_of)
    cfg.jacobian_mode = _abi.JACOBIAN_G2O_NUMERIC
    s.set_config(cfg)
    with pytest.raises(planner.TebAmdError) as e:
        _optimize(s, cfg)
    assert e.value.code == _abi.ERR_INVALID_ARG and "ANALYTIC" in str(e.value)
    cfg.jacobian_mode = _abi.JACOBIAN_ANALYTIC
    s.set_config(cfg)
    # the single-scene calls are refused with a message that names the way out
    refused = {
        "set_obstacles": lambda: s.set_obstacles(f.tables[0]),
        "set_via_points": lambda: s.set_via_points(f.vias[0]),
        "set_obstacles_from_costmap": lambda: s.set_obstacles_from_costmap((0.0, 0.0, 0.0), 1.0),
        "set_obstacles_from_costmap_polygons": lambda: s.set_obstacles_from_costmap_polygons((0.0, 0.0, 0.0), 1.0),
        "compute_h_signatures": lambda: s.h_signatures(),
        "filter_equivalence_classes": lambda: s.filter_equivalence_classes(),
        "explore_candidates": lambda: s.explore_candidates((0.0, 0.0, 0.0), (1.0, 0.0, 0.0)),
        "filter_detours": lambda: s.filter_detours(np.ones(f.batch.count, np.int32), 0),
        "select_best": lambda: s.select_best(),
        "debug_linearize": lambda: s.debug_linearize(0, int(f.batch.n[0])),
        "debug_distance": lambda: s.debug_distance([0], [0.0], [0.0], [0.0]),
    }
    for name, call in refused.items():
        with pytest.raises(planner.TebAmdError) as e:
            call()
        assert e.value.code == _abi.ERR_INVALID_ARG and "teb_amd_clear_scenes" in str(e.value) and name in str(e.value), (name, str(e.value))
    # back to the single-scene table as it was
    s.clear_scenes()
    assert s.scene_count() == 0
    s.upload(f.batch)
    _optimize(s, cfg)
    _assert_same_run((s.download(f.batch.copy()), s.results()), single, "clear_scenes against the run before set_scenes")
    s.close()


def test_distributed_calls_are_refused_in_fleet_mode_and_still_enter_the_collective():
    """teb_amd_select_best_distributed and teb_amd_broadcast_band are collectives: a rank whose handle is in fleet mode is refused like
    any rank with a local error - it enters the all-gather, sends the unusable record / its status, and returns the error afterwards.
    On a world of one (the box has one GPU) the proof is the one of tests/test_gpu_distributed.py: the call returns its error AND the
    communicator is still usable - the next calls on it, after clear_scenes, give the right answers."""
    from teb_local_planner_amd import parallel
    f = fleet_cases.point_fleet(101, stride=96)
    s = _fleet_solver(f, "cr")
    _optimize(s, f.cfg)
    comm = parallel.RcclComm(parallel.RcclComm.unique_id(), 0, 1, 0)
    refused = {
        "teb_amd_select_best_distributed": lambda: s.select_best_distributed(comm, 10),
        "teb_amd_broadcast_band": lambda: s.broadcast_band(comm, 0, 0, f.batch.stride),
    }
    for _ in range(2):   # the second pass runs on a communicator that has been through two refused collectives
        for name, call in refused.items():
            with pytest.raises(planner.TebAmdError) as e:
                call()
            assert e.value.code == _abi.ERR_INVALID_ARG and "teb_amd_clear_scenes" in str(e.value) and name in str(e.value), (name, str(e.value))
    assert s.scene_count() == f.n_scenes
    s.clear_scenes()
    g, c, owner = s.select_best_distributed(comm, 10)
    assert g >= 10 and (g - 10, c) == s.select_best(-1, -1) and owner == 0
    strips = s.broadcast_band(comm, 0, g - 10, f.batch.stride)
    out = s.download(f.batch.copy())
    for u, v in zip(strips, out.get_teb(g - 10)):
        np.testing.assert_array_equal(u, v)
    comm.close()
    s.close()


def test_compact_bands_moves_the_band_scene_map_with_the_bands():
    """teb_amd_compact_bands drops bands and moves the last best one to the front; the band -> scene map follows, so that every kept
    band still runs against its own scene: after the compaction band k ends with the bits band map[k] has in the fleet left as it was."""
    f = fleet_cases.point_fleet(106, stride=96)
    B = f.batch.count
    out0, res0, _ = _run_fleet(f, "cr")
    keep = np.array([b % 3 != 1 for b in range(B)], np.int32)
    best = max(b for b in range(B) if keep[b] and f.scene_of[b] != f.scene_of[0])   # a kept band of another scene than band 0's goes first
    order = list(range(B))
    order[0], order[best] = order[best], order[0]
    moved = [b for b in order if keep[b]]
    assert [int(f.scene_of[b]) for b in moved] != [int(x) for x in f.scene_of[:len(moved)]], "the map need not move: the case checks nothing"
    s = _fleet_solver(f, "cr")
    assert s.compact_bands(keep, best) == (len(moved), 0)
    _optimize(s, f.cfg)
    out, res = s.download(f.batch.copy()), s.results()
    s.close()
    for k, b in enumerate(moved):
        _assert_bands_equal(out, res, k, out0, res0, b, "after compact_bands")


def test_set_config_in_fleet_mode_rederives_every_scenes_lists():
    f = fleet_cases.point_fleet(106, stride=96)
    assert f.cfg.obstacles.include_dynamic_obstacles
    s = _fleet_solver(f, "cr")
    _optimize(s, f.cfg)
    on = s.results().chi2.copy()
    f.cfg.obstacles.include_dynamic_obstacles = False
    s.set_config(f.cfg)
    s.upload(f.batch)
    _optimize(s, f.cfg)
    out, res = s.download(f.batch.copy()), s.results()
    s.close()
    assert (res.chi2 != on).any(), "the dynamic obstacles change nothing here: the case checks nothing"
    for idx, out1, res1, _ in _run_single_scenes(f, "cr"):
        for k, b in enumerate(idx):
            _assert_bands_equal(out, res, b, out1, res1, k, "include_dynamic_obstacles off")


def test_fleet_planner_beside_eight_optimal_planners():
    from teb_local_planner_amd.config import TebConfig
    R, ticks, max_poses = 8, 3, 128
    rng = np.random.default_rng(107)
    cfg = TebConfig()
    cfg.obstacles.include_dynamic_obstacles = True
    origin = rng.uniform(-20, 20, (R, 2))
    tables = []
    for r in range(R):
        t = _abi.ObstacleTable()
        for _ in range(int(rng.integers(5, 30))):
            t.add_point(origin[r, 0] + rng.uniform(0.5, 5.5), origin[r, 1] + rng.uniform(-1.5, 1.5))
        t.add_point(origin[r, 0] + 3.0, origin[r, 1] + 0.4, vel=(0.0, -0.1))
        tables.append(t)
    singles = [planner.TebOptimalPlanner(cfg, tables[r], [], max_poses=max_poses) for r in range(R)]
    fleet = planner.TebFleetPlanner(cfg, R, max_poses=max_poses, max_obstacles=sum(len(t) for t in tables))
    goal_shift = rng.uniform(-0.3, 0.3, (R, 2))
    prev = None   # the velocity commands of the last tick: the start velocities of this one
    for tick in range(ticks):
        starts = [(origin[r, 0] + 0.25 * tick, origin[r, 1] + 0.02 * tick * (r % 3 - 1), 0.01 * tick) for r in range(R)]
        # robot 5 gets a new far goal at tick 2: its band is initialised again while the others warm start
        goals = [(origin[r, 0] + 6.0 + goal_shift[r, 0] + (2.0 if (r == 5 and tick == 2) else 0.0), origin[r, 1] + goal_shift[r, 1], 0.1 * (r % 3 - 1)) for r in range(R)]
        ok = fleet.plan(starts, goals, prev, tables, [[] for _ in range(R)])
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
