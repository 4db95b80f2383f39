"""Both ends of a fleet tick per scene on the device (include/teb_amd.h): teb_amd_set_costmaps, teb_amd_set_scenes_from_costmaps,
teb_amd_is_trajectory_feasible_per_scene, teb_amd_update_and_prune_per_scene, teb_amd_get_velocity_commands, and
FleetHomotopyClassPlanner on top of them. Every kernel is the single-scene body behind a per-scene lookup, so the checks are equalities:
with the restatement / the oracle where the arithmetic is integer or IEEE-exact, bit for bit with the single-scene calls on twin
handles everywhere. The one tolerance: velocity commands against the CPU oracle pass through sin / cos, device against host libm -
1e-12 as in tests/test_gpu_strip_ops.py; against the per-band call on the device they are bit-equal."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import feasibility_cases  # noqa: E402
import fleet_tick_cases as FT  # noqa: E402
from test_costmap_obstacles import reference_costmap_obstacles  # noqa: E402
from oracle.oracle_py import Costmap  # noqa: E402
from teb_local_planner_amd import _abi, planner  # noqa: E402
from teb_local_planner_amd.config import TebConfig  # noqa: E402

pytestmark = pytest.mark.gpu
SINGLE = dict(generic_config_path=True, multi_cu=-1, speculative_trials=-1)   # the fleet contract of include/teb_amd.h
TOL = 1e-12


def _bits(v):
    a = np.ascontiguousarray(np.asarray(v))
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _same(u, v, what=""):
    u, v = _bits(u), _bits(v)
    assert u.shape == v.shape and np.array_equal(u, v), what


def _expected_points(t):
    return [reference_costmap_obstacles(g.cells, g.resolution, g.origin_x, g.origin_y, t.poses[s], t.dist) for s, g in enumerate(t.grids)]


def _solver(t, rows, verts=32, vias=4):
    s = planner.TebBatchSolver(t.cfg, t.batch.count, t.batch.stride, max(rows, 1), verts, vias, options=_abi.Options(**SINGLE))
    return s


def _state(s, t):
    """Everything the two handles must agree on after the scene set is installed (the pattern of tests/test_gpu_costmap_obstacles.py)."""
    s.set_band_scenes(t.scene_of)
    s.upload(t.batch)
    s.optimize(4, 3, compute_cost=True)
    r = s.results()
    b = s.download(t.batch.copy())
    out = {"res": (r.status, r.lm_iterations, r.lm_trials, r.chi2, r.cost), "band": (b.n, b.x, b.y, b.theta, b.dt),
           "inst": np.array(s.last_instantiation()), "best": s.select_best_per_scene()}
    sig = s.h_signatures_per_scene()
    out["hsig"] = tuple(sig)
    return out


def _assert_same_state(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert len(a[k]) == len(b[k]), k
        for p, q in zip(a[k], b[k]):
            _same(p, q, k)


@pytest.mark.parametrize("name", list(FT.SET_SHAPES))
def test_tables_of_every_scene_from_its_costmap(name):
    t = FT.table_set(name)
    pts = _expected_points(t)
    tables = [FT.concat_table(xs, ys, t.customs[s]) for s, (xs, ys) in enumerate(pts)]
    rows = sum(len(q) for q in tables)
    a, b = _solver(t, rows), _solver(t, rows)
    a.set_costmaps(t.grids)
    n, got = a.set_scenes_from_costmaps(t.poses, t.dist, t.customs)
    assert a.scene_count() == t.n_scenes
    for s, (xs, ys) in enumerate(pts):
        assert n[s] == len(xs), (s, n[s], len(xs))
        _same(got[s][0], xs, "x of scene %d" % s); _same(got[s][1], ys, "y of scene %d" % s)
    b.set_scenes(tables)
    _assert_same_state(_state(a, t), _state(b, t))
    # the set is not consumed: the same call again, and with the poses of another heading, gives the restatement again
    turned = t.poses.copy(); turned[:, 2] += 2.5
    n2, got2 = a.set_scenes_from_costmaps(turned, t.dist, None)
    for s, g in enumerate(t.grids):
        xs, ys = reference_costmap_obstacles(g.cells, g.resolution, g.origin_x, g.origin_y, turned[s], t.dist)
        assert n2[s] == len(xs)
        _same(got2[s][0], xs); _same(got2[s][1], ys)
    a.close(); b.close()


def test_tables_errors_leave_the_previous_set_and_the_single_costmap():
    t = FT.table_set("three_far")
    pts = _expected_points(t)
    tables = [FT.concat_table(xs, ys, t.customs[s]) for s, (xs, ys) in enumerate(pts)]
    rows = sum(len(q) for q in tables)
    a, b = _solver(t, rows), _solver(t, rows)
    L = planner.lib()
    with pytest.raises(planner.TebAmdError) as e:
        a.set_scenes_from_costmaps(t.poses, t.dist, t.customs)                 # no costmap set yet
    assert e.value.code == _abi.ERR_INVALID_ARG
    single = Costmap(np.full((4, 5), 254, np.uint8), 0.1, -0.3, 0.2)
    a.set_costmap(single.cells, single.resolution, single.origin_x, single.origin_y)
    a.set_costmaps(t.grids)
    a.set_scenes_from_costmaps(t.poses, t.dist, t.customs)
    b.set_scenes(tables)
    want = _state(b, t)
    _assert_same_state(_state(a, t), want)
    # a set of another size: refused
    a.set_costmaps(t.grids[:2])
    with pytest.raises(planner.TebAmdError) as e:
        a.set_scenes_from_costmaps(t.poses, t.dist, t.customs)
    assert e.value.code == _abi.ERR_INVALID_ARG
    # a bad grid in the set: the previous set (two grids) stays
    bad = [t.grids[0], Costmap(t.grids[1].cells, -1.0, 0.0, 0.0)]
    with pytest.raises(planner.TebAmdError) as e:
        a.set_costmaps(bad)
    assert e.value.code == _abi.ERR_INVALID_ARG
    with pytest.raises(planner.TebAmdError) as e:
        a.set_costmaps(t.grids * 9)                                            # more grids than max_tebs
    assert e.value.code == _abi.ERR_CAPACITY
    n2, _ = a.set_scenes_from_costmaps(t.poses[:2], t.dist, t.customs[:2])     # two scenes from the two grids that stayed
    assert list(n2) == [len(pts[0][0]), len(pts[1][0])] and a.scene_count() == 2
    # capacity: a full grid in the middle. n_costmap is reported, the live set (three scenes again) and its results stay
    a.set_costmaps(t.grids)
    a.set_scenes_from_costmaps(t.poses, t.dist, t.customs)
    full = [t.grids[0], Costmap(np.full_like(t.grids[1].cells, 254), t.grids[1].resolution, t.grids[1].origin_x, t.grids[1].origin_y), t.grids[2]]
    a.set_costmaps(full)
    n = np.full(3, -1, np.int32)
    poses = np.ascontiguousarray(t.poses)
    p = _abi.pack_scenes([c if c is not None else _abi.ObstacleTable() for c in t.customs])
    rc = L.teb_amd_set_scenes_from_costmaps(a._h, 3, _abi._ptr(poses, C.c_double), t.dist, p.obstacles, None, None, None, _abi._ptr(n, C.c_int32),
                                            None, None, 0)
    assert rc == _abi.ERR_CAPACITY
    assert list(n) == [len(pts[0][0]), 119 * 119, len(pts[2][0])]
    assert a.scene_count() == 3
    _assert_same_state(_state(a, t), want)                                     # as if the failed call had never been made
    # a bad custom table: refused, set intact
    wrong = _abi.ObstacleTable(); wrong.add_point(1.0, 1.0); wrong.type[0] = 9
    a.set_costmaps(t.grids)
    with pytest.raises(planner.TebAmdError) as e:
        a.set_scenes_from_costmaps(t.poses, t.dist, [wrong, None, None])
    assert e.value.code == _abi.ERR_INVALID_ARG
    _assert_same_state(_state(a, t), want)
    # the single costmap was never touched: a single-scene call after clear_scenes sees ITS grid (4 x 3 visited cells, all lethal)
    a.set_costmaps([])
    with pytest.raises(planner.TebAmdError):
        a.set_scenes_from_costmaps(t.poses, t.dist, t.customs)                 # the set is dropped
    a.clear_scenes()
    assert a.set_obstacles_from_costmap((0.0, 0.5, 0.0), 100.0)[0] == 4 * 3
    a.close(); b.close()


def _feas_solver(f, cfg):
    s = planner.TebBatchSolver(cfg, f.batch.count, f.batch.stride, 4, 4, 4)
    s.set_scenes([_abi.ObstacleTable() for _ in f.grids])
    s.set_band_scenes(f.scene_of)
    s.upload(f.batch)
    s.set_costmaps(f.grids)
    return s


def test_feasibility_of_one_band_per_scene_against_its_own_grid(oracle):
    f = FT.feasibility_fleet()
    cfg = TebConfig()
    ns = len(f.grids)
    s = _feas_solver(f, cfg)
    singles = []
    for k in range(ns):
        one = planner.TebBatchSolver(cfg, 1, f.batch.stride, 4, 4, 4)
        one.upload(f.singles[k])
        one.set_costmap(f.grids[k].cells, f.grids[k].resolution, f.grids[k].origin_x, f.grids[k].origin_y)
        singles.append(one)
    bands = f.bands.copy()
    for i, fp in enumerate(feasibility_cases.FOOTPRINTS.values()):
        for (inscribed, ang, look, dist) in FT.FEAS_PARAMS:
            use = bands.copy()
            use[i % ns] = -1 - i                                               # a negative entry, another scene every time
            ok, first = s.is_trajectory_feasible_per_scene(use, fp, inscribed, ang, look, dist)
            for k in range(ns):
                if use[k] < 0:
                    assert (ok[k], first[k]) == (-1, -1)
                    continue
                want = oracle.is_trajectory_feasible(f.batch, int(use[k]), f.grids[k], fp, inscribed, ang, look, dist)
                assert (bool(ok[k]), int(first[k])) == want, (i, k)
                assert singles[k].is_trajectory_feasible(0, fp, inscribed, ang, look, dist) == want, (i, k)
    # the first band of every scene (the decoys) against the same grids
    fp = feasibility_cases.FOOTPRINTS["rect"]
    ok, first = s.is_trajectory_feasible_per_scene(f.decoys, fp, 0.25, 0.3)
    for k in range(ns):
        assert (bool(ok[k]), int(first[k])) == oracle.is_trajectory_feasible(f.batch, int(f.decoys[k]), f.grids[k], fp, 0.25, 0.3)
    for one in singles:
        one.close()
    s.close()


def test_feasibility_per_scene_refuses_what_it_cannot_answer():
    f = FT.feasibility_fleet()
    cfg = TebConfig()
    fp = feasibility_cases.FOOTPRINTS["rect"]
    s = _feas_solver(f, cfg)

    def refused(bands, code=_abi.ERR_INVALID_ARG, inscribed=0.25):
        with pytest.raises(planner.TebAmdError) as e:
            s.is_trajectory_feasible_per_scene(bands, fp, inscribed, 0.3)
        assert e.value.code == code, str(e.value)

    other = f.bands.copy(); other[2] = f.bands[3]
    refused(other)                                                             # a band of another scene
    beyond = f.bands.copy(); beyond[0] = f.batch.count
    refused(beyond)                                                            # a band index >= count
    refused(f.bands, _abi.ERR_CAPACITY, inscribed=1e-12)                       # the sample limit of the single call
    s.set_costmaps(f.grids[:-1])
    refused(f.bands)                                                           # a costmap set of another size
    s.set_costmaps([])
    refused(f.bands)                                                           # no costmap set
    s.set_costmaps(f.grids)
    ok, _ = s.is_trajectory_feasible_per_scene(f.bands, fp, 0.25, 0.3)
    assert set(ok) <= {0, 1}
    s.clear_scenes()
    s._n_scenes = len(f.grids)   # (the wrapper's own shape check passes: the library answers)
    refused(f.bands)                                                           # no scenes set
    s.close()


def _prune_solver(f, fleet):
    s = planner.TebBatchSolver(f.cfg, f.batch.count, f.batch.stride, 4, 4, 4)
    if fleet:
        s.set_scenes([_abi.ObstacleTable() for _ in FT.PRUNE_COUNTS])
        s.set_band_scenes(f.scene_of)
    s.upload(f.batch)
    return s


def _prune_state(s, f):
    b = s.download(f.batch.copy())
    _, has_vs, _ = s.band_flags()
    vs = np.array([s.velocity_profile(k)[0] for k in range(f.batch.count)])     # row 0 of the profile is the band's start velocity
    return b, has_vs, vs


@pytest.mark.parametrize("with_goal", [True, False])
@pytest.mark.parametrize("vel", ["none", "all", "mask"])
def test_update_all_tebs_of_every_robot_in_one_launch(oracle, with_goal, vel):
    f = FT.prune_fleet()
    ms = FT.PRUNE_MIN_SAMPLES
    a, b = _prune_solver(f, True), _prune_solver(f, False)
    goals = f.goals if with_goal else None
    vels = None if vel == "none" else f.vels
    mask = f.mask if vel == "mask" else None
    a.update_and_prune_per_scene(f.starts, goals, ms, vels, mask)
    for k in range(f.batch.count):                                             # what it replaces: per band on the twin
        sc = int(f.scene_of[k])
        b.update_and_prune(f.starts[sc], None if goals is None else goals[sc], ms, b=k)
        if vels is not None and (mask is None or mask[sc]):
            b.set_velocity_start(vels[sc], True, b=k)
    (ba, fa, va), (bb, fb, vb) = _prune_state(a, f), _prune_state(b, f)
    _same(ba.n, bb.n, "counts"); _same(fa, fb, "has_vel_start"); _same(va, vb, "vel_start")
    for k in range(f.batch.count):
        sc = int(f.scene_of[k])
        want = oracle.update_and_prune(*f.batch.get_teb(k), f.starts[sc], None if goals is None else goals[sc], ms)
        for u, v, w in zip(ba.get_teb(k), bb.get_teb(k), want):
            _same(u, v, "band %d against the per-band call" % k); _same(u, w, "band %d against the oracle" % k)
        fixed = vels is not None and (mask is None or mask[sc])
        assert fa[k] == (1 if fixed else f.batch.has_vel_start[k])
        _same(va[k], vels[sc] if fixed else f.batch.vel_start[k], "start velocity of band %d" % k)
    # goals alone (no start): nothing is deleted
    a.upload(f.batch); b.upload(f.batch)
    a.update_and_prune_per_scene(None, f.goals, ms)
    for k in range(f.batch.count):
        b.update_and_prune(None, f.goals[int(f.scene_of[k])], ms, b=k)
    ba, bb = a.download(f.batch.copy()), b.download(f.batch.copy())
    _same(ba.n, f.batch.n)
    for k in range(f.batch.count):
        for u, v in zip(ba.get_teb(k), bb.get_teb(k)):
            _same(u, v)
    a.close(); b.close()


def test_update_and_prune_per_scene_refuses_what_it_cannot_do():
    f = FT.prune_fleet()
    s = planner.TebBatchSolver(f.cfg, f.batch.count, f.batch.stride, 8, 4, 4)
    ns = len(FT.PRUNE_COUNTS)
    L = planner.lib()
    st = np.ascontiguousarray(f.starts)
    call = lambda: L.teb_amd_update_and_prune_per_scene(s._h, _abi._ptr(st, C.c_double), None, 3, None, None)
    assert call() == _abi.ERR_INVALID_ARG                                      # no scenes set
    tables = []
    for k in range(ns):
        tables.append(_abi.ObstacleTable()); tables[-1].add_point(50.0 + k, 50.0)
    s.set_scenes(tables)
    assert call() == _abi.ERR_INVALID_ARG                                      # no bands
    s.set_band_scenes(np.where(f.scene_of == ns - 1, ns, f.scene_of))
    s.upload(f.batch)
    assert call() == _abi.ERR_INVALID_ARG and "maps to scene" in L.teb_amd_last_error().decode()   # a band of a scene >= n_scenes
    got = s.download(f.batch.copy())
    _same(got.n, f.batch.n); _same(got.x, f.batch.x)                           # nothing ran
    s.set_band_scenes(f.scene_of)
    assert call() == _abi.OK
    # the per-scene signatures are stale after the call
    s.h_signatures_per_scene(values=False)
    s.filter_equivalence_classes_per_scene(0.1, None)
    assert call() == _abi.OK
    with pytest.raises(planner.TebAmdError) as e:
        s.filter_equivalence_classes_per_scene(0.1, None)
    assert "first" in str(e.value)
    s.close()


@pytest.mark.parametrize("fleet", [True, False])
def test_commands_of_many_bands_in_one_call(oracle, fleet):
    f = FT.prune_fleet()
    s = _prune_solver(f, fleet)
    B = f.batch.count
    bands = np.array(list(range(B - 1, -1, -2)) + [-1] + list(range(0, B, 3)), np.int32)
    for la, prevent in ((1, 0), (4, 2)):
        ok, cmd = s.velocity_commands(bands, la, prevent)
        for i, k in enumerate(bands):
            if k < 0:
                assert not ok[i] and not cmd[i].any()
                continue
            one_ok, one = s.velocity_command(int(k), la, prevent)
            assert ok[i] == one_ok
            _same(cmd[i], one, "against the per-band call")
            want = oracle.consumers(f.cfg, f.batch, int(k), la, prevent)
            assert ok[i] == bool(want["ok"]) and np.abs(cmd[i] - want["cmd"]).max() <= TOL
    ok, cmd = s.velocity_commands([-1, -5])
    assert not ok.any() and not cmd.any()
    with pytest.raises(planner.TebAmdError) as e:
        s.velocity_commands([0, B])
    assert e.value.code == _abi.ERR_INVALID_ARG
    s.close()


def _tick_costmap(rng, ox, oy):
    """120 x 120 cells of 5 cm; a few lethal blobs ahead of the robot (it starts at (ox + 0.6, oy + 3) and drives along +x)."""
    cells = rng.integers(0, 100, size=(120, 120)).astype(np.uint8)
    for _ in range(int(rng.integers(2, 5))):
        mx, my = int(rng.integers(40, 90)), int(rng.integers(45, 75))
        cells[my:my + 2, mx:mx + 2] = 254
    cells[10, 5] = 254                                                         # behind the robot and far: filtered at 1.5 m
    return Costmap(cells, 0.05, ox, oy)


def test_whole_ticks_from_costmaps_to_commands_beside_one_planner_per_robot():
    """Three ticks of FleetHomotopyClassPlanner.plan(costmaps_per_robot=...), isTrajectoryFeasible, hasDiverged and getVelocityCommands
    on 3 robots beside three HomotopyClassPlanner objects of their own, each fed by set_obstacles_from_costmap: bands bit for bit; best
    band, verdict, divergence flag and command equal."""
    R = 3
    rng = np.random.default_rng(515)
    cfg = TebConfig()
    cfg.hcp.max_number_classes = 4
    cfg.optim.no_inner_iterations = 3; cfg.optim.no_outer_iterations = 2
    cfg.recovery.divergence_detection_enable = True
    cfg.recovery.divergence_detection_max_chi_squared = 2.0
    origins = [(-7.0, 3.0), (11.0, -4.0), (2.5, 9.0)]
    grids = [_tick_costmap(rng, ox, oy) for ox, oy in origins]
    customs = [None, FT.custom_pointlike(origins[1][0] + 1.0, origins[1][1] + 3.0), None]
    tables = [c if c is not None else _abi.ObstacleTable() for c in customs]
    starts = [(ox + 0.6, oy + 3.0, 0.0) for ox, oy in origins]
    goals = [(ox + 5.0, oy + 3.0 + 0.2 * r, 0.0) for r, (ox, oy) in enumerate(origins)]
    vels = [(0.0, 0.0, 0.0)] * R
    dist = cfg.obstacles.costmap_obstacles_behind_robot_dist
    cap = 64
    fleet = planner.FleetHomotopyClassPlanner(cfg, R, max_tebs=4 * R, max_poses=96, max_obstacles=R * cap, max_obstacle_vertices=8, max_via_points=4,
                                              options=_abi.Options(**SINGLE))
    ones = []
    for r in range(R):
        hp = planner.HomotopyClassPlanner(cfg, _abi.ObstacleTable(), [], None, max_tebs=4, max_poses=96)
        hp.solver.close()
        hp.solver = planner.TebBatchSolver(cfg, 4, 96, cap, 8, 4, options=_abi.Options(**SINGLE))
        hp.solver.set_via_points([])
        ones.append(hp)
    footprints = [feasibility_cases.FOOTPRINTS["tri"], feasibility_cases.FOOTPRINTS["rect"],
                  [(-0.3, -0.9), (0.9, -0.9), (0.9, 0.9), (-0.3, 0.9)]]         # the last one is wide: bands near a blob become infeasible
    for tick in range(3):
        best = fleet.plan(starts, goals, vels, tables, None, now=float(tick + 1), costmaps_per_robot=grids)
        for r, hp in enumerate(ones):
            g = grids[r]
            hp.solver.set_costmap(g.cells, g.resolution, g.origin_x, g.origin_y)
            n, xs, _ = hp.solver.set_obstacles_from_costmap(starts[r], dist, customs[r])
            assert 1 <= n <= cap - 3
            hp.plan(starts[r], goals[r], vels[r])
        bands = fleet.bands()
        for r, hp in enumerate(ones):
            mine, want = fleet.bands_of(r), hp.bands()
            assert len(mine) == len(want) >= 1, (tick, r)
            for k, b in enumerate(mine):
                for u, v in zip(bands[b], want[k]):
                    _same(u, v, "tick %d robot %d band %d" % (tick, r, k))
            assert best[r] == mine[hp.best_teb_], (tick, r)
        diverged = fleet.hasDiverged()
        assert diverged == [hp.solver.has_diverged(hp.best_teb_) for hp in ones], tick
        verdict = fleet.isTrajectoryFeasible(footprints[tick], 0.25)
        assert verdict == [hp.isTrajectoryFeasible(grids[r], footprints[tick], 0.25) for r, hp in enumerate(ones)], tick
        bands = fleet.bands()
        for r, hp in enumerate(ones):                                          # the checks removed the same bands on both sides
            mine, want = fleet.bands_of(r), hp.bands()
            assert len(mine) == len(want), (tick, r)
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
    for hp in ones:
        hp.solver.close()
    fleet.solver.close()
