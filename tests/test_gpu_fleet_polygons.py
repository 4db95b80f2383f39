"""teb_amd_set_scenes_from_costmap_polygons on the device (include/teb_amd.h): the polygon route of the costmap for every scene of a
fleet in three launches, and FleetHomotopyClassPlanner.plan(costmap_tile_cells=...) on top of it. The scene-set kernels are the
single-scene block body behind a per-scene record, so every check is an equality: the converted rows bit for bit with the restatement
of tests/costmap_polygon_cases.py and with the single-scene call on a handle that holds only that grid; the handle afterwards bit for bit
with a twin that got the same tables through teb_amd_set_scenes."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import costmap_polygon_cases as CP  # noqa: E402
import feasibility_cases  # noqa: E402
import fleet_polygon_cases as FP  # noqa: E402
import fleet_tick_cases as FT  # noqa: E402
from oracle.oracle_py import Costmap  # noqa: E402
from teb_local_planner_amd import _abi, planner  # noqa: E402
from teb_local_planner_amd.config import TebConfig  # noqa: E402

pytestmark = pytest.mark.gpu
SINGLE = dict(generic_config_path=True, multi_cu=-1, speculative_trials=-1)   # the fleet contract of include/teb_amd.h
SENTINEL = -12345


def _bits(v):
    a = np.ascontiguousarray(np.asarray(v))
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _same(u, v, what=""):
    u, v = _bits(u), _bits(v)
    assert u.shape == v.shape and np.array_equal(u, v), what


def _solver(t, rows, verts=32, vias=4):
    return planner.TebBatchSolver(t.cfg, t.batch.count, t.batch.stride, max(rows, 1), max(verts, 1), vias, options=_abi.Options(**SINGLE))


def _state(s, t):
    """Everything two handles must agree on after the scene set is installed (the pattern of tests/test_gpu_fleet_tick.py)."""
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


def _tables(t, rows):
    return [FP.concat_table(rows[s], t.customs[s]) for s in range(t.n_scenes)]


def _need(tables):
    return sum(len(q) for q in tables), sum(len(q.vert_x) for q in tables)


class Raw:
    """One raw call of teb_amd_set_scenes_from_costmap_polygons: rc, n_obstacles, n_points, out_offset, out_x, out_y (sentinel-filled)."""

    def __init__(self, a, poses, dist, tiles, customs, cap_o, cap_p, n_scenes=None, outs=True, via_count=None):
        ns = len(poses) if n_scenes is None else n_scenes
        poses = np.ascontiguousarray(np.asarray(poses, np.float64))
        self.n_o = np.full(len(poses), SENTINEL, np.int32); self.n_p = np.full(len(poses), SENTINEL, np.int32)
        self.off = np.full(max(cap_o, 0) + 2, SENTINEL, np.int32)
        self.x = np.full(max(cap_p, 0) + 1, float(SENTINEL)); self.y = np.full(max(cap_p, 0) + 1, float(SENTINEL))
        tl = None if tiles is None else _abi.i32(tiles)
        p = None if customs is None else _abi.pack_scenes([c if c is not None else _abi.ObstacleTable() for c in customs])
        I = lambda v: _abi._ptr(v, C.c_int32)
        D = lambda v: _abi._ptr(v, C.c_double)
        vc = None if via_count is None else _abi.i32(via_count)
        self.rc = planner.lib().teb_amd_set_scenes_from_costmap_polygons(
            a._h, ns, D(poses), float(dist), I(tl), None if p is None else p.obstacles, I(vc), None, None, I(self.n_o), I(self.n_p),
            I(self.off) if outs else None, D(self.x) if outs else None, D(self.y) if outs else None, cap_o, cap_p)

    def untouched(self):
        return (self.off == SENTINEL).all() and (self.x == SENTINEL).all() and (self.y == SENTINEL).all()


def _check_rows(got_n_o, got_n_p, off, xs, ys, rows):
    """the polygon list of the scenes one after the other against the restatement of every scene"""
    r0 = v0 = 0
    for s, (types, eoff, ex, ey) in enumerate(rows):
        n, nv = len(types), len(ex)
        assert (got_n_o[s], got_n_p[s]) == (n, nv), (s, got_n_o[s], got_n_p[s], n, nv)
        _same(off[r0:r0 + n + 1] - v0, eoff, "offsets of scene %d" % s)
        _same(xs[v0:v0 + nv], ex, "x of scene %d" % s); _same(ys[v0:v0 + nv], ey, "y of scene %d" % s)
        r0 += n; v0 += nv
    return r0, v0


@pytest.mark.parametrize("name", list(FP.SET_SHAPES))
def test_rows_of_every_scene_bit_for_bit_with_the_restatement(name):
    t = FP.polygon_set(name)
    rows = FP.expected_rows(name)
    need_r, need_v = _need(_tables(t, rows))
    a = _solver(t, need_r, need_v)
    a.set_costmaps(t.grids)
    nr, nv = sum(len(r[0]) for r in rows), sum(len(r[2]) for r in rows)
    c = Raw(a, t.poses, t.dist, t.tiles, t.customs, nr, nv)
    assert c.rc == _abi.OK, planner.lib().teb_amd_last_error()
    assert _check_rows(c.n_o, c.n_p, c.off, c.x, c.y, rows) == (nr, nv)
    assert c.off[nr] == nv and c.off[nr + 1] == SENTINEL and c.x[nv] == SENTINEL and c.y[nv] == SENTINEL   # nothing beyond
    assert a.scene_count() == t.n_scenes
    # the binding's tables
    got = a.set_scenes_from_costmap_polygons(t.poses, t.dist, t.tiles, t.customs)
    for s, (_, off, xs, ys) in enumerate(rows):
        want = CP.as_table(off, xs, ys)
        for k in ("type", "dynamic", "vert_offset"):
            assert getattr(got[s], k) == getattr(want, k), (s, k)
        for k in ("ax", "ay", "bx", "by", "radius", "vx", "vy", "vert_x", "vert_y"):
            _same(np.array(getattr(got[s], k), np.float64), np.array(getattr(want, k), np.float64), "%s of scene %d" % (k, s))
    # the set is not consumed: every heading turned by 2.5 rad gives the restatement again
    turned = t.poses.copy(); turned[:, 2] += 2.5
    rows2 = FP.expected_rows(name, 2.5)
    c = Raw(a, turned, t.dist, t.tiles, None, need_r, 2 * need_r + need_v)
    assert c.rc == _abi.OK
    _check_rows(c.n_o, c.n_p, c.off, c.x, c.y, rows2)
    a.close()


@pytest.mark.parametrize("name", list(FP.SET_SHAPES))
def test_every_scene_equals_the_single_scene_call_on_its_grid(name):
    t = FP.polygon_set(name)
    rows = FP.expected_rows(name)
    nr, nv = sum(len(r[0]) for r in rows), sum(len(r[2]) for r in rows)
    pv = sum(len(q.vert_x) for q in _tables(t, rows))
    a, one = _solver(t, nr, pv), _solver(t, nr, pv)
    a.set_costmaps(t.grids)
    c = Raw(a, t.poses, t.dist, t.tiles, None, nr, nv)
    assert c.rc == _abi.OK
    L = planner.lib()
    r0 = v0 = 0
    for s, g in enumerate(t.grids):
        one.set_costmap(g.cells, g.resolution, g.origin_x, g.origin_y)
        pose = _abi.f64(t.poses[s])
        n_o, n_p = C.c_int32(-1), C.c_int32(-1)
        off = np.full(nr + 1, SENTINEL, np.int32); xs = np.zeros(max(nv, 1)); ys = np.zeros(max(nv, 1))
        rc = L.teb_amd_set_obstacles_from_costmap_polygons(one._h, _abi._ptr(pose, C.c_double), t.dist, int(t.tiles[s]), None, C.byref(n_o),
                                                           C.byref(n_p), _abi._ptr(off, C.c_int32), _abi._ptr(xs, C.c_double),
                                                           _abi._ptr(ys, C.c_double), nr, nv)
        assert rc == _abi.OK
        assert (n_o.value, n_p.value) == (c.n_o[s], c.n_p[s]), s
        _same(c.off[r0:r0 + n_o.value + 1] - v0, off[:n_o.value + 1], "offsets of scene %d" % s)
        _same(c.x[v0:v0 + n_p.value], xs[:n_p.value], "x of scene %d" % s); _same(c.y[v0:v0 + n_p.value], ys[:n_p.value], "y of scene %d" % s)
        r0 += n_o.value; v0 += n_p.value
    assert (r0, v0) == (nr, nv)
    a.close(); one.close()


@pytest.mark.parametrize("name", list(FP.SET_SHAPES))
def test_the_handle_is_the_one_set_scenes_makes_from_the_same_tables(name):
    t = FP.polygon_set(name)
    tables = _tables(t, FP.expected_rows(name))
    need_r, need_v = _need(tables)
    a, b = _solver(t, need_r, need_v), _solver(t, need_r, need_v)
    a.set_costmaps(t.grids)
    a.set_scenes_from_costmap_polygons(t.poses, t.dist, t.tiles, t.customs)
    b.set_scenes(tables)
    _assert_same_state(_state(a, t), _state(b, t))
    a.close(); b.close()


@pytest.mark.parametrize("name", list(FP.SET_SHAPES))
def test_tiles_of_one_cell_everywhere_are_the_point_route(name):
    t = FP.polygon_set(name)
    rows = FP.expected_rows(name, 0.0, 1)
    need_r, need_v = _need(_tables(t, rows))
    a, b = _solver(t, need_r, need_v), _solver(t, need_r, need_v)
    a.set_costmaps(t.grids); b.set_costmaps(t.grids)
    got = a.set_scenes_from_costmap_polygons(t.poses, t.dist, 1, t.customs)
    n, pts = b.set_scenes_from_costmaps(t.poses, t.dist, t.customs)
    for s in range(t.n_scenes):
        assert len(got[s]) == n[s] == len(rows[s][0]) and set(got[s].type) <= {CP.POINT}
        _same(np.array(got[s].ax, np.float64), pts[s][0]); _same(np.array(got[s].ay, np.float64), pts[s][1])
    _assert_same_state(_state(a, t), _state(b, t))
    a.close(); b.close()


def test_refusals_leave_the_previous_set_and_the_single_costmap():
    t = FP.polygon_set("mixed")
    rows = FP.expected_rows("mixed")
    tables = _tables(t, rows)
    need_r, need_v = _need(tables)
    nr, nv = sum(len(r[0]) for r in rows), sum(len(r[2]) for r in rows)
    L = planner.lib()
    a = _solver(t, need_r, need_v)
    single = Costmap(np.full((4, 5), 254, np.uint8), 0.1, -0.3, 0.2)
    a.set_costmap(single.cells, single.resolution, single.origin_x, single.origin_y)
    # no costmap set, no scenes yet: nothing is installed. The issue's "no costmap set leaves the previous set" is the call after
    # set_costmaps([]) near the end of this test, where a scene set exists to be left
    assert Raw(a, t.poses, t.dist, t.tiles, t.customs, nr, nv).rc == _abi.ERR_INVALID_ARG
    assert a.scene_count() == 0
    a.set_costmaps(t.grids)
    a.set_scenes_from_costmap_polygons(t.poses, t.dist, t.tiles, t.customs)
    want = _state(a, t)

    def refused(call, code=_abi.ERR_INVALID_ARG):
        assert call.rc == code, (call.rc, L.teb_amd_last_error())
        assert a.scene_count() == t.n_scenes
        _assert_same_state(_state(a, t), want)                                  # as if the call had never been made
        return call

    a.set_costmaps(t.grids[:2])
    refused(Raw(a, t.poses, t.dist, t.tiles, t.customs, nr, nv))               # a set of another size
    a.set_costmaps(t.grids)
    refused(Raw(a, t.poses, t.dist, None, t.customs, nr, nv))                  # tile_cells null
    for bad in (0, 65):                                                        # a tile outside 1 .. 64 in a middle scene
        tiles = t.tiles.copy(); tiles[2] = bad
        refused(Raw(a, t.poses, t.dist, tiles, t.customs, nr, nv))
    refused(Raw(a, t.poses, t.dist, t.tiles, t.customs, -1, nv))               # a negative capacity
    refused(Raw(a, t.poses, t.dist, t.tiles, t.customs, nr, -1))
    wrong = _abi.ObstacleTable(); wrong.add_point(1.0, 1.0); wrong.type[0] = 9
    refused(Raw(a, t.poses, t.dist, t.tiles, [None, None, wrong, None], nr, nv))   # a bad custom table
    refused(Raw(a, t.poses, t.dist, t.tiles, t.customs, nr, nv, via_count=[0, 0, -1, 0]))   # bad via arrays
    refused(Raw(a, t.poses, t.dist, t.tiles, t.customs, nr, nv, n_scenes=0))
    # row capacity: a full grid at T = 1 in the middle; the counts are reported
    g1 = t.grids[1]
    a.set_costmaps([t.grids[0], Costmap(np.full_like(g1.cells, 254), g1.resolution, g1.origin_x, g1.origin_y), t.grids[2], t.grids[3]])
    c = refused(Raw(a, t.poses, t.dist, t.tiles, t.customs, nr, nv), _abi.ERR_CAPACITY)
    assert list(c.n_o) == [len(rows[0][0]), 119 * 119, len(rows[2][0]), len(rows[3][0])]
    assert list(c.n_p) == [len(rows[0][2]), 119 * 119, len(rows[2][2]), len(rows[3][2])]
    assert c.untouched()
    a.set_costmaps(t.grids)
    # the out arrays: written only when both capacities suffice (the call itself succeeds either way)
    for cap_o, cap_p, written in ((nr - 1, nv, False), (nr, nv - 1, False), (nr, nv, True)):
        c = Raw(a, t.poses, t.dist, t.tiles, t.customs, cap_o, cap_p)
        assert c.rc == _abi.OK and list(c.n_o) == [len(r[0]) for r in rows]
        assert c.untouched() == (not written)
        if written:
            _check_rows(c.n_o, c.n_p, c.off, c.x, c.y, rows)
    assert Raw(a, t.poses, t.dist, t.tiles, t.customs, nr, nv, outs=False).rc == _abi.OK
    _assert_same_state(_state(a, t), want)
    # the single-scene polygon call stays refused while scenes are set
    pose = _abi.f64(t.poses[0])
    n_o = C.c_int32(-1)
    assert L.teb_amd_set_obstacles_from_costmap_polygons(a._h, _abi._ptr(pose, C.c_double), 1.5, 8, None, C.byref(n_o), None, None, None, None,
                                                         0, 0) == _abi.ERR_INVALID_ARG
    # the single costmap was never touched: a single-scene call after clear_scenes sees ITS grid (4 x 3 visited cells, all lethal)
    a.set_costmaps([])
    refused(Raw(a, t.poses, t.dist, t.tiles, t.customs, nr, nv))               # the set is dropped
    a.clear_scenes()
    assert a.set_obstacles_from_costmap((0.0, 0.5, 0.0), 100.0)[0] == 4 * 3
    a.close()


def test_polygon_vertex_capacity_one_short_leaves_the_previous_set():
    t = FP.polygon_set("mixed")
    rows = FP.expected_rows("mixed")
    need_r, need_v = _need(_tables(t, rows))
    custom_v = sum(len(c.vert_x) for c in t.customs if c is not None)
    assert custom_v >= 1
    a = _solver(t, need_r, need_v - 1)
    a.set_costmaps(t.grids)
    a.set_scenes_from_costmap_polygons(t.poses, t.dist, t.tiles, None)        # the converted rows alone fit
    want = _state(a, t)
    nr, nv = sum(len(r[0]) for r in rows), sum(len(r[2]) for r in rows)
    c = Raw(a, t.poses, t.dist, t.tiles, t.customs, nr, nv)
    assert c.rc == _abi.ERR_CAPACITY and "vertices" in planner.lib().teb_amd_last_error().decode()
    assert list(c.n_o) == [len(r[0]) for r in rows] and list(c.n_p) == [len(r[2]) for r in rows]
    assert c.untouched()
    _assert_same_state(_state(a, t), want)
    a.close()


def _tick_costmap(rng, ox, oy):
    """120 x 120 cells of 5 cm; a few lethal blobs ahead of the robot (it starts at (ox + 0.6, oy + 3) and drives along +x)."""
    cells = rng.integers(0, 100, size=(120, 120)).astype(np.uint8)
    for _ in range(int(rng.integers(2, 5))):
        mx, my = int(rng.integers(40, 90)), int(rng.integers(45, 75))
        cells[my:my + 2, mx:mx + 2] = 254
    cells[10, 5] = 254                                                         # behind the robot and far: filtered at 1.5 m
    return Costmap(cells, 0.05, ox, oy)


def test_whole_ticks_on_the_polygon_route_beside_one_planner_per_robot():
    """Three ticks of FleetHomotopyClassPlanner.plan(costmaps_per_robot=..., costmap_tile_cells=[8, 1, 8]), isTrajectoryFeasible,
    hasDiverged and getVelocityCommands on 3 robots beside three HomotopyClassPlanner objects of their own, each fed by
    set_obstacles_from_costmap_polygons with the same tile: bands bit for bit; best band, verdict, divergence flag and command equal
    (the comparison of tests/test_gpu_fleet_tick.py)."""
    R = 3
    tiles = [8, 1, 8]
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
    cap, vcap = 64, 64
    fleet = planner.FleetHomotopyClassPlanner(cfg, R, max_tebs=4 * R, max_poses=96, max_obstacles=R * cap, max_obstacle_vertices=R * vcap,
                                              max_via_points=4, options=_abi.Options(**SINGLE))
    with pytest.raises(ValueError):
        fleet.plan(starts, goals, vels, tables, None, now=0.5, costmap_tile_cells=tiles)   # tiles without costmaps
    with pytest.raises(ValueError):
        fleet.plan(starts, goals, vels, tables, None, now=0.5, costmap_tile_cells=8)
    ones = []
    for r in range(R):
        hp = planner.HomotopyClassPlanner(cfg, _abi.ObstacleTable(), [], None, max_tebs=4, max_poses=96)
        hp.solver.close()
        hp.solver = planner.TebBatchSolver(cfg, 4, 96, cap, vcap, 4, options=_abi.Options(**SINGLE))
        hp.solver.set_via_points([])
        ones.append(hp)
    footprints = [feasibility_cases.FOOTPRINTS["tri"], feasibility_cases.FOOTPRINTS["rect"],
                  [(-0.3, -0.9), (0.9, -0.9), (0.9, 0.9), (-0.3, 0.9)]]         # the last one is wide: bands near a blob become infeasible
    kinds = set()
    for tick in range(3):
        best = fleet.plan(starts, goals, vels, tables, None, now=float(tick + 1), costmaps_per_robot=grids, costmap_tile_cells=tiles)
        for r, hp in enumerate(ones):
            g = grids[r]
            hp.solver.set_costmap(g.cells, g.resolution, g.origin_x, g.origin_y)
            conv = hp.solver.set_obstacles_from_costmap_polygons(starts[r], dist, tiles[r], customs[r])
            assert 1 <= len(conv) <= cap - 3
            kinds |= set(conv.type)
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
    assert CP.POLYGON in kinds and CP.POINT in kinds                           # the ticks ran on polygon rows, not on points alone
    for hp in ones:
        hp.solver.close()
    fleet.solver.close()
