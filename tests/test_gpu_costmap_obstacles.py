"""teb_amd_set_obstacles_from_costmap on the device: updateObstacleContainerWithCostmap (reference src/teb_local_planner_ros.cpp:478-504)
on the grid of teb_amd_set_costmap, bit for bit against the restatement of tests/test_costmap_obstacles.py, and a handle that got its
table this way behaves exactly like one that got the same concatenated table through teb_amd_set_obstacles."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from test_costmap_obstacles import reference_costmap_obstacles  # noqa: E402
from teb_local_planner_amd import _abi, planner, scenes  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(1, 37), (41, 1), (2, 2), (63, 65), (120, 120), (401, 257), (1000, 1000)]   # (size_x, size_y)
DISTS = [-1.0, 0.0, 1.5, 100.0]


def _grid(rng, sx, sy, frac):
    """uint8 [sy, sx]: every cost value present where the grid is large enough, a fraction frac of the cells lethal."""
    cells = rng.integers(0, 256, size=(sy, sx)).astype(np.uint8)
    cells[cells == 254] = 253
    flat = cells.reshape(-1)
    if flat.size >= 256:
        flat[rng.permutation(flat.size)[:256]] = rng.permutation(256).astype(np.uint8)
    if frac > 0:
        flat[rng.random(flat.size) < frac] = 254
    return cells


def _solver(max_obstacles, cfg=None, batch=None, max_verts=1):
    cfg = cfg or scenes.scene_c1()[0]
    s = planner.TebBatchSolver(cfg, batch.count if batch is not None else 1, batch.stride if batch is not None else 16,
                               max(max_obstacles, 1), max(max_verts, 1), 4)
    if batch is not None:
        s.upload(batch)
    return s


def _concat(xs, ys, custom):
    """The table teb_amd_set_obstacles gets: the cell points, then the custom rows (cells have no vertices: offsets unchanged)."""
    t = _abi.ObstacleTable()
    for x, y in zip(xs, ys):
        t.add_point(float(x), float(y))
    if custom is not None:
        for k in ("type", "ax", "ay", "bx", "by", "radius", "vx", "vy", "dynamic", "vert_x", "vert_y"):
            getattr(t, k).extend(getattr(custom, k))
        t.vert_offset.extend(custom.vert_offset[1:])
    return t


def _custom_mixed():
    c = _abi.ObstacleTable()
    c.add_point(1.5, 0.45)
    c.add_circle(2.4, 0.9, 0.2)
    c.add_line(4.0, 0.7, 4.8, 1.2)
    c.add_pill(1.0, -0.9, 1.8, -1.1, 0.15)
    c.add_polygon([(4.5, -0.5), (5.1, -0.8), (5.0, -0.2)])
    c.add_point(2.0, -1.5, vel=(0.05, 0.12))
    c.add_circle(5.0, 1.5, 0.15, vel=(-0.1, -0.1))
    return c


def _custom_pointlike():
    c = _abi.ObstacleTable()
    c.add_point(1.5, 0.45)
    c.add_circle(2.4, 0.9, 0.2)
    c.add_point(3.2, -0.6)
    return c


def _state(s, M, batch):
    """Everything the tests require to be equal on the two handles."""
    rng = np.random.default_rng(11)
    q = 3
    oi = np.repeat(np.arange(M), q)
    x = rng.uniform(-0.5, 6.5, M * q); y = rng.uniform(-1.5, 1.5, M * q); th = rng.uniform(-math.pi, math.pi, M * q)
    out = {}
    if M > 0:
        out["dist"] = s.debug_distance(oi, x, y, th)
        out["dist_t"] = s.debug_distance(oi, x, y, th, t=np.full(M * q, 0.7))
    s.upload(batch)
    s.optimize(4, 3, compute_cost=True)
    r = s.results()
    out["inst"] = s.last_instantiation()
    out["res"] = (r.status, r.lm_iterations, r.lm_trials, r.chi2, r.cost)
    b = s.download(batch.copy())
    out["band"] = (b.n, b.x, b.y, b.theta, b.dt)
    out["best"] = s.select_best()
    out["hsig"] = s.h_signatures()
    return out


def _bits(v):
    """Arrays and scalars by their bits (NaN and signed zeros included)."""
    a = np.ascontiguousarray(np.asarray(v))
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _assert_same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        u, v = a[k], b[k]
        u, v = (u, v) if isinstance(u, tuple) else ((u,), (v,))
        assert len(u) == len(v), k
        for p, q in zip(u, v):
            p, q = _bits(p), _bits(q)
            assert p.shape == q.shape and np.array_equal(p, q), k


def _pair(cfg, batch, cells, res, ox, oy, pose, dist, custom, max_verts=16):
    xs, ys = reference_costmap_obstacles(cells, res, ox, oy, pose, dist)
    M = len(xs) + (len(custom) if custom is not None else 0)
    a = _solver(M, cfg, batch, max_verts)
    b = _solver(M, cfg, batch, max_verts)
    a.set_costmap(cells, res, ox, oy)
    n, gx, gy = a.set_obstacles_from_costmap(pose, dist, custom)
    assert n == len(xs) and np.array_equal(gx, xs) and np.array_equal(gy, ys)
    b.set_obstacles(_concat(xs, ys, custom))
    return a, b, M


@pytest.mark.parametrize("seed", range(42))
def test_list_bit_for_bit(seed):
    rng = np.random.default_rng(7000 + seed)
    sx, sy = SHAPES[seed % len(SHAPES)]
    big = sx * sy >= 1000 * 1000
    frac = [0.0, 0.01, 0.02, 0.045][seed // len(SHAPES) % 4] if big else [0.0, 0.02, 0.1, 0.3][seed // len(SHAPES) % 4]
    cells = _grid(rng, sx, sy, frac)
    res = float(rng.uniform(0.02, 0.2)); ox, oy = float(rng.uniform(-20, 5)), float(rng.uniform(-20, 5))
    pose = (ox + rng.uniform(0, sx * res), oy + rng.uniform(0, sy * res), rng.uniform(-4, 4))
    dist = DISTS[seed % 4]
    xs, ys = reference_costmap_obstacles(cells, res, ox, oy, pose, dist)
    assert len(xs) <= 50000
    s = _solver(len(xs))
    s.set_costmap(cells, res, ox, oy)
    n, gx, gy = s.set_obstacles_from_costmap(pose, dist)
    assert n == len(xs), (n, len(xs))
    assert np.array_equal(gx, xs) and np.array_equal(gy, ys)
    s.close()


def test_boundaries_of_the_behind_filter():
    res, ox, oy = 0.1, -0.3, 0.2
    cells = np.zeros((10, 10), np.uint8)
    cells[3, 2] = 254                        # centre (-0.05, 0.55)
    pose = (0.77, 0.51, 0.3)
    wx, wy = ox + 2.5 * res, oy + 3.5 * res
    dx, dy = np.float64(wx - pose[0]), np.float64(wy - pose[1])
    assert dx * math.cos(pose[2]) + dy * math.sin(pose[2]) < 0
    norm = float(np.sqrt(dx * dx + dy * dy))
    s = _solver(4)
    s.set_costmap(cells, res, ox, oy)
    assert s.set_obstacles_from_costmap(pose, norm)[0] == 1                        # norm > dist is false: kept
    assert s.set_obstacles_from_costmap(pose, np.nextafter(norm, -np.inf))[0] == 0  # one ulp less: far and behind, dropped
    # robot on the centre line of column 4 facing +x: dot == 0 exactly for that column, which is never "behind"
    cells = np.zeros((12, 9), np.uint8)
    cells[:, 4] = 254
    cells[:, 1] = 254
    pose = (ox + 4.5 * res, oy + 0.5, 0.0)
    s2 = _solver(32)
    s2.set_costmap(cells, res, ox, oy)
    n, gx, gy = s2.set_obstacles_from_costmap(pose, 0.0)
    xs, ys = reference_costmap_obstacles(cells, res, ox, oy, pose, 0.0)
    assert n == 11 and np.array_equal(gx, xs) and np.array_equal(gy, ys)     # column 4 (rows 0 .. 10), column 1 dropped
    assert np.all(gx == pose[0])
    s.close(); s2.close()


def _scene_grid(rng, frac, sx=140, sy=60):
    """A grid over the bands of scenes.scene_small_mixed (x 0 .. 6, y within +-1): 5 cm cells from (-0.5, -1.5)."""
    cells = _grid(rng, sx, sy, frac)
    return cells, 0.05, -0.5, -1.5


@pytest.mark.parametrize("B", [1, 8])
def test_same_handle_as_set_obstacles_mixed_table(B):
    cfg, _, via, batch = scenes.scene_small_mixed(B=B, footprint="polygon")
    cells, res, ox, oy = _scene_grid(np.random.default_rng(B), 0.004)
    a, b, M = _pair(cfg, batch, cells, res, ox, oy, (0.3, 0.1, 0.2), 1.5, _custom_mixed())
    for s in (a, b):
        s.set_via_points(via)
    _assert_same(_state(a, M, batch), _state(b, M, batch))
    cfg.obstacles.include_dynamic_obstacles = not cfg.obstacles.include_dynamic_obstacles
    a.set_config(cfg); b.set_config(cfg)
    _assert_same(_state(a, M, batch), _state(b, M, batch))
    a.close(); b.close()


def test_same_handle_as_set_obstacles_point_like_both_distance_paths():
    cfg, _, via, batch = scenes.scene_small_mixed(B=4, footprint="circular")
    insts = []
    for frac, lo, hi in ((0.024, 100, 400), (0.6, 4000, 8000)):   # ~ 200 cells: LDS obstacle cache; ~ 5000: generic distance path
        cells, res, ox, oy = _scene_grid(np.random.default_rng(3), frac)
        a, b, M = _pair(cfg, batch, cells, res, ox, oy, (0.0, 0.0, 0.0), 1.5, _custom_pointlike())
        assert lo <= M <= hi, M
        sa, sb = _state(a, M, batch), _state(b, M, batch)
        _assert_same(sa, sb)
        insts.append(sa["inst"])
        a.close(); b.close()
    assert insts[0] != insts[1], insts


def test_errors_leave_the_table_intact():
    cfg, _, via, batch = scenes.scene_small_mixed(B=2, footprint="polygon")
    custom = _custom_mixed()
    a = _solver(len(custom) + 40, cfg, batch, 16)
    b = _solver(len(custom) + 40, cfg, batch, 16)
    with pytest.raises(planner.TebAmdError) as e:
        a.set_obstacles_from_costmap((0.0, 0.0, 0.0), 1.5, custom)   # no costmap yet
    assert e.value.code == _abi.ERR_INVALID_ARG
    cells, res, ox, oy = _scene_grid(np.random.default_rng(9), 0.002)
    for s in (a, b):
        s.set_costmap(cells, res, ox, oy)
        s.set_obstacles_from_costmap((0.3, 0.1, 0.2), 1.5, custom)
    full = np.full_like(cells, 254)
    a.set_costmap(full, res, ox, oy)
    n = C.c_int32(-1)
    pose = _abi.f64([0.3, 0.1, 0.2])
    rc = planner.lib().teb_amd_set_obstacles_from_costmap(a._h, _abi._ptr(pose, C.c_double), 1.5, C.byref(custom.freeze()), C.byref(n),
                                                          None, None, 0)
    assert rc == _abi.ERR_CAPACITY
    assert n.value == len(reference_costmap_obstacles(full, res, ox, oy, (0.3, 0.1, 0.2), 1.5)[0])
    M = len(reference_costmap_obstacles(cells, res, ox, oy, (0.3, 0.1, 0.2), 1.5)[0]) + len(custom)
    _assert_same(_state(a, M, batch), _state(b, M, batch))   # as if the failed call had never been made
    # a bad custom table: refused, table intact
    bad = _abi.ObstacleTable(); bad.add_point(1.0, 1.0); bad.type[0] = 9
    with pytest.raises(planner.TebAmdError) as e:
        a.set_obstacles_from_costmap((0.3, 0.1, 0.2), 1.5, bad)
    assert e.value.code == _abi.ERR_INVALID_ARG
    _assert_same(_state(a, M, batch), _state(b, M, batch))
    a.close(); b.close()


def test_free_grid_repeated_calls_and_feasibility():
    cfg, _, via, batch = scenes.scene_small_mixed(B=2, footprint="polygon")
    custom = _custom_mixed()
    fp = [(-0.2, -0.15), (0.4, -0.15), (0.4, 0.15), (-0.2, 0.15)]
    rng = np.random.default_rng(21)
    cells, res, ox, oy = _scene_grid(rng, 0.01)
    a = _solver(len(custom) + 200, cfg, batch, 16)
    b = _solver(len(custom) + 200, cfg, batch, 16)
    # all-free grid: n = 0, the table is the custom table alone
    a.set_costmap(np.zeros_like(cells), res, ox, oy)
    assert a.set_obstacles_from_costmap((0.3, 0.1, 0.2), 1.5, custom)[0] == 0
    b.set_obstacles(custom)
    _assert_same(_state(a, len(custom), batch), _state(b, len(custom), batch))
    # a full grid, then another pose, then a smaller re-set grid: no stale rows of an earlier call
    a.set_costmap(cells, res, ox, oy)
    before = a.is_trajectory_feasible(-1, fp, 0.15)
    a.set_obstacles_from_costmap((0.3, 0.1, 0.2), 1.5, custom)
    after = a.is_trajectory_feasible(-1, fp, 0.15)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])   # the grid is not consumed
    pose = (4.0, -0.3, 2.5)
    n, gx, gy = a.set_obstacles_from_costmap(pose, 0.5, custom)
    xs, ys = reference_costmap_obstacles(cells, res, ox, oy, pose, 0.5)
    assert n == len(xs) and np.array_equal(gx, xs) and np.array_equal(gy, ys)
    b.set_obstacles(_concat(xs, ys, custom))
    _assert_same(_state(a, n + len(custom), batch), _state(b, n + len(custom), batch))
    small = cells[:30, :70].copy()
    a.set_costmap(small, res, ox, oy)
    n, gx, gy = a.set_obstacles_from_costmap(pose, 0.5, custom)
    xs, ys = reference_costmap_obstacles(small, res, ox, oy, pose, 0.5)
    assert n == len(xs) and np.array_equal(gx, xs) and np.array_equal(gy, ys)
    b.set_obstacles(_concat(xs, ys, custom))
    _assert_same(_state(a, n + len(custom), batch), _state(b, n + len(custom), batch))
    a.close(); b.close()
