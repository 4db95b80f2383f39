"""teb_amd_set_obstacles_from_costmap_polygons on the device: the converted rows bit for bit against the restatement of
tests/costmap_polygon_cases.py, and a handle that got its table this way behaves exactly like one that got the same table through
teb_amd_set_obstacles (and, at one cell per tile, like one fed by the point route)."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from costmap_polygon_cases import POLYGON, as_table, reference_costmap_polygons, reference_hulls, structured_grid  # noqa: E402
from test_gpu_costmap_obstacles import (DISTS, SHAPES, _assert_same, _custom_mixed, _grid, _scene_grid, _solver,  # noqa: E402
                                        _state)
from teb_local_planner_amd import _abi, planner, scenes  # noqa: E402

pytestmark = pytest.mark.gpu

TILES = [1, 2, 3, 8, 16, 64]


def _raw(s, pose, dist, tile, custom=None, cap_o=None, cap_p=None):
    """The C entry point itself: (rc, n_obstacles, n_points, offset, xs, ys)."""
    cap_o = s.max_obstacles if cap_o is None else cap_o
    cap_p = 2 * s.max_obstacles + s.max_obstacle_vertices if cap_p is None else cap_p
    p = _abi.f64([float(v) for v in pose])
    n_o, n_p = C.c_int32(-1), C.c_int32(-1)
    off = np.full(max(cap_o, 0) + 1, -5, np.int32)
    xs = np.full(max(cap_p, 1), np.nan); ys = np.full(max(cap_p, 1), np.nan)
    rc = planner.lib().teb_amd_set_obstacles_from_costmap_polygons(
        s._h, _abi._ptr(p, C.c_double), float(dist), int(tile), C.byref(custom.freeze()) if custom is not None else None,
        C.byref(n_o), C.byref(n_p), _abi._ptr(off, C.c_int32), _abi._ptr(xs, C.c_double), _abi._ptr(ys, C.c_double), cap_o, cap_p)
    return rc, n_o.value, n_p.value, off, xs, ys


def _bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _tables_equal(t, u):
    for k in ("type", "dynamic", "vert_offset"):
        if list(getattr(t, k)) != list(getattr(u, k)):
            return False
    return all(_bits_equal(np.array(getattr(t, k), np.float64), np.array(getattr(u, k), np.float64))
               for k in ("ax", "ay", "bx", "by", "radius", "vx", "vy", "vert_x", "vert_y"))


def _join(t, custom):
    """The table teb_amd_set_obstacles gets: the converted rows, then the custom rows (their vertex offsets shifted)."""
    u = _abi.ObstacleTable()
    for k in ("type", "ax", "ay", "bx", "by", "radius", "vx", "vy", "dynamic", "vert_x", "vert_y"):
        getattr(u, k).extend(getattr(t, k))
    u.vert_offset = list(t.vert_offset)
    if custom is not None:
        for k in ("type", "ax", "ay", "bx", "by", "radius", "vx", "vy", "dynamic", "vert_x", "vert_y"):
            getattr(u, k).extend(getattr(custom, k))
        u.vert_offset.extend(v + t.vert_offset[-1] for v in custom.vert_offset[1:])
    return u


def _poly_verts(types, off):
    return int(sum(off[i + 1] - off[i] for i in range(len(types)) if types[i] == POLYGON))


def _case(seed):
    rng = np.random.default_rng(9000 + seed)
    sx, sy = SHAPES[seed % len(SHAPES)]
    tile = TILES[seed % len(TILES)]
    dist = DISTS[seed % len(DISTS)]
    if (seed // len(SHAPES)) % 2:   # structured: walls, boxes, disks (cropped to the shape)
        n = max(sx, sy)
        cells = structured_grid(rng, n, walls=n >= 24, noise=0.02 if n < 1000 else 0.0)[:sy, :sx].copy()
    else:
        big = sx * sy >= 1000 * 1000
        cells = _grid(rng, sx, sy, [0.01, 0.045][seed % 2] if big else [0.02, 0.1, 0.3][seed % 3])
    res = float(rng.uniform(0.02, 0.2)); ox, oy = float(rng.uniform(-20, 5)), float(rng.uniform(-20, 5))
    pose = (ox + rng.uniform(0, sx * res), oy + rng.uniform(0, sy * res), rng.uniform(-4, 4))
    return cells, res, ox, oy, pose, dist, tile


@pytest.mark.parametrize("seed", range(42))
def test_rows_bit_for_bit(seed):
    cells, res, ox, oy, pose, dist, tile = _case(seed)
    types, off, xs, ys = reference_costmap_polygons(cells, res, ox, oy, pose, dist, tile)
    assert len(types) <= 60000
    s = _solver(len(types), max_verts=_poly_verts(types, off))
    s.set_costmap(cells, res, ox, oy)
    rc, n_o, n_p, goff, gx, gy = _raw(s, pose, dist, tile)
    assert rc == _abi.OK, planner.lib().teb_amd_last_error()
    assert (n_o, n_p) == (len(types), len(xs))
    assert np.array_equal(goff[:n_o + 1], off)
    assert _bits_equal(gx[:n_p], xs) and _bits_equal(gy[:n_p], ys)
    t = s.set_obstacles_from_costmap_polygons(pose, dist, tile)   # the binding: the same rows as an ObstacleTable
    assert list(t.type) == types.tolist() and _tables_equal(t, as_table(off, xs, ys))
    s.close()


def test_out_arrays_only_when_both_capacities_suffice():
    cells, res, ox, oy = _scene_grid(np.random.default_rng(4), 0.02)
    types, off, xs, ys = reference_costmap_polygons(cells, res, ox, oy, (0.3, 0.1, 0.2), 1.5, 4)
    s = _solver(len(types), max_verts=_poly_verts(types, off))
    s.set_costmap(cells, res, ox, oy)
    for cap_o, cap_p in ((len(types) - 1, len(xs)), (len(types), len(xs) - 1)):
        rc, n_o, n_p, goff, gx, gy = _raw(s, (0.3, 0.1, 0.2), 1.5, 4, cap_o=cap_o, cap_p=cap_p)
        assert rc == _abi.OK and (n_o, n_p) == (len(types), len(xs))
        assert np.all(goff == -5) and np.all(np.isnan(gx))   # counts reported, nothing written
    rc, n_o, n_p, goff, gx, gy = _raw(s, (0.3, 0.1, 0.2), 1.5, 4, cap_o=len(types), cap_p=len(xs))
    assert rc == _abi.OK and np.array_equal(goff, off) and _bits_equal(gx, xs) and _bits_equal(gy, ys)
    s.close()


@pytest.mark.parametrize("footprint", ["circular", "polygon"])
def test_tile_one_is_the_point_route(footprint):
    cfg, _, via, batch = scenes.scene_small_mixed(B=4, footprint=footprint)
    cells, res, ox, oy = _scene_grid(np.random.default_rng(3), 0.03)
    custom = _custom_mixed()
    n = len(reference_costmap_polygons(cells, res, ox, oy, (0.3, 0.1, 0.2), 1.5, 1)[0])
    M = n + len(custom)
    a = _solver(M, cfg, batch, 16)
    b = _solver(M, cfg, batch, 16)
    for s in (a, b):
        s.set_costmap(cells, res, ox, oy)
        s.set_via_points(via)
    t = a.set_obstacles_from_costmap_polygons((0.3, 0.1, 0.2), 1.5, 1, custom)
    assert len(t) == n and b.set_obstacles_from_costmap((0.3, 0.1, 0.2), 1.5, custom)[0] == n
    _assert_same(_state(a, M, batch), _state(b, M, batch))
    a.close(); b.close()


def _scene_cells(seed):
    """Structured 5 cm cells over the bands of scenes.scene_small_mixed (x -0.5 .. 6.5, y -1.5 .. 1.5)."""
    rng = np.random.default_rng(seed)
    cells = structured_grid(rng, 140, walls=False, boxes=14, disks=10)[40:100, :].copy()
    return cells, 0.05, -0.5, -1.5


@pytest.mark.parametrize("B", [1, 8])
def test_same_handle_as_set_obstacles_mixed_table(B):
    cfg, _, via, batch = scenes.scene_small_mixed(B=B, footprint="polygon")
    cells, res, ox, oy = _scene_cells(B)
    custom = _custom_mixed()
    pose, dist, tile = (0.3, 0.1, 0.2), 1.5, 8
    types, off, xs, ys = reference_costmap_polygons(cells, res, ox, oy, pose, dist, tile)
    assert np.any(types == POLYGON) and len(types) >= 10
    M = len(types) + len(custom)
    mv = _poly_verts(types, off) + len(custom.vert_x)
    a = _solver(M, cfg, batch, mv)
    b = _solver(M, cfg, batch, mv)
    a.set_costmap(cells, res, ox, oy)
    t = a.set_obstacles_from_costmap_polygons(pose, dist, tile, custom)
    assert _tables_equal(t, as_table(off, xs, ys))
    b.set_obstacles(_join(t, custom))
    for s in (a, b):
        s.set_via_points(via)
    _assert_same(_state(a, M, batch), _state(b, M, batch))
    cfg.obstacles.include_dynamic_obstacles = not cfg.obstacles.include_dynamic_obstacles
    a.set_config(cfg); b.set_config(cfg)
    _assert_same(_state(a, M, batch), _state(b, M, batch))
    a.close(); b.close()


def _outside(qx, qy, hull):
    """(qx, qy) in cell-index coordinates strictly outside the closed hull (polygons only; points and lines have no inside)."""
    if len(hull) < 3:
        return True
    return any((b[0] - a[0]) * (qy - a[1]) - (b[1] - a[1]) * (qx - a[0]) < -1e-9 for a, b in zip(hull, hull[1:] + hull[:1]))


@pytest.mark.parametrize("tile", [2, 4, 8, 16])
def test_distances_cover_the_cells(tile):
    """Point footprint: the nearest converted row is never farther than the nearest kept cell centre, and nearer by at most the
    diagonal of a tile's cell centres."""
    cfg, _, _, _ = scenes.scene_c1()
    rng = np.random.default_rng(50 + tile)
    cells = structured_grid(rng, 120, walls=True, noise=0.01)
    res, ox, oy = 0.05, -3.0, -3.0
    pose, dist = (0.0, 0.0, 0.0), math.inf
    hulls = reference_hulls(cells, res, ox, oy, pose, dist, tile)
    n_pts = sum(len(c) for c, _ in hulls)
    types, off, _, _ = reference_costmap_polygons(cells, res, ox, oy, pose, dist, tile)
    a = _solver(len(types), cfg, max_verts=_poly_verts(types, off))
    p = _solver(n_pts, cfg)
    for s in (a, p):
        s.set_costmap(cells, res, ox, oy)
    assert len(a.set_obstacles_from_costmap_polygons(pose, dist, tile)) == len(types)
    assert p.set_obstacles_from_costmap(pose, dist)[0] == n_pts
    q = []
    while len(q) < 48:
        x, y = rng.uniform(-3.2, 3.2, 2)
        ix, iy = (x - ox) / res - 0.5, (y - oy) / res - 0.5
        if all(_outside(ix, iy, h) for _, h in hulls):
            q.append((x, y))
    q = np.array(q)

    def nearest(s, m):
        oi = np.tile(np.arange(m), len(q))
        d = s.debug_distance(oi, np.repeat(q[:, 0], m), np.repeat(q[:, 1], m), np.zeros(m * len(q)))[0]
        return d.reshape(len(q), m).min(axis=1)
    d_conv, d_pts = nearest(a, len(types)), nearest(p, n_pts)
    assert np.all(d_conv <= d_pts + 1e-12), (d_conv - d_pts).max()
    assert np.all(d_conv >= d_pts - (tile - 1) * math.sqrt(2.0) * res - 1e-12), (d_pts - d_conv).max()
    a.close(); p.close()


def test_errors_leave_the_table_intact():
    cfg, _, via, batch = scenes.scene_small_mixed(B=2, footprint="polygon")
    custom = _custom_mixed()
    a = _solver(len(custom) + 40, cfg, batch, 16)
    b = _solver(len(custom) + 40, cfg, batch, 16)
    with pytest.raises(planner.TebAmdError) as e:
        a.set_obstacles_from_costmap_polygons((0.0, 0.0, 0.0), 1.5, 8, custom)   # no costmap yet
    assert e.value.code == _abi.ERR_INVALID_ARG
    cells = np.zeros((60, 140), np.uint8)
    cells[5, 57:63] = 254                                      # a line
    for x, y in ((20, 30), (50, 10)):                          # and two 2 x 2 blocks: 3 rows, 8 polygon vertices
        cells[y:y + 2, x:x + 2] = 254
    res, ox, oy = 0.05, -0.5, -1.5
    pose = (0.3, 0.1, 0.2)
    for s in (a, b):
        s.set_costmap(cells, res, ox, oy)
        s.set_obstacles_from_costmap_polygons(pose, 1.5, 8, custom)
    M = 3 + len(custom)

    def unchanged():
        _assert_same(_state(a, M, batch), _state(b, M, batch))

    for tile in (0, 65, -1):   # tile outside 1 .. 64
        rc, n_o, n_p, *_ = _raw(a, pose, 1.5, tile, custom)
        assert rc == _abi.ERR_INVALID_ARG and n_o == -1 and n_p == -1
    rc, *_ = _raw(a, pose, 1.5, 8, custom, cap_o=-1)           # a negative capacity
    assert rc == _abi.ERR_INVALID_ARG
    n_o = C.c_int32(-1)
    rc = planner.lib().teb_amd_set_obstacles_from_costmap_polygons(a._h, None, 1.5, 8, None, C.byref(n_o), None, None, None, None, 0, 0)
    assert rc == _abi.ERR_INVALID_ARG and n_o.value == -1      # a null pose
    bad = _abi.ObstacleTable(); bad.add_point(1.0, 1.0); bad.type[0] = 9
    with pytest.raises(planner.TebAmdError) as e:
        a.set_obstacles_from_costmap_polygons(pose, 1.5, 8, bad)   # a bad custom table
    assert e.value.code == _abi.ERR_INVALID_ARG
    unchanged()
    # too many rows: a full grid at one cell per tile
    full = np.full_like(cells, 254)
    a.set_costmap(full, res, ox, oy)
    rc, n_o, n_p, goff, gx, _ = _raw(a, pose, 1.5, 1, custom)
    assert rc == _abi.ERR_CAPACITY
    n_want = len(reference_costmap_polygons(full, res, ox, oy, pose, 1.5, 1)[0])
    assert n_o == n_want and n_p == n_want and np.all(goff == -5) and np.all(np.isnan(gx))
    unchanged()
    # too many polygon vertices: rows fit (5 + 7 <= 47), vertices do not (4 blocks: 16 + 3 > 16)
    more = cells.copy()
    for x, y in ((80, 40), (110, 25)):
        more[y:y + 2, x:x + 2] = 254
    a.set_costmap(more, res, ox, oy)
    rc, n_o, n_p, *_ = _raw(a, pose, 1.5, 8, custom)
    assert rc == _abi.ERR_CAPACITY and (n_o, n_p) == (5, 18)
    unchanged()
    # a free grid: the custom table alone
    a.set_costmap(np.zeros_like(cells), res, ox, oy)
    assert len(a.set_obstacles_from_costmap_polygons(pose, 1.5, 8, custom)) == 0
    b.set_obstacles(custom)
    _assert_same(_state(a, len(custom), batch), _state(b, len(custom), batch))
    a.close(); b.close()
