"""The costmap's lethal cells as convex obstacles (teb_amd_set_obstacles_from_costmap_polygons): hand-worked answers and invariants of
the restatement in tests/costmap_polygon_cases.py, and the CPU-side parts of the entry point (export, argument check). No GPU needed."""
import ctypes as C
import math

import numpy as np
import pytest

from costmap_polygon_cases import (LINE, POINT, POLYGON, kept_cells, monotone_chain, reference_costmap_polygons, reference_hulls,
                                   structured_grid)
from teb_local_planner_amd import _abi, planner
from test_costmap_obstacles import reference_costmap_obstacles

INF = math.inf
FAR = (-100.0, -100.0, 0.0)   # a pose that keeps every cell (the filter is off at dist = inf anyway)


def _grid(n, cells):
    g = np.zeros((n, n), np.uint8)
    for mx, my in cells:
        g[my, mx] = 254
    return g


def _rows(g, tile):
    """[(type, [(mx, my) ..])] of the unit grid (resolution 1, origin -0.5: centres at the cell indices)."""
    types, off, xs, ys = reference_costmap_polygons(g, 1.0, -0.5, -0.5, FAR, INF, tile)
    return [(int(types[i]), [(int(x), int(y)) for x, y in zip(xs[off[i]:off[i + 1]], ys[off[i]:off[i + 1]])]) for i in range(len(types))]


def test_single_cell_is_a_point():
    assert _rows(_grid(6, [(2, 3)]), 8) == [(POINT, [(2, 3)])]


def test_runs_are_lines_from_smallest_to_largest():
    assert _rows(_grid(10, [(1, 4), (2, 4), (3, 4), (4, 4)]), 8) == [(LINE, [(1, 4), (4, 4)])]      # horizontal
    assert _rows(_grid(10, [(5, 1), (5, 2), (5, 3)]), 8) == [(LINE, [(5, 1), (5, 3)])]              # vertical
    assert _rows(_grid(10, [(4, 1), (3, 2), (2, 3), (1, 4)]), 8) == [(LINE, [(1, 4), (4, 1)])]      # anti-diagonal
    assert _rows(_grid(10, [(1, 1), (2, 2), (3, 3)]), 8) == [(LINE, [(1, 1), (3, 3)])]              # diagonal
    assert _rows(_grid(10, [(2, 2), (3, 2)]), 8) == [(LINE, [(2, 2), (3, 2)])]                      # two cells


def test_block_is_a_ccw_square_and_tromino_a_triangle():
    assert _rows(_grid(6, [(1, 1), (2, 1), (1, 2), (2, 2)]), 8) == [(POLYGON, [(1, 1), (2, 1), (2, 2), (1, 2)])]
    assert _rows(_grid(6, [(1, 1), (1, 2), (2, 1)]), 8) == [(POLYGON, [(1, 1), (2, 1), (1, 2)])]
    # a collinear cell on an edge is no vertex: a 3 x 2 block has 4 vertices
    assert _rows(_grid(6, [(x, y) for x in (1, 2, 3) for y in (1, 2)]), 8) == [(POLYGON, [(1, 1), (3, 1), (3, 2), (1, 2)])]


def test_checkerboard_is_one_component():
    cb = [(x, y) for x in range(8) for y in range(8) if (x + y) % 2 == 0]
    rows = _rows(_grid(9, cb), 8)
    assert len(rows) == 1 and rows[0] == (POLYGON, [(0, 0), (6, 0), (7, 1), (7, 7), (1, 7), (0, 6)])


def test_wall_across_a_tile_border_gives_two_rows_in_tile_order():
    wall = [(x, 5) for x in range(2, 13)]              # tiles of 8: columns 2 .. 7 and 8 .. 12
    assert _rows(_grid(16, wall), 8) == [(LINE, [(2, 5), (7, 5)]), (LINE, [(8, 5), (12, 5)])]
    two = [(1, 9), (1, 2)]                              # one tile column: ty 0 before ty 1
    assert _rows(_grid(16, two), 8) == [(POINT, [(1, 2)]), (POINT, [(1, 9)])]
    same = [(5, 1), (1, 6), (2, 6)]                     # one tile: by the smallest (mx, my), (1, 6) first
    assert _rows(_grid(16, same), 8) == [(LINE, [(1, 6), (2, 6)]), (POINT, [(5, 1)])]


def test_last_row_and_column_and_values_are_the_point_routes():
    g = _grid(5, [(4, 1), (1, 4), (2, 2)])              # (4, 1) and (1, 4) lie in the last column / row: never visited
    g[1, 1] = 253
    g[3, 3] = 255
    assert _rows(g, 8) == [(POINT, [(2, 2)])]


def test_monotone_chain_degenerate_inputs():
    assert monotone_chain([]) == [] and monotone_chain([(3, 4), (3, 4)]) == [(3, 4)]
    assert monotone_chain([(0, 0), (2, 2), (1, 1), (3, 3)]) == [(0, 0), (3, 3)]


def _seeded(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(5, 70))
    cells = structured_grid(rng, n, walls=bool(seed % 2), noise=float(rng.choice([0.0, 0.05, 0.2])))
    res, ox, oy = float(rng.uniform(0.02, 0.2)), float(rng.uniform(-5, 1)), float(rng.uniform(-5, 1))
    pose = (ox + rng.uniform(0, n * res), oy + rng.uniform(0, n * res), rng.uniform(-4, 4))
    dist = float(rng.choice([-1.0, 0.0, 1.5, INF]))
    return cells, res, ox, oy, pose, dist


@pytest.mark.parametrize("seed", range(12))
def test_tile_one_is_the_point_route(seed):
    cells, res, ox, oy, pose, dist = _seeded(seed)
    types, off, xs, ys = reference_costmap_polygons(cells, res, ox, oy, pose, dist, 1)
    px, py = reference_costmap_obstacles(cells, res, ox, oy, pose, dist)
    assert np.all(types == POINT) and np.array_equal(off, np.arange(len(px) + 1))
    assert np.array_equal(xs, px) and np.array_equal(ys, py)


def _in_closed_hull(p, hull):
    if len(hull) == 1:
        return p == hull[0]
    if len(hull) == 2:
        a, b = hull
        return (b[0] - a[0]) * (p[1] - a[1]) - (b[1] - a[1]) * (p[0] - a[0]) == 0 and \
            min(a[0], b[0]) <= p[0] <= max(a[0], b[0]) and min(a[1], b[1]) <= p[1] <= max(a[1], b[1])
    return all((b[0] - a[0]) * (p[1] - a[1]) - (b[1] - a[1]) * (p[0] - a[0]) >= 0 for a, b in zip(hull, hull[1:] + hull[:1]))


@pytest.mark.parametrize("seed", range(12))
@pytest.mark.parametrize("tile", [2, 3, 8, 16, 64])
def test_invariants_on_seeded_grids(seed, tile):
    cells, res, ox, oy, pose, dist = _seeded(100 + seed)
    kept = kept_cells(cells, res, ox, oy, pose, dist)
    hulls = reference_hulls(cells, res, ox, oy, pose, dist, tile)
    assert sorted(c for comp, _ in hulls for c in comp) == sorted(kept)          # every kept cell in exactly one row
    for comp, hull in hulls:
        tiles = {(c[0] // tile, c[1] // tile) for c in comp}
        assert len(tiles) == 1                                                     # components never cross a tile border
        assert set(hull) <= set(comp)                                              # vertices are kept cells of that tile
        assert hull[0] == min(hull)                                                # starts at the smallest vertex
        assert all(_in_closed_hull(c, hull) for c in comp)                         # every kept centre lies in its row's hull
        if len(hull) >= 3:                                                         # strictly convex, counter-clockwise
            for a, b, c in zip(hull, hull[1:] + hull[:1], hull[2:] + hull[:2]):
                assert (b[0] - a[0]) * (c[1] - b[1]) - (b[1] - a[1]) * (c[0] - b[0]) > 0
    types, off, xs, ys = reference_costmap_polygons(cells, res, ox, oy, pose, dist, tile)
    assert len(types) == len(hulls) and off[-1] == len(xs) == sum(len(h) for _, h in hulls)
    for i, (_, hull) in enumerate(hulls):                                          # world coordinates: the point route's centres
        assert [(xs[k], ys[k]) for k in range(off[i], off[i + 1])] == [kept[v] for v in hull]


def test_library_exports_the_entry_point_and_rejects_a_null_handle():
    L = planner.lib()
    assert hasattr(L, "teb_amd_set_obstacles_from_costmap_polygons")
    pose = _abi.f64([0.0, 0.0, 0.0])
    n_o, n_p = C.c_int32(-7), C.c_int32(-9)
    rc = L.teb_amd_set_obstacles_from_costmap_polygons(None, _abi._ptr(pose, C.c_double), 1.5, 8, None, C.byref(n_o), C.byref(n_p),
                                                       None, None, None, 0, 0)
    assert rc == _abi.ERR_INVALID_ARG
    assert n_o.value == -7 and n_p.value == -9   # nothing counted, nothing written
