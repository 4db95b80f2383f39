"""The four costmap-to-obstacles entry points (teb_amd_set_obstacles_from_costmap, .._polygons, teb_amd_set_scenes_from_costmaps,
.._costmap_polygons) share one driver and one scratch (csrc/teb_amd.hip, convert_costmaps). What that can newly get wrong is state
carried from one call to the next: here they run interleaved on ONE handle, over grids that grow and shrink between the calls, sets of
1, 3 and 2 scenes and tiles of 1 and 8 cells, and after every call the counts, the out arrays and the behaviour of the installed
table(s) are bit for bit those of the same call made on a fresh handle.

The library has no call that downloads the installed table, so its behaviour stands in for the table state: the out arrays give the
converted rows themselves; the distances from random poses to EVERY row (static and at t = 0.7) read each row's type, points, radius,
velocity and vertices; one optimisation, the selection and the H-signatures read the centroids, the static / dynamic lists and the
layout chosen for the table. A row's bounding radius is read only where a band comes near enough for the far-field test to use it;
the host check of csrc/teb_costmap_host.hpp pins the radii of the tables the conversion builds."""
import functools
import math
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from oracle.oracle_py import Costmap  # noqa: E402
from teb_local_planner_amd import _abi, planner, scenes  # noqa: E402
from teb_local_planner_amd.config import TebConfig  # noqa: E402

pytestmark = pytest.mark.gpu
SINGLE = dict(generic_config_path=True, multi_cu=-1, speculative_trials=-1)   # the fleet contract of include/teb_amd.h
MAX_OBST, MAX_VERTS, STRIDE = 700, 400, 32
DIST = 1.5


@functools.lru_cache(maxsize=None)
def _grid(sx, sy):
    """A 5 cm grid in front of the bands: 1.5 % of the cells lethal, and where there is room a solid box (polygons at tile 8)."""
    rng = np.random.default_rng([991, sx, sy])
    cells = rng.integers(0, 254, size=(sy, sx)).astype(np.uint8)
    cells[rng.random((sy, sx)) < 0.015] = 254
    if sx >= 9 and sy >= 12:
        cells[sy // 2:sy // 2 + 5, sx // 3:sx // 3 + 4] = 254
    if (sx, sy) == (2, 2):
        cells[0, 0] = 254   # the one cell that is visited
    return Costmap(cells, 0.05, 0.4, -0.5 * sy * 0.05)


@functools.lru_cache(maxsize=None)
def _batch():
    cfg = TebConfig()
    cfg.obstacles.include_dynamic_obstacles = True   # signatures with one value per row of the table
    batch = _abi.TebBatchHost(3, STRIDE)
    for b in range(3):
        px, py, th, dt = scenes.sine_band(14 + 3 * b, 3.5, 0.3 - 0.25 * b, 1 + b % 2, cfg.robot.max_vel_x)
        batch.set_teb(b, px, py + 0.2 * (b - 1), th, dt)
    return cfg, batch


def _polygon_custom():
    c = _abi.ObstacleTable()
    c.add_point(1.5, 0.45)
    c.add_polygon([(2.5, -0.5), (3.1, -0.8), (3.0, -0.2)])
    c.add_circle(2.4, 0.9, 0.2, vel=(-0.1, -0.1))
    return c


def _handle():
    cfg, batch = _batch()
    return planner.TebBatchSolver(cfg, batch.count, batch.stride, MAX_OBST, MAX_VERTS, 4, options=_abi.Options(**SINGLE))


def _table(t):
    return tuple(np.asarray(getattr(t, k)) for k in ("type", "ax", "ay", "bx", "by", "vert_offset", "vert_x", "vert_y"))


def _behaviour(s, n_scenes):
    """What the installed table(s) do: distances to every row (single scene), an optimisation, the selection, the signatures."""
    cfg, batch = _batch()
    out = {}
    if n_scenes == 0:
        M = s._n_obst
        rng = np.random.default_rng(11)
        oi = np.repeat(np.arange(M), 2)
        x = rng.uniform(0.0, 4.0, 2 * M); y = rng.uniform(-1.5, 1.5, 2 * M); th = rng.uniform(-math.pi, math.pi, 2 * M)
        if M > 0:
            out["dist"] = (s.debug_distance(oi, x, y, th), s.debug_distance(oi, x, y, th, t=np.full(2 * M, 0.7)))
    else:
        s.set_band_scenes(np.arange(batch.count) % n_scenes)
    s.upload(batch)
    s.optimize(3, 2, compute_cost=True)
    r = s.results()
    b = s.download(batch.copy())
    out["res"] = (r.status, r.lm_iterations, r.lm_trials, r.chi2, r.cost)
    out["band"] = (b.n, b.x, b.y, b.theta, b.dt)
    out["inst"] = (np.array(s.last_instantiation()),)
    if n_scenes == 0:
        out["best"] = (np.array(s.select_best()),)
        out["hsig"] = (s.h_signatures(),)
    else:
        out["best"] = s.select_best_per_scene()
        out["hsig"] = tuple(s.h_signatures_per_scene())
    return out


# one call of an entry point on handle s: the grid(s) first - on the shared handle they replace larger or smaller ones - then the call;
# returns (what the call gave back, the number of scenes installed: 0 = the single scene)
def _single_points(shape, custom=None):
    def call(s):
        g = _grid(*shape)
        s.clear_scenes()
        s.set_costmap(g.cells, g.resolution, g.origin_x, g.origin_y)
        n, xs, ys = s.set_obstacles_from_costmap((0.0, 0.0, 0.2), DIST, custom)
        return (np.array(n), xs, ys), 0
    return call


def _single_polygons(shape, tile, custom=None):
    def call(s):
        g = _grid(*shape)
        s.clear_scenes()
        s.set_costmap(g.cells, g.resolution, g.origin_x, g.origin_y)
        return _table(s.set_obstacles_from_costmap_polygons((0.0, 0.0, 0.2), DIST, tile, custom)), 0
    return call


def _poses(n):
    return [(0.1 * k, 0.05 * k, 0.2 - 0.3 * k) for k in range(n)]


def _set_points(shapes, customs=None, vias=None):
    def call(s):
        s.set_costmaps([_grid(*q) for q in shapes])
        n, pts = s.set_scenes_from_costmaps(_poses(len(shapes)), DIST, customs, vias)
        return (n,) + tuple(a for p in pts for a in p), len(shapes)
    return call


def _set_polygons(shapes, tiles, customs=None, vias=None):
    def call(s):
        s.set_costmaps([_grid(*q) for q in shapes])
        tabs = s.set_scenes_from_costmap_polygons(_poses(len(shapes)), DIST, tiles, customs, vias)
        return tuple(a for t in tabs for a in _table(t)), len(shapes)
    return call


def _bits(v):
    a = np.ascontiguousarray(np.asarray(v))
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _leaves(v):
    return [a for u in v for a in _leaves(u)] if isinstance(v, (tuple, list)) else [v]


def _same(u, v, what):
    u, v = _leaves(u), _leaves(v)
    assert len(u) == len(v), what
    for p, q in zip(u, v):
        p, q = _bits(p), _bits(q)
        assert p.shape == q.shape and np.array_equal(p, q), what


def test_interleaved_calls_on_one_handle_equal_fresh_handles():
    vias3 = [[(1.0, 0.2)], [], [(2.0, -0.1), (3.0, 0.1)]]
    steps = [
        ("points 120x120", _single_points((120, 120))),
        ("polygons 120x120 tile 8", _single_polygons((120, 120), 8, _polygon_custom())),
        ("points 2x2", _single_points((2, 2))),
        ("set of 3, points", _set_points([(63, 65), (1, 37), (9, 12)], [None, None, _polygon_custom()], vias3)),
        ("set of 3, polygons, tiles 8 1 8", _set_polygons([(63, 65), (1, 37), (9, 12)], [8, 1, 8], [None, None, _polygon_custom()], vias3)),
        ("polygons 1x37 tile 1", _single_polygons((1, 37), 1)),
        ("polygons 63x65 tile 8", _single_polygons((63, 65), 8)),
        ("set of 1, polygons, tile 1", _set_polygons([(120, 120)], 1)),
        ("set of 2, points", _set_points([(2, 2), (120, 120)])),
        ("set of 2, polygons, tiles 1 8", _set_polygons([(120, 120), (9, 12)], [1, 8], [_polygon_custom(), None])),
        ("polygons 9x12 tile 1", _single_polygons((9, 12), 1, _polygon_custom())),
        ("points 9x12", _single_points((9, 12), _polygon_custom())),
        ("points 120x120 again", _single_points((120, 120))),
        ("set of 3, polygons, tile 8", _set_polygons([(9, 12), (63, 65), (2, 2)], 8)),
    ]
    shared = _handle()
    for name, call in steps:
        fresh = _handle()
        got, ns = call(shared)
        want, _ = call(fresh)
        _same(got, want, name + ": counts / out arrays")
        a, b = _behaviour(shared, ns), _behaviour(fresh, ns)
        assert a.keys() == b.keys()
        for k in a:
            _same(a[k], b[k], "%s: %s" % (name, k))
        fresh.close()
    shared.close()
