"""Fixtures for the polygon route of the costmap per scene (teb_amd_set_scenes_from_costmap_polygons, include/teb_amd.h):
tests/test_fleet_polygon_cases.py holds them to the restatement on the CPU, tests/test_gpu_fleet_polygons.py runs them on the device.

  polygon_set(name)   a costmap set with a tile size per scene, robot poses, a behind-robot distance, custom rows and bands.

The shapes are the smallest at which the indexing of the scene-set kernels can go wrong (SET_SHAPES). Everything is seeded and built once
per process (functools.lru_cache); the tests do not change what they get."""
import functools

import numpy as np

from oracle.oracle_py import Costmap
from teb_local_planner_amd import _abi, scenes
from teb_local_planner_amd.config import TebConfig

import costmap_polygon_cases as CP
import fleet_tick_cases as FT

# (size_x, size_y, tile) of every scene
SET_SHAPES = {
    "one": [(63, 65, 8)],                                                        # a single scene, a single block column run
    # two adjacent scenes without blocks first and one last; T = 64 on 65 x 129 visited cells: 2 x 3 blocks with k = 1 and clipped tiles
    # (nby > 1); one visited cell under T = 64; T = 3 does not divide 4096 (k = 455)
    "edges": [(1, 37, 8), (41, 1, 1), (66, 130, 64), (2, 2, 64), (120, 120, 3), (33, 1, 16)],
    "mixed": [(120, 120, 8), (120, 120, 1), (90, 50, 2), (120, 120, 16)],        # scene 1 all free: blocks but no rows, between scenes with rows
}
SET_DIST = {"one": -1.0, "edges": 1.5, "mixed": float("inf")}
SET_FREE = {"one": [], "edges": [], "mixed": [1]}
SET_NO_BLOCKS = {"one": [], "edges": [0, 1, 5], "mixed": []}
SET_CUSTOM = {"one": {0: "pointlike"}, "edges": {1: "mixed", 2: "pointlike", 4: "mixed"}, "mixed": {0: "mixed", 1: "pointlike"}}
STRIDE = 48


def block_rule(size_x, size_y, tile):
    """(ncols, nrows, k, nty, nby, blocks) of teb_amd_set_obstacles_from_costmap_polygons on a grid: k = 4096 / T^2 tiles of one tile
    column per block (csrc/teb_costmap_polygons.hpp)."""
    ncols, nrows = size_x - 1, size_y - 1
    k = 4096 // (tile * tile)
    if ncols <= 0 or nrows <= 0:
        return ncols, nrows, k, 0, 0, 0
    nty = (nrows + tile - 1) // tile
    nby = (nty + k - 1) // k
    return ncols, nrows, k, nty, nby, ((ncols + tile - 1) // tile) * nby


class PolygonSet(FT.TableSet):
    """FT.TableSet + tiles [n]: the tile size of every scene"""

    def __init__(self, tiles, *a):
        super().__init__(*a)
        self.tiles = np.asarray(tiles, np.int32)


def _cells(rng, sx, sy, free):
    if min(sx, sy) >= 24:   # walls, boxes, disks and 2 % noise: rows of all three kinds
        n = max(sx, sy)
        cells = CP.structured_grid(rng, n, noise=0.0 if free else 0.02)[:sy, :sx].copy()
        if free:
            cells[cells == 254] = 0
    else:
        cells = rng.integers(0, 253, size=(sy, sx)).astype(np.uint8)
        if not free:
            cells[rng.random((sy, sx)) < 0.125] = 254
    flat = cells.reshape(-1)
    spots = rng.permutation(cells.size)[:min(6, cells.size // 2)]              # neither 253 nor 255 is an obstacle
    flat[spots[::2]] = 253
    flat[spots[1::2]] = 255
    if (sx, sy) == (2, 2):
        cells[0, 0], cells[0, 1], cells[1, 0] = 254, 253, 255                  # (0, 0) is the one cell the reference visits
    return cells


@functools.lru_cache(maxsize=None)
def polygon_set(name):
    shapes = SET_SHAPES[name]
    rng = np.random.default_rng([7321, sorted(SET_SHAPES).index(name)])
    cfg = TebConfig()
    cfg.obstacles.include_dynamic_obstacles = True
    grids, poses, customs = [], [], []
    for s, (sx, sy, _) in enumerate(shapes):
        res = 0.05 if (sx, sy) == (120, 120) else float(rng.uniform(0.03, 0.12))
        ox, oy = float(rng.uniform(-20, 20)), float(rng.uniform(-20, 20))       # every robot somewhere else on the floor
        grids.append(Costmap(_cells(rng, sx, sy, s in SET_FREE[name]), res, ox, oy))
        poses.append((ox + 0.2 * sx * res, oy + 0.5 * sy * res, float(rng.uniform(-0.4, 0.4))))   # the robot inside its grid
        kind = SET_CUSTOM[name].get(s)
        customs.append(None if kind is None else (FT.custom_mixed if kind == "mixed" else FT.custom_pointlike)(poses[-1][0], poses[-1][1]))
    counts = [1 + (s % 2) for s in range(len(shapes))]
    scene_of = np.repeat(np.arange(len(shapes)), counts)
    rng.shuffle(scene_of)
    batch = _abi.TebBatchHost(len(scene_of), STRIDE)
    for b, s in enumerate(scene_of):
        n = int(rng.integers(12, 21))
        px, py, th, dt = scenes.sine_band(n, 3.5, float(rng.uniform(-0.4, 0.4)), float(rng.integers(1, 3)), cfg.robot.max_vel_x)
        th = th + rng.normal(0.0, 2e-3, th.shape)
        batch.set_teb(b, px + poses[s][0], py + poses[s][1], th, dt)
    return PolygonSet([t for _, _, t in shapes], name, cfg, grids, np.array(poses), SET_DIST[name], customs, batch, scene_of)


def polygon_sets():
    return [polygon_set(k) for k in SET_SHAPES]


@functools.lru_cache(maxsize=None)
def expected_rows(name, turned=0.0, tile=None):
    """[(types, offset, xs, ys)] per scene: the restatement on grid s with pose s (heading + turned) and tile s (or `tile` everywhere)."""
    t = polygon_set(name)
    out = []
    for s, g in enumerate(t.grids):
        pose = (t.poses[s][0], t.poses[s][1], t.poses[s][2] + turned)
        out.append(CP.reference_costmap_polygons(g.cells, g.resolution, g.origin_x, g.origin_y, pose, t.dist, int(t.tiles[s]) if tile is None else tile))
    return out


def concat_table(rows, custom):
    """The table teb_amd_set_scenes gets for a scene: the converted rows (a polygon list), then the custom rows."""
    _, off, xs, ys = rows
    t = CP.as_table(off, xs, ys)
    if custom is not None:
        base = t.vert_offset[-1]
        for k in ("type", "ax", "ay", "bx", "by", "radius", "vx", "vy", "dynamic", "vert_x", "vert_y"):
            getattr(t, k).extend(getattr(custom, k))
        t.vert_offset.extend(base + v for v in custom.vert_offset[1:])
    return t
