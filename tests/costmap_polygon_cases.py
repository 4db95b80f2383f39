"""The costmap's lethal cells as convex obstacles (teb_amd_set_obstacles_from_costmap_polygons, include/teb_amd.h): the restatement
the tests compare the device against, and the seeded grids they share. Plain numpy / Python: a breadth-first search per tile and
Andrew's monotone chain on integers. The kept cells and their centres come from the point route's restatement
(tests/test_costmap_obstacles.py), so both routes share one rule and one set of bits."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_costmap_obstacles import reference_costmap_obstacles  # noqa: E402

POINT, LINE, POLYGON = 0, 2, 4   # TEB_AMD_OBST_POINT / _LINE / _POLYGON


def kept_cells(cells, res, ox, oy, pose, dist):
    """{(mx, my): (wx, wy)} of the cells the point route keeps, in its order (mx outer, my inner)."""
    xs, ys = reference_costmap_obstacles(cells, res, ox, oy, pose, dist)
    mx = np.rint((xs - ox) / res - 0.5).astype(np.int64)
    my = np.rint((ys - oy) / res - 0.5).astype(np.int64)
    assert np.array_equal(ox + (mx + 0.5) * res, xs) and np.array_equal(oy + (my + 0.5) * res, ys)   # the indices are exact
    return {(int(a), int(b)): (float(x), float(y)) for a, b, x, y in zip(mx, my, xs, ys)}


def _cross(o, a, b):
    return (a[0] - o[0]) * (b[1] - o[1]) - (a[1] - o[1]) * (b[0] - o[0])


def monotone_chain(points):
    """Andrew's monotone chain on integer points, strict turns only: counter-clockwise from the lexicographically smallest point, no
    repeated closing point; 1 point -> [it], collinear points -> [smallest, largest]."""
    p = sorted(set(points))
    if len(p) <= 1:
        return p
    lower, upper = [], []
    for q in p:
        while len(lower) >= 2 and _cross(lower[-2], lower[-1], q) <= 0:
            lower.pop()
        lower.append(q)
    for q in reversed(p):
        while len(upper) >= 2 and _cross(upper[-2], upper[-1], q) <= 0:
            upper.pop()
        upper.append(q)
    return lower[:-1] + upper[:-1]


def tile_components(kept, tile):
    """[(tile (tx, ty), [cells of one component])] in table order: tiles tx outer, ty inner; inside a tile by the smallest (mx, my)."""
    tiles = {}
    for c in kept:
        tiles.setdefault((c[0] // tile, c[1] // tile), set()).add(c)
    out = []
    for t in sorted(tiles):
        left = set(tiles[t])
        comps = []
        while left:
            seed = min(left)
            left.discard(seed)
            comp, todo = [seed], [seed]
            while todo:
                x, y = todo.pop()
                for dx in (-1, 0, 1):
                    for dy in (-1, 0, 1):
                        n = (x + dx, y + dy)
                        if n in left:
                            left.discard(n)
                            comp.append(n)
                            todo.append(n)
            comps.append(sorted(comp))
        for comp in sorted(comps):
            out.append((t, comp))
    return out


def reference_costmap_polygons(cells, res, ox, oy, pose, dist, tile):
    """The converted rows as a polygon list: (types int32 [n], offset int32 [n + 1], xs, ys float64 [offset[n]]), vertices in the
    order of the rule (point; line from the smallest to the largest (mx, my); counter-clockwise polygon from the smallest vertex)."""
    kept = kept_cells(cells, res, ox, oy, pose, dist)
    types, offset, xs, ys = [], [0], [], []
    for _, comp in tile_components(kept, tile):
        hull = monotone_chain(comp)
        types.append(POINT if len(hull) == 1 else LINE if len(hull) == 2 else POLYGON)
        for v in hull:
            xs.append(kept[v][0]); ys.append(kept[v][1])
        offset.append(len(xs))
    return np.array(types, np.int32), np.array(offset, np.int32), np.array(xs), np.array(ys)


def reference_hulls(cells, res, ox, oy, pose, dist, tile):
    """[(cells of the component, hull vertices as (mx, my))] in table order: what the invariant tests check."""
    kept = kept_cells(cells, res, ox, oy, pose, dist)
    return [(comp, monotone_chain(comp)) for _, comp in tile_components(kept, tile)]


def as_table(offset, xs, ys):
    """The polygon list as the ObstacleTable updateObstacleContainerWithCostmapConverter would build."""
    from teb_local_planner_amd import _abi
    return _abi.ObstacleTable.from_polygon_list(offset, xs, ys)


def structured_grid(rng, n, walls=True, boxes=6, disks=6, noise=0.0):
    """uint8 [n, n] of a seeded indoor map: two-cell room walls with door gaps, boxes, disks (254), on free / inflated background
    values; noise: a fraction of further random lethal cells."""
    cells = rng.integers(0, 253, size=(n, n)).astype(np.uint8)
    cells[cells > 200] = 0
    if walls:
        room = max(n // 4, 12)
        for k in range(room, n - 2, room):
            cells[k:k + 2, :] = 254
            cells[:, k:k + 2] = 254
            for d in range(room // 2, n, room):   # a door in every wall segment
                cells[k:k + 2, d:d + 4] = 0
                cells[d:d + 4, k:k + 2] = 0
    for _ in range(boxes):
        w, h = (int(v) for v in rng.integers(2, max(3, min(n // 10, 40)), 2))
        x, y = (int(v) for v in rng.integers(0, n - 1, 2))
        cells[y:y + h, x:x + w] = 254
    yy, xx = np.mgrid[0:n, 0:n]
    for _ in range(disks):
        r = float(rng.uniform(1.0, max(2.0, min(n / 25, 15.0))))
        cx, cy = rng.uniform(0, n, 2)
        cells[(xx - cx) ** 2 + (yy - cy) ** 2 <= r * r] = 254
    if noise > 0:
        cells[rng.random((n, n)) < noise] = 254
    return cells
