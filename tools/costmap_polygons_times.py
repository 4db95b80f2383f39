#!/usr/bin/env python3
"""set_obstacles_from_costmap_polygons (the costmap's lethal cells as convex points / lines / polygons, converted on the device) against
set_obstacles_from_costmap (one point per cell) on seeded 5 cm maps: 120^2, 400^2, 1000^2 indoor maps (two-cell room walls with doors,
boxes, disks: tests/costmap_polygon_cases.py structured_grid) and the random grids of tools/costmap_obstacles_times.py (2 % and 10 %
lethal). Per case one line for the point route and one per tile size T in {1, 4, 8, 16, 32}: rows, vertices and polygon vertices
against the point count, median wall ms of the C call (call_ms: from the grid already on the device to the installed table) and of the
Python binding (binding_ms: + the ObstacleTable it returns), and - up to 20 000 rows - the optimise kernel ms (median of 5 launches) of
one 100-pose band over that table with the instantiation it took (last_instantiation: layout, Jacobian mode, scene kind). One JSON
line each; the first line carries the binary hash of the library.

    python tools/costmap_polygons_times.py [--reps 21] [--tiles 1 4 8 16 32] [--grids 120 400 1000]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from teb_local_planner_amd import _abi, planner, scenes  # noqa: E402
from teb_local_planner_amd.config import TebConfig  # noqa: E402
from costmap_polygon_cases import structured_grid  # noqa: E402


def _median_ms(fn, reps):
    fn()   # warm-up (first launch of the kernels, allocations)
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); ts.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(ts))


def _c_call(s, pose, dist, T=None):
    """The C entry point alone, with its out arrays (what a C++ binding pays); T = None: the point route."""
    p = _abi.f64([float(v) for v in pose])
    cap_o = s.max_obstacles
    cap_p = 2 * cap_o + s.max_obstacle_vertices
    off = np.zeros(cap_o + 1, np.int32); xs = np.zeros(cap_p); ys = np.zeros(cap_p)
    n_o, n_p = C.c_int32(0), C.c_int32(0)
    if T is None:
        f = planner.lib().teb_amd_set_obstacles_from_costmap
        args = (s._h, _abi._ptr(p, C.c_double), float(dist), None, C.byref(n_o), _abi._ptr(xs, C.c_double), _abi._ptr(ys, C.c_double), cap_o)
    else:
        f = planner.lib().teb_amd_set_obstacles_from_costmap_polygons
        args = (s._h, _abi._ptr(p, C.c_double), float(dist), int(T), None, C.byref(n_o), C.byref(n_p), _abi._ptr(off, C.c_int32),
                _abi._ptr(xs, C.c_double), _abi._ptr(ys, C.c_double), cap_o, cap_p)

    def call():
        if f(*args) != _abi.OK:
            raise RuntimeError(planner.lib().teb_amd_last_error())
    return call


def _optimise(s, batch, cfg):
    ks = []
    for _ in range(5):
        s.upload(batch)
        s.optimize(cfg.optim.no_inner_iterations, cfg.optim.no_outer_iterations)
        s.synchronize()
        ks.append(s.last_kernel_ms())
    layout, jmode, kind = s.last_instantiation()
    return dict(optimise_kernel_ms=round(float(np.median(ks)), 3), layout=layout, jacobian_mode=jmode, scene_kind=kind)


def _cases(grids):
    for N in grids:
        yield N, "structured", structured_grid(np.random.default_rng(N), N, walls=True, boxes=max(6, N // 20), disks=max(6, N // 20))
        for frac in (0.02, 0.10):   # tools/costmap_obstacles_times.py's grids
            rng = np.random.default_rng(N + int(frac * 100))
            yield N, "random_%g" % frac, np.where(rng.random((N, N)) < frac, 254, rng.integers(0, 253, (N, N))).astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--tiles", type=int, nargs="+", default=[1, 4, 8, 16, 32])
    ap.add_argument("--grids", type=int, nargs="+", default=[120, 400, 1000])
    args = ap.parse_args()
    binary_hash = planner.TebBatchSolver.build_info()[0]
    print(json.dumps(dict(binary_hash=binary_hash, reps=args.reps, tiles=args.tiles)), flush=True)
    res, pose, dist = 0.05, (0.0, 0.0, 0.3), 1.5
    for N, kind, cells in _cases(args.grids):
        ox = oy = -0.5 * N * res
        cfg = TebConfig()
        batch = _abi.TebBatchHost(1, 200)
        L = min(10.0, 0.45 * N * res)
        px, py, th, dt = scenes.sine_band(100, L, 0.3, 1.0, cfg.robot.max_vel_x)
        batch.set_teb(0, px - 0.5 * L, py, th, dt)
        n = int(np.count_nonzero(cells[:-1, :-1] == 254))   # an upper bound of the kept cells: the capacity of both routes
        s = planner.TebBatchSolver(cfg, 1, 200, n, 2 * n, 1)
        s.upload(batch)
        s.set_costmap(cells, res, ox, oy)
        n_pts = s.set_obstacles_from_costmap(pose, dist)[0]
        line = dict(grid=N, map=kind, route="points", rows=n_pts, vertices=n_pts, polygon_vertices=0,
                    call_ms=round(_median_ms(_c_call(s, pose, dist), args.reps), 4),
                    binding_ms=round(_median_ms(lambda: s.set_obstacles_from_costmap(pose, dist), args.reps), 4))
        if n_pts <= 20000:
            s.set_obstacles_from_costmap(pose, dist)
            line.update(_optimise(s, batch, cfg))
        print(json.dumps(line), flush=True)
        for T in args.tiles:
            t = s.set_obstacles_from_costmap_polygons(pose, dist, T)
            rows = len(t)
            line = dict(grid=N, map=kind, route="polygons", tile_cells=T, rows=rows,
                        vertices=int(sum(1 if ty == _abi.OBST_POINT else 2 if ty == _abi.OBST_LINE else 0 for ty in t.type) + len(t.vert_x)),
                        polygon_vertices=len(t.vert_x), lines=int(t.type.count(_abi.OBST_LINE)),
                        polygons=int(t.type.count(_abi.OBST_POLYGON)), rows_per_point=round(rows / max(n_pts, 1), 4),
                        call_ms=round(_median_ms(_c_call(s, pose, dist, T), args.reps), 4),
                        binding_ms=round(_median_ms(lambda: s.set_obstacles_from_costmap_polygons(pose, dist, T), args.reps), 4))
            if rows <= 20000:
                s.set_obstacles_from_costmap_polygons(pose, dist, T)
                line.update(_optimise(s, batch, cfg))
            print(json.dumps(line), flush=True)
        s.close()


if __name__ == "__main__":
    main()
