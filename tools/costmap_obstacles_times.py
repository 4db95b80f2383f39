#!/usr/bin/env python3
"""Wall time of teb_amd_set_obstacles_from_costmap (the grid already uploaded by set_costmap) against the host route: the reference's
loop restated on the host (numpy, tests/test_costmap_obstacles.py) + ObstacleTable + set_obstacles. Grids 120^2, 400^2, 1000^2 at 2 %
and 10 % lethal cells; one JSON line per case. Up to 20 000 obstacles it also runs one optimise of a single band over the grid and
reports the distance path that took (last_instantiation: layout, Jacobian mode, scene kind).

    python tools/costmap_obstacles_times.py [--reps 21]"""
import argparse
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
from test_costmap_obstacles import reference_costmap_obstacles  # noqa: E402


def _median_ms(fn, reps):
    fn()   # warm-up (first launch of the kernels, allocations)
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); ts.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=21)
    args = ap.parse_args()
    res = 0.05
    for N in (120, 400, 1000):
        for frac in (0.02, 0.10):
            rng = np.random.default_rng(N + int(frac * 100))
            cells = np.where(rng.random((N, N)) < frac, 254, rng.integers(0, 253, (N, N))).astype(np.uint8)
            ox = oy = -0.5 * N * res
            pose = (0.0, 0.0, 0.3)
            dist = 1.5
            xs, ys = reference_costmap_obstacles(cells, res, ox, oy, pose, dist)
            n = len(xs)
            cfg = TebConfig()
            batch = _abi.TebBatchHost(1, 200)
            L = min(10.0, 0.45 * N * res)
            px, py, th, dt = scenes.sine_band(100, L, 0.3, 1.0, cfg.robot.max_vel_x)
            batch.set_teb(0, px - 0.5 * L, py, th, dt)
            s = planner.TebBatchSolver(cfg, 1, 200, n, 1, 1)
            s.upload(batch)
            s.set_costmap(cells, res, ox, oy)
            dev_ms = _median_ms(lambda: s.set_obstacles_from_costmap(pose, dist), args.reps)

            def host_route():
                hx, hy = reference_costmap_obstacles(cells, res, ox, oy, pose, dist)
                t = _abi.ObstacleTable()
                for x, y in zip(hx.tolist(), hy.tolist()):
                    t.add_point(x, y)
                s.set_obstacles(t)
            host_ms = _median_ms(host_route, max(3, args.reps // 4))
            t = _abi.ObstacleTable()
            for x, y in zip(xs.tolist(), ys.tolist()):
                t.add_point(x, y)
            t.freeze()
            upload_ms = _median_ms(lambda: s.set_obstacles(t), args.reps)
            line = dict(grid=N, lethal=frac, n=n, set_obstacles_from_costmap_ms=round(dev_ms, 4),
                        set_obstacles_ms=round(upload_ms, 4), host_loop_and_set_obstacles_ms=round(host_ms, 4))
            if n <= 20000:
                s.set_obstacles_from_costmap(pose, dist)
                s.optimize(cfg.optim.no_inner_iterations, cfg.optim.no_outer_iterations)
                s.synchronize()
                layout, jmode, kind = s.last_instantiation()
                line.update(optimise_kernel_ms=round(s.last_kernel_ms(), 3), layout=layout, jacobian_mode=jmode, scene_kind=kind)
            print(json.dumps(line), flush=True)
            s.close()


if __name__ == "__main__":
    main()
