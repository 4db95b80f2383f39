"""The polygon route of the costmap for a fleet (set_scenes_from_costmap_polygons) against the point route (set_scenes_from_costmaps)
and against what a user did before it existed: robots x 4 bands x 100 poses (capacity 160), one seeded 5 cm costmap per robot - the
structured 120^2 and 400^2 maps of tests/costmap_polygon_cases.py (structured_grid: walls, boxes, disks; another seed per robot) and the
random 120^2 map with 2 % lethal cells of tools/costmap_polygons_times.py - at 1, 8 and 64 robots, the robot in the middle of its map,
behind-robot distance 1.5 m; the lethal cells within 0.8 m of the line from start to goal are cleared (a corridor the tick's candidates
can pass). Per (map, robots):

  rows       the rows of a scene (mean over the scenes) and of the whole set: point route, polygon route at T = 8;
  tables     (p)  set_scenes_from_costmap_polygons at T = 8, the costmap set already on the device;
             (a)  set_scenes_from_costmaps on the same set;
             (b)  one single-scene handle per robot, its grid already on the device: set_obstacles_from_costmap_polygons on each, summed;
  optimise   the fleet's optimise launch (kernel ms of last_kernel_ms, median of 5) over the polygon tables and over the point tables;
  tick       FleetHomotopyClassPlanner.plan(costmaps_per_robot) with costmap_tile_cells = 8 and without (None), wall ms, and the bands
             the planner holds afterwards.

Median wall milliseconds of 10 repeats after 3 warm-ups (ticks: 5 after 2); every timed region ends with a stream synchronisation. Every
(map, robots) runs in a process of its own under a time limit, lightest first; the output file is rewritten after every one. A process
that fails or passes its limit ends the run: what it had measured by then is kept, the rest of its line reads "-". A tick that takes
longer than TICK_LIMIT_S is reported and not repeated. The (p) and (a) figures are those of the Python binding: they include the out
arrays it allocates by the handle's capacities and the ObstacleTable it returns per scene; the tick does without both
(return_tables = False).
    python tools/fleet_polygons_bench.py [--out profiles/fleet_polygons_times.txt]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

REPEATS, WARMUP, TICK_REPEATS, TICK_WARMUP, CELL_TIMEOUT_S, TICK_LIMIT_S = 10, 3, 5, 2, 300, 5.0
BANDS, POSES, STRIDE, RES, DIST, TILE, CORRIDOR = 4, 100, 160, 0.05, 1.5, 8, 0.8
MAPS = (("structured", 120), ("structured", 400), ("random_0.02", 120))
ROBOTS = (1, 8, 64)


class Grid:
    def __init__(self, cells, ox, oy):
        self.cells, self.resolution, self.origin_x, self.origin_y = cells, RES, ox, oy


def workload(kind, N, n):
    import numpy as np
    from costmap_polygon_cases import structured_grid
    from teb_local_planner_amd import _abi, scenes
    from teb_local_planner_amd.config import TebConfig
    cfg = TebConfig()
    cfg.hcp.max_number_classes = BANDS
    span = N * RES
    grids, poses, goals = [], [], []
    for r in range(n):
        rng = np.random.default_rng(N + 1000 * r)                              # robot 0: the map of tools/costmap_polygons_times.py
        if kind == "structured":
            cells = structured_grid(rng, N, walls=True, boxes=max(6, N // 20), disks=max(6, N // 20))
        else:
            rng = np.random.default_rng(N + 2 + 1000 * r)
            cells = np.where(rng.random((N, N)) < 0.02, 254, rng.integers(0, 253, (N, N))).astype(np.uint8)
        cx, cy = (span + 2.0) * (r % 8), (span + 2.0) * (r // 8)              # every robot somewhere else on the floor
        L = min(10.0, 0.45 * span)
        # a free corridor of CORRIDOR m either side of the line from start to goal: without it no candidate of the tick survives on
        # either kind of table (walls and scattered cells everywhere within min_obstacle_dist) and the tick would measure an early return
        c0, c1 = int((0.5 * (span - L) - CORRIDOR) / RES), int((0.5 * (span + L) + CORRIDOR) / RES) + 1
        r0, r1 = int((0.5 * span - CORRIDOR) / RES), int((0.5 * span + CORRIDOR) / RES) + 1
        lane = cells[max(r0, 0):r1, max(c0, 0):c1]
        lane[lane == 254] = 0
        grids.append(Grid(cells, cx - 0.5 * span, cy - 0.5 * span))
        poses.append((cx - 0.5 * L, cy, 0.3))
        goals.append((cx + 0.5 * L, cy, 0.0))
    batch = _abi.TebBatchHost(n * BANDS, STRIDE)
    scene_of = np.tile(np.arange(n), BANDS).astype(np.int32)                  # interleaved
    rng = np.random.default_rng(99)
    for b in range(n * BANDS):
        s = int(scene_of[b])
        L = min(10.0, 0.45 * span)
        px, py, th, dt = scenes.sine_band(POSES, L, 0.1 * (b // n) - 0.15, 1.0, cfg.robot.max_vel_x)
        batch.set_teb(b, px + poses[s][0], py + poses[s][1], th + rng.normal(0.0, 2e-3, th.shape), dt)
    return cfg, grids, np.array(poses), np.array(goals), batch, scene_of


def worker(kind, N, n):
    import numpy as np
    from teb_local_planner_amd import planner
    cfg, grids, poses, goals, batch, scene_of = workload(kind, N, n)
    B = n * BANDS
    lethal = [int(np.count_nonzero(g.cells[:-1, :-1] == 254)) for g in grids]  # an upper bound of the kept cells of both routes
    cap, vcap = sum(lethal) + 1, 2 * sum(lethal) + 1

    def median_ms(run, sync, reps, warm):
        ts = []
        for step in range(warm + reps):
            sync()
            t0 = time.perf_counter(); run(); sync()
            if step >= warm:
                ts.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(ts))

    out = dict(map=kind, grid=N, robots=n)
    points_ok = True
    try:
        s = planner.TebBatchSolver(cfg, B, STRIDE, cap, vcap, 1)
    except planner.TebAmdError as e:
        # a handle with room for the point rows of every scene cannot be created (the association table of bands x max_obstacles): the
        # point route has no figures here, the polygon route runs on a handle an eighth of that size
        points_ok = False
        out["points_refused"] = str(e)
        cap, vcap = cap // 8, vcap // 8
        s = planner.TebBatchSolver(cfg, B, STRIDE, cap, vcap, 1)
    s.set_costmaps(grids)
    n_pts = np.array(lethal)
    if points_ok:
        n_pts, _ = s.set_scenes_from_costmaps(poses, DIST)
    conv = s.set_scenes_from_costmap_polygons(poses, DIST, TILE)
    out.update(point_rows=int(n_pts.sum()), polygon_rows=int(sum(len(t) for t in conv)),
               polygon_vertices=int(sum(len(t.vert_x) for t in conv)), lines=int(sum(t.type.count(2) for t in conv)),
               polygons=int(sum(t.type.count(4) for t in conv)))
    # tables
    out["tables_p_ms"] = median_ms(lambda: s.set_scenes_from_costmap_polygons(poses, DIST, TILE), s.synchronize, REPEATS, WARMUP)
    if points_ok:
        out["tables_a_ms"] = median_ms(lambda: s.set_scenes_from_costmaps(poses, DIST), s.synchronize, REPEATS, WARMUP)
    hs = []
    for k in range(n):
        h = planner.TebBatchSolver(cfg, BANDS, STRIDE, lethal[k] + 1, 2 * lethal[k] + 1, 1)
        h.set_costmap(grids[k].cells, RES, grids[k].origin_x, grids[k].origin_y)
        hs.append(h)

    def singles():
        for k, h in enumerate(hs):
            h.set_obstacles_from_costmap_polygons(poses[k], DIST, TILE)
    out["tables_b_ms"] = median_ms(singles, lambda: [h.synchronize() for h in hs], REPEATS, WARMUP)
    for h in hs:
        h.close()
    print(json.dumps(out), flush=True)                                         # every phase leaves a line: the last one counts

    # the optimise launch of the fleet over each kind of table
    def optimise(install):
        install()
        s.set_band_scenes(scene_of)
        ks = []
        for _ in range(5):
            s.upload(batch)
            s.optimize(cfg.optim.no_inner_iterations, cfg.optim.no_outer_iterations)
            s.synchronize()
            ks.append(s.last_kernel_ms())
        return float(np.median(ks)), list(s.last_instantiation()), float(s.last_shader_clock_mhz())
    out["optimise_polygons_ms"], out["inst_polygons"], out["clock_mhz"] = optimise(lambda: s.set_scenes_from_costmap_polygons(poses, DIST, TILE))
    print(json.dumps(out), flush=True)
    if points_ok:
        out["optimise_points_ms"], out["inst_points"], _ = optimise(lambda: s.set_scenes_from_costmaps(poses, DIST))
    s.close()
    print(json.dumps(out), flush=True)

    # the whole tick
    st = [tuple(p) for p in poses]; gl = [tuple(p) for p in goals]; vl = [(0.1, 0.0, 0.02)] * n
    for name, tiles in (("polygons", TILE), ("points", None)) if points_ok else (("polygons", TILE),):
        fl = planner.FleetHomotopyClassPlanner(cfg, n, max_tebs=B, max_poses=STRIDE, max_obstacles=cap, max_obstacle_vertices=vcap, max_via_points=1)
        run = lambda: fl.plan(st, gl, vl, costmaps_per_robot=grids, costmap_obstacles_behind_robot_dist=DIST, now=0.0, costmap_tile_cells=tiles)
        t0 = time.perf_counter(); run(); fl.solver.synchronize()
        first = time.perf_counter() - t0
        if first > TICK_LIMIT_S:
            out["tick_%s_ms" % name], out["tick_%s_repeats" % name] = first * 1e3, 1
        else:
            out["tick_%s_ms" % name] = median_ms(run, fl.solver.synchronize, TICK_REPEATS, TICK_WARMUP)
            out["tick_%s_repeats" % name] = TICK_REPEATS
        out["tick_%s_bands" % name] = int(fl.solver.count)
        fl.solver.close()
        print(json.dumps(out), flush=True)


def report(rows, note=None):
    from teb_local_planner_amd import planner
    lines = ["# tools/fleet_polygons_bench.py (library %s): robots x %d bands x %d poses (capacity %d), one %g m costmap per robot, dist %g m, T = %d;"
             % (planner.TebBatchSolver.build_info()[0], BANDS, POSES, STRIDE, RES, DIST, TILE),
             "# wall ms: median of %d repeats after %d warm-ups (ticks: %d after %d; a tick over %g s is run once: marked *), every timed region ends with a"
             % (REPEATS, WARMUP, TICK_REPEATS, TICK_WARMUP, TICK_LIMIT_S),
             "# stream synchronisation; optimise: kernel ms of the fleet's launch, median of 5; inst: (layout, Jacobian mode, scene kind) it took.",
             "# tables: (p) set_scenes_from_costmap_polygons  (a) set_scenes_from_costmaps  (b) N single-scene handles, set_obstacles_from_costmap_polygons each;",
             "# (p), (a), (b) are the Python binding's calls: out arrays sized by the handle's capacities and one ObstacleTable per scene included; the",
             "# tick skips both. '-': not measured (the process of that line ended first).",
             "%-12s %5s %6s | %9s %9s %9s | %9s %9s %9s | %10s %10s %-9s %-9s | %10s %10s %6s %6s | %5s"
             % ("map", "grid", "robots", "pt rows", "poly rows", "poly vtx", "(p) ms", "(a) ms", "(b) ms", "opt poly", "opt pts", "inst poly", "inst pts",
                "tick poly", "tick pts", "bands", "bands", "MHz")]
    f = lambda r, k, fmt, w: (fmt % r[k]).rjust(w) if r.get(k) is not None else "-".rjust(w)
    inst = lambda r, k: ("/".join(map(str, r[k])) if r.get(k) is not None else "-").ljust(9)
    tick = lambda r, k: ("%9.2f%s" % (r["tick_%s_ms" % k], "*" if r["tick_%s_repeats" % k] == 1 else " ")) if r.get("tick_%s_ms" % k) is not None else "-".rjust(10)
    for r in rows:
        lines.append("%-12s %5d %6d | %s %s %s | %s %s %s | %s %s %s %s | %s %s %s %s | %s"
                     % (r["map"], r["grid"], r["robots"], f(r, "point_rows", "%d", 9), f(r, "polygon_rows", "%d", 9), f(r, "polygon_vertices", "%d", 9),
                        f(r, "tables_p_ms", "%.3f", 9), f(r, "tables_a_ms", "%.3f", 9), f(r, "tables_b_ms", "%.3f", 9),
                        f(r, "optimise_polygons_ms", "%.3f", 10), f(r, "optimise_points_ms", "%.3f", 10), inst(r, "inst_polygons"), inst(r, "inst_points"),
                        tick(r, "polygons"), tick(r, "points"), f(r, "tick_polygons_bands", "%d", 6), f(r, "tick_points_bands", "%d", 6),
                        f(r, "clock_mhz", "%.0f", 5)))
    ratio = lambda r, a, b: "%.2f" % (r[a] / r[b]) if r.get(a) is not None and r.get(b) is not None else "-"
    for r in rows:
        if r.get("points_refused"):
            lines.append("# %-12s %4d^2 %2d robots: no handle with room for the point rows (their count: lethal cells of the grids); %s"
                         % (r["map"], r["grid"], r["robots"], r["points_refused"]))
        if r.get("point_rows") is None:
            continue
        lines.append("# %-12s %4d^2 %2d robots: rows/scene %7.1f -> %6.1f; tables (p)/(a) = %s, (p)/(b) = %s; optimise poly/pts = %s; tick poly/pts = %s"
                     % (r["map"], r["grid"], r["robots"], r["point_rows"] / r["robots"], r["polygon_rows"] / r["robots"],
                        ratio(r, "tables_p_ms", "tables_a_ms"), ratio(r, "tables_p_ms", "tables_b_ms"),
                        ratio(r, "optimise_polygons_ms", "optimise_points_ms"), ratio(r, "tick_polygons_ms", "tick_points_ms")))
    if note:
        lines.append("# " + note)
    return "\n".join(lines) + "\n"


def main():
    import tempfile
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker"); ap.add_argument("--grid", type=int); ap.add_argument("--robots", type=int)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fleet_polygons_times.txt"))
    a = ap.parse_args()
    if a.worker:
        return worker(a.worker, a.grid, a.robots)
    rows, note = [], None
    for kind, N, n in sorted(((k, N, n) for k, N in MAPS for n in ROBOTS), key=lambda c: c[1] * c[1] * c[2]):   # lightest first
        with tempfile.TemporaryFile("w+") as so:
            p = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker", kind, "--grid", str(N), "--robots", str(n)],
                                 stdout=so, stderr=subprocess.PIPE, text=True)
            try:
                _, err = p.communicate(timeout=CELL_TIMEOUT_S)
                if p.returncode != 0:
                    sys.stderr.write(err)
                    note = "(%s, %d, %d robots) ended with status %d: nothing more was started" % (kind, N, n, p.returncode)
            except subprocess.TimeoutExpired:
                p.kill(); p.communicate()
                note = "(%s, %d, %d robots) passed its limit of %d s: nothing more was started" % (kind, N, n, CELL_TIMEOUT_S)
            so.seek(0)
            done = [ln for ln in so.read().splitlines() if ln.startswith("{")]
        rows.append(json.loads(done[-1]) if done else dict(map=kind, grid=N, robots=n))
        print(rows[-1], flush=True)
        with open(a.out, "w") as fh:                                           # what is measured so far survives a later failure
            fh.write(report(rows, note))
        if note:
            print(report(rows, note))
            sys.exit(note)
    print(report(rows))


if __name__ == "__main__":
    main()
