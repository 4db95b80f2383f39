"""What the two ends of a fleet tick cost beside its middle: scenes x 4 bands x 100 poses (capacity 160), one 120 x 120 costmap of 5 cm
cells per scene with 60 lethal cells ahead of the robot (all kept by the behind-robot filter), at 1, 8 and 64 scenes. For each of the
four ends (a) the per-scene call and (b) what it replaces, run with ANOTHER build of the library (--parent-lib: the parent commit's
libteb_amd.so, which has none of the per-scene calls):

  tables       (a)  set_costmaps + set_scenes_from_costmaps (the grids change every tick: their upload belongs to the tick);
               (a') set_scenes_from_costmaps alone, the set already on the device;
               (b)  every table built on the host (the numpy restatement of the reference's loop), then set_scenes;
               (b') set_costmap + set_obstacles_from_costmap on N single-scene handles in turn;
  prune        (a)  update_and_prune_per_scene with start velocities;   (b) update_and_prune + set_velocity_start band by band;
  commands     (a)  velocity_commands of every robot's band;            (b) velocity_command robot by robot;
  feasibility  (a)  is_trajectory_feasible_per_scene;                   (b) set_costmap + is_trajectory_feasible robot by robot;
  tick         FleetHomotopyClassPlanner: plan(costmaps_per_robot) + isTrajectoryFeasible + hasDiverged + getVelocityCommands against
               the parent's tick (host tables, set_scenes, the per-band / per-robot loops), same starts and goals every repeat.

Every timed region ends with a stream synchronisation. Median wall milliseconds of 20 repeats after 5 warm-ups; every cell runs in a
process of its own under a time limit, and the first cell that fails ends the run.
    python tools/fleet_tick_bench.py --parent-lib PATH [--out profiles/fleet_tick_times.txt]"""
import argparse
import json
import math
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPEATS, WARMUP, CELL_TIMEOUT_S = 20, 5, 240
BANDS, POSES, STRIDE, CELLS, GRID, RES, DIST = 4, 100, 160, 60, 120, 0.05, 1.5
FOOTPRINT = [(-0.2, -0.15), (0.3, -0.15), (0.3, 0.15), (-0.2, 0.15)]


class Grid:
    def __init__(self, cells, ox, oy):
        self.cells, self.resolution, self.origin_x, self.origin_y = cells, RES, ox, oy


def host_points(g, pose, dist):
    """updateObstacleContainerWithCostmap on the host (the restatement of tests/test_costmap_obstacles.py)."""
    import numpy as np
    sy, sx = g.cells.shape
    mx, my = np.nonzero(g.cells[:sy - 1, :sx - 1].T == 254)
    wx = g.origin_x + (mx.astype(np.float64) + 0.5) * g.resolution
    wy = g.origin_y + (my.astype(np.float64) + 0.5) * g.resolution
    c, s = math.cos(pose[2]), math.sin(pose[2])
    dx, dy = wx - pose[0], wy - pose[1]
    skip = (dx * c + dy * s < 0) & (np.sqrt(dx * dx + dy * dy) > dist)
    return wx[~skip], wy[~skip]


def host_table(g, pose, dist):
    from teb_local_planner_amd import _abi
    t = _abi.ObstacleTable()
    for x, y in zip(*host_points(g, pose, dist)):
        t.add_point(float(x), float(y))
    return t


def workload(n_scenes):
    import numpy as np
    from teb_local_planner_amd import _abi, scenes
    from teb_local_planner_amd.config import TebConfig
    rng = np.random.default_rng(808)
    cfg = TebConfig()
    cfg.hcp.max_number_classes = BANDS
    grids, poses, goals = [], [], []
    batch = _abi.TebBatchHost(n_scenes * BANDS, STRIDE)
    scene_of = np.tile(np.arange(n_scenes), BANDS).astype(np.int32)           # interleaved
    for s in range(n_scenes):
        ox, oy = 8.0 * (s % 8), 8.0 * (s // 8)
        cells = rng.integers(0, 100, size=(GRID, GRID)).astype(np.uint8)
        k = 0
        while k < CELLS:                                                       # ahead of the robot, off its centre line
            mx, my = int(rng.integers(30, GRID - 2)), int(rng.integers(5, GRID - 5))
            if abs(my - GRID // 2) >= 12 and cells[my, mx] != 254:
                cells[my, mx] = 254; k += 1
        grids.append(Grid(cells, ox, oy))
        poses.append((ox + 0.5, oy + 3.0, 0.0))
        goals.append((ox + 5.5, oy + 3.0, 0.0))
    for b in range(n_scenes * BANDS):
        s = int(scene_of[b])
        px, py, th, dt = scenes.sine_band(POSES, 5.0, 0.1 * (b // n_scenes) - 0.15, 1.0, cfg.robot.max_vel_x)
        batch.set_teb(b, px + poses[s][0], py + poses[s][1], th + rng.normal(0.0, 2e-3, th.shape), dt)
    return cfg, grids, np.array(poses), np.array(goals), batch, scene_of


def worker(end, variant, n):
    import numpy as np
    from teb_local_planner_amd import _abi, planner
    cfg, grids, poses, goals, batch, scene_of = workload(n)
    B = n * BANDS
    cap = n * (CELLS + 4)
    vels = np.tile(np.array([0.1, 0.0, 0.02]), (n, 1))
    tables = [host_table(g, poses[s], DIST) for s, g in enumerate(grids)]
    assert all(len(t) == CELLS for t in tables)

    def fleet_handle():
        s = planner.TebBatchSolver(cfg, B, STRIDE, cap, 1, 1)
        s.set_scenes(tables)
        s.set_band_scenes(scene_of)
        s.upload(batch)
        return s

    setup = lambda: None
    if end == "tables":
        if variant in ("a", "a1", "b"):
            s = fleet_handle()
            if variant == "a":
                def run():
                    s.set_costmaps(grids); s.set_scenes_from_costmaps(poses, DIST)
            elif variant == "a1":
                s.set_costmaps(grids)
                run = lambda: s.set_scenes_from_costmaps(poses, DIST)
            else:
                run = lambda: s.set_scenes([host_table(g, poses[k], DIST) for k, g in enumerate(grids)])
            sync = s.synchronize
        else:
            hs = [planner.TebBatchSolver(cfg, BANDS, STRIDE, CELLS + 4, 1, 1) for _ in range(n)]

            def run():
                for k, h in enumerate(hs):
                    h.set_costmap(grids[k].cells, RES, grids[k].origin_x, grids[k].origin_y)
                    h.set_obstacles_from_costmap(poses[k], DIST)
            sync = lambda: [h.synchronize() for h in hs]
    elif end == "prune":
        s = fleet_handle()
        starts = np.array([(batch.x[np.nonzero(scene_of == k)[0][0], 2], batch.y[np.nonzero(scene_of == k)[0][0], 2], 0.0) for k in range(n)])
        setup = lambda: s.upload(batch)
        if variant == "a":
            run = lambda: s.update_and_prune_per_scene(starts, goals, 3, vels)
        else:
            def run():
                for b in range(B):
                    k = int(scene_of[b])
                    s.update_and_prune(starts[k], goals[k], 3, b=b)
                    s.set_velocity_start(vels[k], True, b=b)
        sync = s.synchronize
    elif end == "commands":
        s = fleet_handle()
        best = np.array([np.nonzero(scene_of == k)[0][1] for k in range(n)], np.int32)
        setup = lambda: s.set_velocity_goal(None, True)                       # invalidates the consumers' outputs
        if variant == "a":
            run = lambda: s.velocity_commands(best, 1, 0)
        else:
            run = lambda: [s.velocity_command(int(b), 1, 0) for b in best]
        sync = s.synchronize
    elif end == "feasibility":
        s = fleet_handle()
        best = np.array([np.nonzero(scene_of == k)[0][1] for k in range(n)], np.int32)
        if variant == "a":
            s.set_costmaps(grids)
            run = lambda: s.is_trajectory_feasible_per_scene(best, FOOTPRINT, 0.15)
        else:
            def run():
                for k, b in enumerate(best):
                    s.set_costmap(grids[k].cells, RES, grids[k].origin_x, grids[k].origin_y)
                    s.is_trajectory_feasible(int(b), FOOTPRINT, 0.15)
        sync = s.synchronize
    else:   # the whole tick
        fl = planner.FleetHomotopyClassPlanner(cfg, n, max_tebs=B, max_poses=STRIDE, max_obstacles=cap, max_obstacle_vertices=1, max_via_points=1)
        s = fl.solver
        st = [tuple(p) for p in poses]; gl = [tuple(p) for p in goals]; vl = [tuple(v) for v in vels]
        if variant == "a":
            def run():
                fl.plan(st, gl, vl, costmaps_per_robot=grids, costmap_obstacles_behind_robot_dist=DIST, now=0.0)
                fl.isTrajectoryFeasible(FOOTPRINT, 0.15); fl.hasDiverged(); fl.getVelocityCommands()
        else:
            def update_all(starts, goals_, start_vels=None):                   # the parent's updateAllTEBs: one call per band
                if s.count > 0:
                    so = s.band_scenes()
                    for b in range(s.count):
                        r = int(so[b])
                        s.update_and_prune(starts[r], goals_[r], cfg.trajectory.min_samples, b=b)
                        s.set_velocity_start(start_vels[r], True, b=b)
                fl._goal = [tuple(g) for g in goals_]
            fl.updateAllTEBs = update_all

            def run():
                fl.plan(st, gl, vl, obstacles_per_robot=[host_table(g, st[k], DIST) for k, g in enumerate(grids)], now=0.0)
                t = cfg.trajectory
                for r in range(n):                                             # the parent's checks and commands: robot by robot
                    b = int(fl.best_teb_[r])
                    s.set_costmap(grids[r].cells, RES, grids[r].origin_x, grids[r].origin_y)
                    s.is_trajectory_feasible(b, FOOTPRINT, 0.15, t.min_resolution_collision_check_angular)
                    s.has_diverged(b)
                    s.velocity_command(b, t.control_look_ahead_poses, t.prevent_look_ahead_poses_near_goal)
        sync = s.synchronize

    # one optimise step first: the shader clock the table quotes is the one of an optimise kernel on this device
    clock = 0.0
    if end != "tick" and not (end == "tables" and variant == "b1"):
        s.optimize(1, 1); clock = float(s.last_shader_clock_mhz()); s.upload(batch)
    wall = []
    for step in range(WARMUP + REPEATS):
        setup(); sync()
        t0 = time.perf_counter()
        run(); sync()
        t1 = time.perf_counter()
        if step >= WARMUP:
            wall.append((t1 - t0) * 1e3)
    if end == "tick":
        clock = float(s.last_shader_clock_mhz())
    print(json.dumps({"end": end, "variant": variant, "scenes": n, "wall_ms": float(np.median(wall)), "wall_min_ms": float(min(wall)), "clock_mhz": clock}))


LABEL = {("tables", "a"): "(a) set_costmaps + set_scenes_from_costmaps", ("tables", "a1"): "(a') set_scenes_from_costmaps alone",
         ("tables", "b"): "(b) host tables + set_scenes, parent", ("tables", "b1"): "(b') N handles: set_obstacles_from_costmap, parent",
         ("prune", "a"): "(a) update_and_prune_per_scene", ("prune", "b"): "(b) per band prune + velocity, parent",
         ("commands", "a"): "(a) velocity_commands", ("commands", "b"): "(b) per robot velocity_command, parent",
         ("feasibility", "a"): "(a) is_trajectory_feasible_per_scene", ("feasibility", "b"): "(b) per robot set_costmap + check, parent",
         ("tick", "a"): "(a) plan(costmaps) + checks + commands", ("tick", "b"): "(b) the parent's tick"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker"); ap.add_argument("--variant"); ap.add_argument("--scenes", type=int)
    ap.add_argument("--parent-lib", default=None, help="libteb_amd.so of the parent commit for the (b) rows; without it they run on this build")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fleet_tick_times.txt"))
    ap.add_argument("--ends", default="tables,prune,commands,feasibility,tick")
    a = ap.parse_args()
    if a.worker:
        return worker(a.worker, a.variant, a.scenes)
    rows = []
    for end in a.ends.split(","):
        for n in (1, 8, 64):
            for (e, variant), label in LABEL.items():
                if e != end:
                    continue
                env = dict(os.environ)
                if variant.startswith("b") and a.parent_lib:
                    env["TEB_AMD_LIB"] = os.path.abspath(a.parent_lib)
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", end, "--variant", variant, "--scenes", str(n)],
                                   capture_output=True, text=True, timeout=CELL_TIMEOUT_S, env=env)
                if p.returncode != 0:
                    sys.stderr.write(p.stdout + p.stderr)
                    sys.exit("cell (%s, %s, %d scenes) ended with status %d: nothing more is started" % (end, variant, n, p.returncode))
                r = json.loads(p.stdout.strip().splitlines()[-1])
                r["label"] = label
                rows.append(r)
                print(r, flush=True)
    lines = ["# tools/fleet_tick_bench.py: scenes x %d bands x %d poses (capacity %d), one %d x %d costmap of %g m cells per scene with %d kept" % (BANDS, POSES, STRIDE, GRID, GRID, RES, CELLS),
             "# lethal cells; median wall ms of %d repeats after %d warm-ups, every timed region ends with a stream synchronisation;" % (REPEATS, WARMUP),
             "# (b) rows: %s; clock: shader clock of an optimise kernel in the same process [MHz] (0: none ran)" % ("the parent commit's library" if a.parent_lib else "THIS build (no --parent-lib)"),
             "%-12s %-52s %7s %10s %10s %7s" % ("end", "variant", "scenes", "wall ms", "min ms", "clock")]
    for r in rows:
        lines.append("%-12s %-52s %7d %10.3f %10.3f %7.0f" % (r["end"], r["label"], r["scenes"], r["wall_ms"], r["wall_min_ms"], r["clock_mhz"]))
    by = {(r["end"], r["variant"], r["scenes"]): r["wall_ms"] for r in rows}
    for end in a.ends.split(","):
        for n in (1, 8, 64):
            if (end, "a", n) in by and (end, "b", n) in by:
                lines.append("# %-11s %2d scenes: (a) / (b) = %.2f" % (end + ",", n, by[(end, "a", n)] / by[(end, "b", n)]))
    text = "\n".join(lines) + "\n"
    print(text)
    with open(a.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
