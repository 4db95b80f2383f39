"""What robot classes cost a whole tick: FleetHomotopyClassPlanner.plan(costmaps_per_robot) + isTrajectoryFeasible + hasDiverged +
getVelocityCommands on the workload of tools/fleet_tick_bench.py (scenes x 4 bands x 100 poses, one 120 x 120 costmap per scene) at
1, 8 and 64 robots, the same starts and goals every repeat:

  none   no classes: the per-scene calls, the cost triple as arguments of the launch (what tools/fleet_tick_bench.py's tick row runs);
  one    ONE class equal to the fleet's configuration: the class map and the four _per_class calls, the same work;
  two    two classes, robot r in class r mod 2: the second drives faster, keeps another distance, pads to other min_samples, looks two
         poses ahead (a second consumers launch) and has its own cost triple, footprint and look-ahead pair.

Median wall milliseconds of 20 repeats after 5 warm-ups, every timed region ends with a stream synchronisation; the cells alternate
(none, one, two, none, one, two) and each runs in a process of its own under a time limit; the first cell that fails ends the run.
    python tools/fleet_class_tick_bench.py [--out profiles/fleet_class_tick_times.txt]"""
import argparse
import copy
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import fleet_tick_bench as TB  # noqa: E402

REPEATS, WARMUP, CELL_TIMEOUT_S = TB.REPEATS, TB.WARMUP, TB.CELL_TIMEOUT_S
WIDE = [(-0.25, -0.2), (0.35, -0.2), (0.35, 0.2), (-0.25, 0.2)]


def worker(variant, n):
    import numpy as np
    from teb_local_planner_amd import planner
    cfg, grids, poses, goals, batch, scene_of = TB.workload(n)
    B, cap = n * TB.BANDS, n * (TB.CELLS + 4)
    vels = np.tile(np.array([0.1, 0.0, 0.02]), (n, 1))
    kw = dict(max_tebs=B, max_poses=TB.STRIDE, max_obstacles=cap, max_obstacle_vertices=1, max_via_points=1)
    if variant == "none":
        fl = planner.FleetHomotopyClassPlanner(cfg, n, **kw)
        footprint, radius = TB.FOOTPRINT, 0.15
    else:
        fast = copy.deepcopy(cfg)
        if variant == "two":
            fast.robot.max_vel_x, fast.robot.max_vel_theta, fast.robot.acc_lim_x = 0.8, 0.6, 0.9
            fast.obstacles.min_obstacle_dist, fast.trajectory.min_samples = 0.3, 6
            fast.trajectory.control_look_ahead_poses, fast.trajectory.feasibility_check_no_poses = 2, 8
            fast.hcp.selection_obst_cost_scale, fast.hcp.selection_alternative_time_cost = 2.0, True
        cfgs = [cfg, fast] if variant == "two" else [cfg]
        fl = planner.FleetHomotopyClassPlanner(cfg, n, robot_cfgs=cfgs, class_of_robot=[r % len(cfgs) for r in range(n)], **kw)
        footprint, radius = ([TB.FOOTPRINT, WIDE], [0.15, 0.2]) if variant == "two" else (TB.FOOTPRINT, 0.15)
    s = fl.solver
    st = [tuple(p) for p in poses]; gl = [tuple(p) for p in goals]; vl = [tuple(v) for v in vels]
    wall = []
    for step in range(WARMUP + REPEATS):
        s.synchronize()
        t0 = time.perf_counter()
        fl.plan(st, gl, vl, costmaps_per_robot=grids, costmap_obstacles_behind_robot_dist=TB.DIST, now=0.0)
        fl.isTrajectoryFeasible(footprint, radius); fl.hasDiverged(); fl.getVelocityCommands()
        s.synchronize()
        t1 = time.perf_counter()
        if step >= WARMUP:
            wall.append((t1 - t0) * 1e3)
    print(json.dumps({"variant": variant, "robots": n, "bands": int(s.count), "wall_ms": float(np.median(wall)), "wall_min_ms": float(min(wall)),
                      "kernel_ms": float(s.last_kernel_ms()), "clock_mhz": float(s.last_shader_clock_mhz())}))


LABEL = {"none": "no classes (per-scene calls)", "one": "one class (per-class calls)", "two": "two classes (per-class calls)"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker"); ap.add_argument("--robots", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fleet_class_tick_times.txt"))
    a = ap.parse_args()
    if a.worker:
        return worker(a.worker, a.robots)
    rows = []
    for n in (1, 8, 64):
        for variant in ("none", "one", "two") * 2:   # alternating
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", variant, "--robots", str(n)], capture_output=True, text=True,
                               timeout=CELL_TIMEOUT_S)
            if p.returncode != 0:
                sys.stderr.write(p.stdout + p.stderr)
                sys.exit("cell (%s, %d) ended with status %d: nothing more is started" % (variant, n, p.returncode))
            rows.append(json.loads(p.stdout.strip().splitlines()[-1]))
            print(rows[-1], flush=True)
    lines = ["# tools/fleet_class_tick_bench.py: a whole tick (plan from costmaps + feasibility + divergence + commands), median wall ms of %d" % REPEATS,
             "# repeats after %d warm-ups, each cell twice, alternating; kernel ms: the last optimise launch; clock: its shader clock [MHz]" % WARMUP,
             "%-32s %6s %6s %9s %9s %10s %7s" % ("cell", "robots", "bands", "wall ms", "min ms", "kernel ms", "clock")]
    for r in rows:
        lines.append("%-32s %6d %6d %9.3f %9.3f %10.3f %7.0f" % (LABEL[r["variant"]], r["robots"], r["bands"], r["wall_ms"], r["wall_min_ms"], r["kernel_ms"],
                                                              r["clock_mhz"]))
    for n in (1, 8, 64):
        med = {v: sorted(r["wall_ms"] for r in rows if r["variant"] == v and r["robots"] == n) for v in LABEL}
        lines.append("# %2d robots: one class / no classes = %.3f, two classes / one class = %.3f (the better run of each)" % (
            n, med["one"][0] / med["none"][0], med["two"][0] / med["one"][0]))
    text = "\n".join(lines) + "\n"
    print(text)
    with open(a.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
