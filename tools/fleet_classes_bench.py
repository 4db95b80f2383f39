"""What robot classes cost and gain (teb_amd_set_scene_configs). Median milliseconds of 20 steps after 5 warm-ups, the bands restored
before every step; every cell runs in a process of its own under a time limit, the first cell that fails ends the run.

  homogeneous fleets must not pay - the optimise launch of a fleet WITHOUT a class map, kernel ms (HIP events), this tree's library
  against the parent commit's (--parent-lib PATH), alternating, the parent's twice (the spread of a launch measured against itself):
      points  tests/fleet_cases.py: oracle_point_fleet, 64 scenes x 4 bands x 100 poses x 60 point obstacles
      mixed   oracle_mixed_fleet, 6 scenes, 17 bands, every obstacle type, polygon footprint
  what a heterogeneous fleet gains - n robots in the 3 point classes of tests/fleet_config_cases.py (robot r: class r mod 3):
      one     one handle, one class map, one launch
      three   what a user did before: one handle per class with the robots of that class, launched back to back on their own streams
  for the optimise launch (scenes x 4 bands x 100 poses x 60 obstacles) and for the TebFleetPlanner.plan tick (one band per robot).

    python tools/fleet_classes_bench.py --parent-lib tools/libteb_amd_parent.so [--out profiles/fleet_classes_times.txt]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

STEPS, WARMUP, CELL_TIMEOUT_S = 20, 5, 240


def _measure(solvers, cfg):
    import numpy as np
    from teb_local_planner_amd import _abi
    for s in solvers:
        s.snapshot()
    o = cfg.optim
    wall, kern = [], []
    for step in range(WARMUP + STEPS):
        for s in solvers:
            s.restore()
        for s in solvers:
            s.synchronize()
        t0 = time.perf_counter()
        for s in solvers:
            s.optimize(o.no_inner_iterations, o.no_outer_iterations)
        for s in solvers:
            s.synchronize()
        t1 = time.perf_counter()
        if step >= WARMUP:
            wall.append((t1 - t0) * 1e3)
            kern.append(sum(s.last_kernel_ms() for s in solvers))
    ok = all((s.results().status[:s.count] == _abi.TEB_OK).all() for s in solvers)
    return dict(wall_ms=float(np.median(wall)), kernel_ms=float(np.median(kern)), kernel_min_ms=float(min(kern)),
                clock_mhz=float(solvers[0].last_shader_clock_mhz()), instantiation=list(solvers[0].last_instantiation()), all_ok=bool(ok))


def _fleet_handle(f, cfg, cfgs=None, class_of=None):
    from teb_local_planner_amd import planner
    mo, mv, mw = f.capacities()
    s = planner.TebBatchSolver(cfg, f.batch.count, f.batch.stride, mo, mv, mw)
    s.set_scenes(f.tables, f.vias)
    if cfgs is not None:
        s.set_scene_configs(cfgs, class_of)
    s.set_band_scenes(f.scene_of); s.upload(f.batch)
    return s


def _sub_fleet(f, scenes):
    """the scenes `scenes` of fleet f and their bands as a fleet of their own"""
    import numpy as np
    import fleet_cases
    from teb_local_planner_amd import _abi
    bands = [b for b in range(f.batch.count) if int(f.scene_of[b]) in scenes]
    sub = _abi.TebBatchHost(len(bands), f.batch.stride)
    for k, b in enumerate(bands):
        for fld in ("n", "x", "y", "theta", "dt", "has_vel_start", "vel_start", "has_vel_goal", "vel_goal", "prefer_rotdir", "via_points_enabled"):
            getattr(sub, fld)[k] = getattr(f.batch, fld)[b]
    return fleet_cases.Fleet(f.cfg, [f.tables[s] for s in scenes], [f.vias[s] for s in scenes], sub, np.asarray([scenes.index(int(f.scene_of[b])) for b in bands]))


def worker(cell, n):
    import numpy as np
    import fleet_cases
    import fleet_config_cases as FC
    from teb_local_planner_amd import _abi, planner
    r = {"cell": cell, "n": n}
    if cell in ("points", "mixed"):
        f = fleet_cases.oracle_point_fleet() if cell == "points" else fleet_cases.oracle_mixed_fleet()
        r.update(_measure([_fleet_handle(f, f.cfg)], f.cfg), bands=int(f.batch.count))
    elif cell in ("one", "three"):
        # stride 192 and not the fleet's own 160: under the fast class (dt_ref = 0.2) the first autoResize takes a band of scene 34 to
        # 166 poses before it shrinks again (CPU oracle, one outer iteration) - at 160 that band overflows and ends FAILED
        f = fleet_cases.oracle_point_fleet(n_scenes=n, stride=192)
        cfgs = FC.point_classes()
        class_of = [s % 3 for s in range(n)]
        if cell == "one":
            solvers = [_fleet_handle(f, cfgs[0], cfgs, class_of)]
        else:
            solvers = [_fleet_handle(_sub_fleet(f, [s for s in range(n) if class_of[s] == k]), cfgs[k]) for k in range(3)]
        r.update(_measure(solvers, cfgs[0]), bands=int(f.batch.count))
    else:   # tick_one / tick_three: TebFleetPlanner.plan, one band per robot, ticks 1 .. are warm starts
        cfgs = FC.point_classes()
        class_of = [k % 3 for k in range(n)]
        rng = np.random.default_rng(307)
        origin = rng.uniform(-20, 20, (n, 2))
        tables = []
        for k in range(n):
            t = _abi.ObstacleTable()
            for _ in range(30):
                t.add_point(origin[k, 0] + rng.uniform(0.5, 5.5), origin[k, 1] + rng.uniform(-1.5, 1.5))
            tables.append(t)
        groups = [list(range(n))] if cell == "tick_one" else [[k for k in range(n) if class_of[k] == c] for c in range(3)]
        if cell == "tick_one":
            planners = [planner.TebFleetPlanner(cfgs[0], n, max_poses=128, max_obstacles=31 * n, robot_cfgs=cfgs, class_of_robot=class_of)]
        else:
            planners = [planner.TebFleetPlanner(cfgs[c], len(g), max_poses=128, max_obstacles=31 * len(g)) for c, g in enumerate(groups)]
        wall = []
        for tick in range(WARMUP + STEPS):
            starts = [(origin[k, 0] + 0.02 * tick, origin[k, 1], 0.0) for k in range(n)]
            goals = [(origin[k, 0] + 6.0, origin[k, 1] + 0.2, 0.0) for k in range(n)]
            t0 = time.perf_counter()
            ok = [p.plan([starts[k] for k in g], [goals[k] for k in g], None, [tables[k] for k in g], [[] for _ in g]) for p, g in zip(planners, groups)]
            t1 = time.perf_counter()
            if tick >= WARMUP:
                wall.append((t1 - t0) * 1e3)
        r.update(wall_ms=float(np.median(wall)), kernel_ms=float(sum(p.solver.last_kernel_ms() for p in planners)), kernel_min_ms=0.0,
                 clock_mhz=float(planners[0].solver.last_shader_clock_mhz()), instantiation=list(planners[0].solver.last_instantiation()),
                 all_ok=bool(all(o.all() for o in ok)), robots_ok=int(sum(int(o.sum()) for o in ok)), bands=n)
    print(json.dumps(r))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker"); ap.add_argument("--n", type=int, default=0)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fleet_classes_times.txt"))
    a = ap.parse_args()
    if a.worker:
        return worker(a.worker, a.n)
    cells = []
    for fleet in ("points", "mixed"):   # alternating libraries: parent, this tree, parent, this tree
        for lib in ("parent", "this", "parent", "this"):
            if lib == "parent" and not a.parent_lib:
                continue
            cells.append((fleet, 0, lib))
    for n in (8, 64):
        cells += [("one", n, "this"), ("three", n, "this"), ("tick_one", n, "this"), ("tick_three", n, "this")]
    rows = []
    for cell, n, lib in cells:
        env = dict(os.environ)
        if lib == "parent":
            env["TEB_AMD_LIB"] = os.path.abspath(a.parent_lib)
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", cell, "--n", str(n)], env=env, capture_output=True, text=True, timeout=CELL_TIMEOUT_S)
        if p.returncode != 0:
            sys.stderr.write(p.stdout + p.stderr)
            sys.exit("cell (%s, %d, %s) ended with status %d: nothing more is started" % (cell, n, lib, p.returncode))
        rows.append(dict(json.loads(p.stdout.strip().splitlines()[-1]), lib=lib))
        print(rows[-1], flush=True)
    names = {"points": "fleet without a map, 64 x 4 point fleet", "mixed": "fleet without a map, mixed fleet", "one": "3 classes, ONE handle, one launch",
             "three": "3 classes, one handle per class", "tick_one": "TebFleetPlanner.plan, 3 classes, ONE handle", "tick_three": "TebFleetPlanner.plan, one planner per class"}
    lines = ["# tools/fleet_classes_bench.py: median ms of %d steps after %d warm-ups; kernel ms: HIP events of the optimise launch(es), summed over" % (STEPS, WARMUP),
             "# the handles of a cell; wall ms: launch .. synchronize (the plan() call for the ticks); clock: shader clock of the last launch [MHz]",
             "%-46s %8s %6s %6s %10s %10s %9s %7s  %s" % ("cell", "library", "robots", "bands", "kernel ms", "min ms", "wall ms", "clock", "kind")]
    for r in rows:
        lines.append("%-46s %8s %6s %6d %10.3f %10.3f %9.3f %7.0f  %s%s" % (names[r["cell"]], r["lib"], r["n"] or "-", r["bands"], r["kernel_ms"], r["kernel_min_ms"], r["wall_ms"],
                                                                         r["clock_mhz"], tuple(r["instantiation"]),
                                                                         "" if r["all_ok"] else "  (%s did not end OK)" % ("%d robots" % (r["bands"] - r["robots_ok"]) if "robots_ok" in r else "a band")))
    for fleet in ("points", "mixed"):
        par = [r["kernel_ms"] for r in rows if r["cell"] == fleet and r["lib"] == "parent"]
        this = [r["kernel_ms"] for r in rows if r["cell"] == fleet and r["lib"] == "this"]
        if par and this:
            lines.append("# %s: parent %s ms (spread %.1f %%), this tree %s ms: worst this / best parent = %.3f, best this / worst parent = %.3f" % (
                fleet, " / ".join("%.3f" % v for v in par), 100.0 * (max(par) - min(par)) / min(par), " / ".join("%.3f" % v for v in this),
                max(this) / min(par), min(this) / max(par)))
    text = "\n".join(lines) + "\n"
    print(text)
    with open(a.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
