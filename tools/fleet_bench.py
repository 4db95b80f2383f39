"""What a fleet costs: 1, 8 and 64 scenes x 4 bands x 100 poses x 60 point obstacles (tests/fleet_cases.py: oracle_point_fleet), median wall
milliseconds of 20 optimise steps after 5 warm-ups, the bands restored before every step.

  (a) fleet      one handle, one launch: every band against its own scene (teb_amd_set_scenes);
  (b) handles    what a fleet had to do before: one single-scene handle per scene, default options, launched back to back on their own
                 streams and synchronised at the end;
  (c) parent     (b) with the library of the parent commit (--parent-lib PATH; left out without it): shows that (b) did not move;
  (d) one scene  all the bands re-based into scene 0 and optimised as ONE scene on the generic path (generic_config_path, no helpers):
                 the price of the indirection and of the non-folded kind is (a) over (d).

Every (variant, scenes) cell runs in a process of its own under a time limit; the first cell that fails ends the run.
    python tools/fleet_bench.py [--parent-lib tools/libteb_amd_parent.so] [--out profiles/fleet_times.txt]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

STEPS, WARMUP, CELL_TIMEOUT_S = 20, 5, 180


def worker(variant, n_scenes):
    import numpy as np
    import fleet_cases
    from teb_local_planner_amd import _abi, planner
    f = fleet_cases.oracle_point_fleet(n_scenes=n_scenes)
    cfg = f.cfg
    mo, mv, mw = f.capacities()
    solvers = []
    if variant == "a":
        s = planner.TebBatchSolver(cfg, f.batch.count, f.batch.stride, mo, mv, mw)
        s.set_scenes(f.tables, f.vias); s.set_band_scenes(f.scene_of); s.upload(f.batch)
        solvers.append(s)
    elif variant in ("b", "c"):
        for sc in range(f.n_scenes):
            sub, _ = f.scene_batch(sc)
            solvers.append(planner.make_solver(cfg, f.tables[sc], f.vias[sc], sub))
    else:   # d: every band moved from its scene's place on the floor to scene 0's
        g = f.batch.copy()
        for b in range(g.count):
            ox, oy = f.origins[int(f.scene_of[b])]
            g.x[b] += f.origins[0][0] - ox; g.y[b] += f.origins[0][1] - oy
        solvers.append(planner.make_solver(cfg, f.tables[0], f.vias[0], g, options=_abi.Options(generic_config_path=True, multi_cu=-1, speculative_trials=-1)))
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
            kern.append(max(s.last_kernel_ms() for s in solvers))
    ok = all((s.results().status == _abi.TEB_OK).all() for s in solvers)
    print(json.dumps({"variant": variant, "scenes": n_scenes, "bands": int(f.batch.count), "wall_ms": float(np.median(wall)), "wall_min_ms": float(min(wall)),
                      "slowest_kernel_ms": float(np.median(kern)), "clock_mhz": float(solvers[0].last_shader_clock_mhz()),
                      "instantiation": list(solvers[0].last_instantiation()), "all_ok": bool(ok)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker"); ap.add_argument("--scenes", type=int)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fleet_times.txt"))
    a = ap.parse_args()
    if a.worker:
        return worker(a.worker, a.scenes)
    rows = []
    names = {"a": "(a) fleet, one launch", "b": "(b) one handle per scene", "c": "(c) the same, parent library", "d": "(d) all bands as ONE scene, generic path"}
    for n in (1, 8, 64):
        for v in ("a", "b", "c", "d"):
            if v == "c" and not a.parent_lib:
                continue
            env = dict(os.environ)
            if v == "c":
                env["TEB_AMD_LIB"] = os.path.abspath(a.parent_lib)
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", v, "--scenes", str(n)], env=env, capture_output=True, text=True, timeout=CELL_TIMEOUT_S)
            if p.returncode != 0:
                sys.stderr.write(p.stdout + p.stderr)
                sys.exit("cell (%s, %d scenes) ended with status %d: nothing more is started" % (v, n, p.returncode))
            rows.append(json.loads(p.stdout.strip().splitlines()[-1]))
            print(rows[-1], flush=True)
    lines = ["# tools/fleet_bench.py: scenes x 4 bands x 100 poses x 60 point obstacles, TebConfig defaults + include_dynamic_obstacles, teb_autosize on;",
             "# median wall ms of %d optimise steps after %d warm-ups (launch .. synchronize of every handle), bands restored before every step;" % (STEPS, WARMUP),
             "# kernel ms: HIP events of the (slowest) handle; clock: shader clock of the last launch [MHz]; kind: (layout, Jacobian mode, scene kind)",
             "%-44s %7s %6s %9s %9s %10s %7s  %s" % ("variant", "scenes", "bands", "wall ms", "min ms", "kernel ms", "clock", "kind")]
    for r in rows:
        lines.append("%-44s %7d %6d %9.3f %9.3f %10.3f %7.0f  %s%s" % (names[r["variant"]], r["scenes"], r["bands"], r["wall_ms"], r["wall_min_ms"], r["slowest_kernel_ms"],
                                                                    r["clock_mhz"], tuple(r["instantiation"]), "" if r["all_ok"] else "  (a band did not end OK)"))
    by = {(r["variant"], r["scenes"]): r["wall_ms"] for r in rows}
    for n in (1, 8, 64):
        if ("a", n) in by and ("b", n) in by and ("d", n) in by:
            lines.append("# %2d scenes: fleet / handles = %.2f, fleet / one scene = %.2f" % (n, by[("a", n)] / by[("b", n)], by[("a", n)] / by[("d", n)]))
    text = "\n".join(lines) + "\n"
    print(text)
    with open(a.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
