"""What the equivalence classes of a fleet cost: 1, 8 and 64 scenes x 4 bands x 100 poses x 60 point obstacles (tests/fleet_cases.py:
oracle_point_fleet), 3-D (HSignature3d, include_dynamic_obstacles) and 2-D (HSignature) signatures, median wall milliseconds of 20
repeats after 5 warm-ups of one compute + one class-filter call.

  (a) fleet      one handle: teb_amd_compute_h_signatures_per_scene + teb_amd_filter_equivalence_classes_per_scene - one launch for
                 every band against its own scene;
  (b) handles    what a fleet had to do before: teb_amd_compute_h_signatures + teb_amd_filter_equivalence_classes on each of N
                 single-scene handles in turn (every compute call synchronises its stream).

The bands do not change between the repeats, so the 2-D products are computed in the first warm-up only, in both variants. Every
(variant, dimension, scenes) cell runs in a process of its own under a time limit; the first cell that fails ends the run.
    python tools/fleet_hsig_bench.py [--out profiles/fleet_hsig_times.txt]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

REPEATS, WARMUP, CELL_TIMEOUT_S = 20, 5, 180


def worker(variant, n_scenes, mode):
    import numpy as np
    import fleet_cases
    from teb_local_planner_amd import planner
    f = fleet_cases.oracle_point_fleet(n_scenes=n_scenes)
    cfg = f.cfg
    cfg.obstacles.include_dynamic_obstacles = (mode == 3)
    hp = cfg.hcp
    mo, mv, mw = f.capacities()
    solvers = []
    if variant == "a":
        s = planner.TebBatchSolver(cfg, f.batch.count, f.batch.stride, mo, mv, mw)
        s.set_scenes(f.tables, f.vias); s.set_band_scenes(f.scene_of); s.upload(f.batch)
        solvers.append(s)
    else:
        for sc in range(f.n_scenes):
            sub, _ = f.scene_batch(sc)
            solvers.append(planner.make_solver(cfg, f.tables[sc], f.vias[sc], sub))
    # one optimise step first: the shader clock the table quotes is the one of an optimise kernel on this device
    solvers[0].snapshot()
    solvers[0].optimize(1, 1)
    clock = float(solvers[0].last_shader_clock_mhz())
    solvers[0].restore()
    wall, kept = [], 0
    for step in range(WARMUP + REPEATS):
        for s in solvers:
            s.synchronize()
        t0 = time.perf_counter()
        if variant == "a":
            solvers[0].h_signatures_per_scene(hp.h_signature_prescaler, values=False)
            keep, _, _ = solvers[0].filter_equivalence_classes_per_scene(hp.h_signature_threshold, None, hp.max_number_plans_in_current_class)
            kept = int(keep.sum())
        else:
            kept = 0
            for s in solvers:
                s.h_signatures(hp.h_signature_prescaler, values=False)
                keep, _, _ = s.filter_equivalence_classes(hp.h_signature_threshold, -1, hp.max_number_plans_in_current_class)
                kept += int(keep.sum())
        t1 = time.perf_counter()
        if step >= WARMUP:
            wall.append((t1 - t0) * 1e3)
    print(json.dumps({"variant": variant, "mode": mode, "scenes": n_scenes, "bands": int(f.batch.count), "wall_ms": float(np.median(wall)),
                      "wall_min_ms": float(min(wall)), "clock_mhz": clock, "kept": kept}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker"); ap.add_argument("--scenes", type=int); ap.add_argument("--mode", type=int)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fleet_hsig_times.txt"))
    a = ap.parse_args()
    if a.worker:
        return worker(a.worker, a.scenes, a.mode)
    rows = []
    names = {"a": "(a) fleet, per-scene compute + filter", "b": "(b) compute + filter on every handle in turn"}
    for mode in (3, 2):
        for n in (1, 8, 64):
            for v in ("a", "b"):
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", v, "--scenes", str(n), "--mode", str(mode)], capture_output=True,
                                   text=True, timeout=CELL_TIMEOUT_S)
                if p.returncode != 0:
                    sys.stderr.write(p.stdout + p.stderr)
                    sys.exit("cell (%s, %d-D, %d scenes) ended with status %d: nothing more is started" % (v, mode, n, p.returncode))
                rows.append(json.loads(p.stdout.strip().splitlines()[-1]))
                print(rows[-1], flush=True)
    lines = ["# tools/fleet_hsig_bench.py: scenes x 4 bands x 100 poses x 60 point obstacles; one H-signature compute + one class-filter call,",
             "# median wall ms of %d repeats after %d warm-ups; clock: shader clock of an optimise kernel in the same process [MHz];" % (REPEATS, WARMUP),
             "# kept: bands the class filter keeps (equal in (a) and (b))",
             "%-48s %4s %7s %6s %9s %9s %7s %5s" % ("variant", "dim", "scenes", "bands", "wall ms", "min ms", "clock", "kept")]
    for r in rows:
        lines.append("%-48s %4s %7d %6d %9.3f %9.3f %7.0f %5d" % (names[r["variant"]], "%d-D" % r["mode"], r["scenes"], r["bands"], r["wall_ms"], r["wall_min_ms"],
                                                                  r["clock_mhz"], r["kept"]))
    by = {(r["variant"], r["mode"], r["scenes"]): r["wall_ms"] for r in rows}
    for mode in (3, 2):
        for n in (1, 8, 64):
            lines.append("# %d-D, %2d scenes: fleet / handles = %.2f" % (mode, n, by[("a", mode, n)] / by[("b", mode, n)]))
    text = "\n".join(lines) + "\n"
    print(text)
    with open(a.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
