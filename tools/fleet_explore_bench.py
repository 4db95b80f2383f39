"""What the candidate exploration of a fleet costs: 1, 8 and 64 scenes x up to 5 candidates x 100 poses capacity x 60 point obstacles
(the tables of tests/fleet_cases.py: oracle_point_fleet; start at the scene's origin, goal 10 m ahead), default hcp parameters, both
graphs (ProbRoadmapGraph with given unit samples, lrKeyPointGraph), HSignature3d. Every repeat starts from handles without bands - the
exploration creates every candidate - and the bands are dropped again outside the timed region. max_paths = 64 bounds the depth-first
enumeration of the 122-vertex keypoint graphs. Median wall milliseconds of 20 repeats after 5 warm-ups.

  (a) fleet      one handle: ONE teb_amd_explore_candidates_per_scene call;
  (b) handles    teb_amd_explore_candidates on each of N single-scene handles in turn, same library;
  (c) parent     the same as (b) with another build of the library (--parent-lib: the parent commit's libteb_amd.so), twice: the
                 guard for the single-scene path, which shares its host rules with the per-scene call;
  (d) parent     the same as (a) with that library, twice: the guard for the per-scene path.
  quota          (a) at 64 scenes with 4, 8 and 16 paths per scene and round (teb_amd_debug_set_explore_quota).

digest: the first 16 hex digits of a SHA-256 over what the last exploration of the cell left, scene by scene: the counts of bands,
vertices and examined paths, the graph (vertices, adjacency bytes) and every band's pose count and x / y / theta / dt up to it. (b) and
(c), (a) and (d) of the same inputs must agree - the two libraries compute the same bits -; the run ends with an error if they do not.

Every cell runs in a process of its own under a time limit; the first cell that fails ends the run.
    python tools/fleet_explore_bench.py [--parent-lib PATH] [--out profiles/fleet_explore_times.txt]"""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

REPEATS, WARMUP, CELL_TIMEOUT_S = 20, 5, 240
POSES, MAX_PATHS, LENGTH = 100, 64, 10.0


def worker(variant, n_scenes, keypoint, quota):
    import numpy as np
    import fleet_cases
    from teb_local_planner_amd import planner
    f = fleet_cases.oracle_point_fleet(n_scenes=n_scenes)
    cfg = f.cfg
    cfg.hcp.simple_exploration = bool(keypoint)
    hp = cfg.hcp
    mo, mv, mw = f.capacities()
    starts = np.array([(x, y, 0.0) for x, y in f.origins])
    goals = starts + np.array([LENGTH, 0.0, 0.0])
    us = np.random.default_rng(5).random((n_scenes, 2 * hp.roadmap_graph_no_samples))
    solvers = []
    if variant == "a":
        s = planner.TebBatchSolver(cfg, n_scenes * hp.max_number_classes, POSES, mo, mv, mw)
        s.set_scenes(f.tables, f.vias)
        if quota:
            s.debug_set_explore_quota(quota)
        solvers.append(s)
    else:
        for sc in range(n_scenes):
            s = planner.TebBatchSolver(cfg, hp.max_number_classes, POSES, max(len(f.tables[sc]), 1), 1, 1)
            s.set_obstacles(f.tables[sc]); s.set_via_points([])
            solvers.append(s)

    counts = np.zeros((n_scenes, 3), np.int64)   # bands, vertices, examined paths of every scene in the last exploration

    def explore():
        if variant == "a":
            r = solvers[0].explore_candidates_per_scene(starts, goals, unit_samples=us, max_paths=MAX_PATHS)
            counts[:] = np.stack([r["n_bands"], r["n_vertices"], r["n_paths"]], 1)
            return int(r["n_total"]), int(r["n_paths"].sum())
        for sc, s in enumerate(solvers):
            r = s.explore_candidates(starts[sc], goals[sc], unit_samples=us[sc], max_paths=MAX_PATHS)
            counts[sc] = r["n_total"], r["n_vertices"], r["n_paths"]
        return int(counts[:, 0].sum()), int(counts[:, 2].sum())

    def digest():
        from teb_local_planner_amd import _abi
        h = hashlib.sha256()
        for sc in range(n_scenes):
            s = solvers[0] if variant == "a" else solvers[sc]
            mine = np.nonzero(s.band_scenes()[:s.count] == sc)[0] if variant == "a" else np.arange(s.count)
            V, A = s.exploration_graph_per_scene(sc) if variant == "a" else s.exploration_graph()
            h.update(counts[sc].tobytes() + np.ascontiguousarray(V, np.float64).tobytes() + np.ascontiguousarray(A, np.uint8).tobytes())
            host = _abi.TebBatchHost(max(s.count, 1), POSES)
            if s.count:
                s.download(host)
            for b in mine:
                strips = host.get_teb(int(b))
                h.update(np.int64(len(strips[0])).tobytes())
                for a in strips:
                    h.update(np.ascontiguousarray(a, np.float64).tobytes())
        return h.hexdigest()[:16]

    def drop():
        for s in solvers:
            if s.count:
                (s.compact_bands_per_scene if variant == "a" else s.compact_bands)(np.zeros(s.count, np.int32))
            s.synchronize()

    # one optimise step first: the shader clock the table quotes is the one of an optimise kernel on this device
    explore()
    solvers[0].optimize(1, 1)
    clock = float(solvers[0].last_shader_clock_mhz())
    drop()
    wall, total, paths = [], 0, 0
    for step in range(WARMUP + REPEATS):
        t0 = time.perf_counter()
        total, paths = explore()
        t1 = time.perf_counter()
        if step == WARMUP + REPEATS - 1:
            left = digest()
        drop()
        if step >= WARMUP:
            wall.append((t1 - t0) * 1e3)
    print(json.dumps({"variant": variant, "graph": "keypoint" if keypoint else "roadmap", "scenes": n_scenes, "quota": quota, "bands": total, "paths": paths,
                      "wall_ms": float(np.median(wall)), "wall_min_ms": float(min(wall)), "clock_mhz": clock, "digest": left}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker"); ap.add_argument("--scenes", type=int); ap.add_argument("--keypoint", type=int, default=0)
    ap.add_argument("--quota", type=int, default=0)
    ap.add_argument("--parent-lib", default=None, help="libteb_amd.so of the parent commit for (c) and (d); without it both are left out")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fleet_explore_times.txt"))
    a = ap.parse_args()
    if a.worker:
        return worker(a.worker, a.scenes, a.keypoint, a.quota)
    rows = []

    def cell(label, variant, n, keypoint, quota=0, lib=None):
        env = dict(os.environ)
        if lib:
            env["TEB_AMD_LIB"] = os.path.abspath(lib)
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", variant, "--scenes", str(n), "--keypoint", str(keypoint), "--quota",
                            str(quota)], capture_output=True, text=True, timeout=CELL_TIMEOUT_S, env=env)
        if p.returncode != 0:
            sys.stderr.write(p.stdout + p.stderr)
            sys.exit("cell (%s, %d scenes) ended with status %d: nothing more is started" % (label, n, p.returncode))
        r = json.loads(p.stdout.strip().splitlines()[-1])
        r["label"] = label
        rows.append(r)
        print(r, flush=True)

    for keypoint in (0, 1):
        for n in (1, 8, 64):
            cell("(a) fleet, one per-scene call", "a", n, keypoint)
            cell("(b) every handle in turn", "b", n, keypoint)
            if a.parent_lib:
                cell("(c) the same, parent library, run 1", "b", n, keypoint, lib=a.parent_lib)
                cell("(c) the same, parent library, run 2", "b", n, keypoint, lib=a.parent_lib)
                cell("(d) fleet, parent library, run 1", "a", n, keypoint, lib=a.parent_lib)
                cell("(d) fleet, parent library, run 2", "a", n, keypoint, lib=a.parent_lib)
                same = [r["digest"] for r in rows[-6:]]   # (a) (b) (c) (c) (d) (d) of these inputs
                if not (same[1] == same[2] == same[3] and same[0] == same[4] == same[5]):
                    sys.exit("%s, %d scenes: the two libraries left different bits: %s" % (rows[-1]["graph"], n, same))
    for keypoint in (0, 1):
        for q in (4, 8, 16):
            cell("(a) 64 scenes, %2d paths per round" % q, "a", 64, keypoint, quota=q)
    lines = ["# tools/fleet_explore_bench.py: scenes x up to 5 candidates x %d poses capacity x 60 point obstacles, default hcp parameters, 3-D" % POSES,
             "# signatures, max_paths = %d; one exploration from handles without bands; median wall ms of %d repeats after %d warm-ups;" % (MAX_PATHS, REPEATS, WARMUP),
             "# clock: shader clock of an optimise kernel in the same process [MHz]; bands / paths: created / examined over all scenes;",
             "# digest: SHA-256 (first 16 hex digits) over the counts, graphs and bands the last exploration left",
             "%-40s %9s %7s %6s %6s %9s %9s %7s  %s" % ("variant", "graph", "scenes", "bands", "paths", "wall ms", "min ms", "clock", "digest")]
    for r in rows:
        lines.append("%-40s %9s %7d %6d %6d %9.3f %9.3f %7.0f  %s" % (r["label"], r["graph"], r["scenes"], r["bands"], r["paths"], r["wall_ms"], r["wall_min_ms"],
                                                                    r["clock_mhz"], r["digest"]))
    by = {(r["label"][:3], r["graph"], r["scenes"]): r["wall_ms"] for r in rows if "per round" not in r["label"] and "run 2" not in r["label"]}
    for g in ("roadmap", "keypoint"):
        for n in (1, 8, 64):
            lines.append("# %s, %2d scenes: fleet / handles = %.2f" % (g, n, by[("(a)", g, n)] / by[("(b)", g, n)]))
    text = "\n".join(lines) + "\n"
    print(text)
    with open(a.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
