"""What a handle does with its bands OUTSIDE the optimise kernel, on this build against ANOTHER build of the library (--parent-lib: the
parent commit's libteb_amd.so, loaded through TEB_AMD_LIB). The owner of the device memory (csrc/teb_scene_store.hpp: DevBuf), the band
store (csrc/teb_band_store.hpp) and their callers in teb_amd.hip are what differs between the two; the kernels are the same.

Warm cells (median wall ms of REPEATS calls after WARMUP on one handle):
  updown packed / strided   upload + download of 16 bands x 40 poses through the packed message (rows of 64) / of 32 bands through the
                            strided copies (rows of 944: the message would exceed its buffer);
  snapshot                  snapshot + restore of a 64-band handle of 128 poses;
  compact                   a compaction of 16 bands that drops two and moves the best band (7) to the front; re-uploaded outside the clock;
  explore single / fleet 1 / fleet 8   one exploration tick from a handle without bands (tests/fleet_cases.py: oracle_point_fleet, 60 point
                            obstacles per scene, goal 10 m ahead, given unit samples, max_paths 64); the bands are dropped outside the clock;
  outgrow                   an optimise call (5 x 4) of 3 bands on a 400-pose handle whose band 0 outgrows the optimistic layout: the
                            launch is repeated from the saved strips.
Cold cells (median of COLD_REPEATS after COLD_WARMUP, every repeat on a handle of its own - where the allocation changes land):
  create                    create + destroy of a handle (64 bands x 128 poses x 60 obstacles);
  first compact             the first compaction of a fresh handle (it allocates the compaction scratch: 19 buffers, 11 in the parent);
  first explore             the first exploration of a fresh handle (it allocates the candidate scratch).
digest: sha256 over what the first timed call left - pose counts, band flags, optimized flags, every band up to its pose count and,
where an optimise call ran, the results; of an exploration also its counts and its graph.
Three processes per cell, the level rule and the second pass: tools/refactor_bench.py.
    python tools/handle_refactor_bench.py --parent-lib PATH [--out profiles/handle_refactor_times.txt]"""
import argparse
import hashlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import refactor_bench as RB  # noqa: E402

REPEATS, WARMUP, COLD_REPEATS, COLD_WARMUP, CELL_TIMEOUT_S = 20, 5, 10, 2, 180
CELLS = [("updown", "packed"), ("updown", "strided"), ("snapshot", "-"), ("compact", "-"), ("explore", "single"), ("explore", "fleet1"),
         ("explore", "fleet8"), ("outgrow", "-"), ("create", "cold"), ("compact", "cold"), ("explore", "cold")]
MAX_PATHS, LENGTH = 64, 10.0


def sine_batch(cfg, B, poses, stride, seed):
    import numpy as np
    from teb_local_planner_amd import _abi, scenes
    rng = np.random.default_rng(seed)
    batch = _abi.TebBatchHost(B, stride)
    for b in range(B):
        batch.set_teb(b, *scenes.sine_band(poses - (b % 5), 8.0, rng.uniform(-0.3, 0.3), float(rng.integers(1, 4)), cfg.robot.max_vel_x))
    batch.has_vel_goal[:] = rng.integers(0, 2, B); batch.via_points_enabled[:] = rng.integers(0, 2, B)
    batch.vel_start[:] = rng.uniform(-0.2, 0.2, (B, 3))
    return batch


def digest_of(s, stride, extra=(), results=False):
    import numpy as np
    from teb_local_planner_amd import _abi
    host = _abi.TebBatchHost(max(s.count, 1), stride)
    if s.count:
        s.download(host)
    parts = [s.pose_counts(), s.optimized_flags()] + list(s.band_flags()) + [v for b in range(s.count) for v in host.get_teb(b)] + list(extra)
    if results:
        r = s.results()
        parts += [r.status, r.lm_iterations, r.lm_trials, r.chi2, r.cost, r.lambda_]
    h = hashlib.sha256()
    for a in parts:
        a = np.ascontiguousarray(a)
        h.update(str((a.dtype, a.shape)).encode()); h.update(a.tobytes())
    return h.hexdigest()[:16]


def worker(cell, arg):
    import numpy as np
    import fleet_cases
    from teb_local_planner_amd import planner, scenes
    from teb_local_planner_amd.config import TebConfig
    cfg = TebConfig()
    cold = arg == "cold"
    repeats, warmup = (COLD_REPEATS, COLD_WARMUP) if cold else (REPEATS, WARMUP)
    out = dict(cell=cell, arg=arg, library=planner.TebBatchSolver.build_info()[1])
    ts = []

    def timed(call, step, digest):
        t0 = time.perf_counter()
        got = call()
        ts.append((time.perf_counter() - t0) * 1e3)
        if step == 0:
            out["digest"] = digest(got)

    if cell == "updown":
        B, stride = (16, 64) if arg == "packed" else (32, 944)
        batch = sine_batch(cfg, B, 40, stride, 7)
        s = planner.TebBatchSolver(cfg, B, stride, 4, 1, 1)
        back = batch.copy()
        for step in range(warmup + repeats):
            timed(lambda: (s.upload(batch), s.download(back)), step, lambda _: digest_of(s, stride))
        s.close()
    elif cell == "snapshot":
        batch = sine_batch(cfg, 64, 100, 128, 8)
        s = planner.TebBatchSolver(cfg, 64, 128, 4, 1, 1)
        s.upload(batch)
        for step in range(warmup + repeats):
            timed(lambda: (s.snapshot(), s.restore(), s.synchronize()), step, lambda _: digest_of(s, 128))
        s.close()
    elif cell == "compact":
        batch = sine_batch(cfg, 16, 100, 128, 9)
        keep = np.ones(16, np.int32); keep[[2, 11]] = 0
        s = None
        for step in range(warmup + repeats):
            if cold or s is None:
                s = planner.TebBatchSolver(cfg, 16, 128, 60, 1, 1)
            s.upload(batch); s.synchronize()
            timed(lambda: (s.compact_bands(keep, 7), s.synchronize())[0], step, lambda r: digest_of(s, 128, [np.array(r, np.int32)]))
            if cold:
                s.close()
        if not cold:
            s.close()
    elif cell == "explore":
        fleet = arg.startswith("fleet")
        ns = int(arg[5:]) if fleet else 1
        f = fleet_cases.oracle_point_fleet(n_scenes=ns)
        hp = f.cfg.hcp
        mo, mv, mw = f.capacities()
        starts = np.array([(x, y, 0.0) for x, y in f.origins])
        goals = starts + np.array([LENGTH, 0.0, 0.0])
        us = np.random.default_rng(5).random((ns, 2 * hp.roadmap_graph_no_samples))

        def make():
            s = planner.TebBatchSolver(f.cfg, ns * hp.max_number_classes, 100, mo, mv, mw)
            if fleet:
                s.set_scenes(f.tables, f.vias)
            else:
                s.set_obstacles(f.tables[0]); s.set_via_points([])
            return s

        def explore(s):
            if fleet:
                r = s.explore_candidates_per_scene(starts, goals, unit_samples=us, max_paths=MAX_PATHS)
                return [np.asarray(r[k], np.int64).ravel() for k in ("n_total", "n_bands", "n_vertices", "n_paths")]
            r = s.explore_candidates(starts[0], goals[0], unit_samples=us[0], max_paths=MAX_PATHS)
            return [np.array([r["n_total"], r["n_vertices"], r["n_paths"]], np.int64)]

        def left(s, counts):
            graphs = [s.exploration_graph_per_scene(sc) for sc in range(ns)] if fleet else [s.exploration_graph()]
            return digest_of(s, 100, counts + [a for g in graphs for a in g] + ([s.band_scenes()] if fleet else []))
        s = None
        for step in range(warmup + repeats):
            if cold or s is None:
                s = make()
            timed(lambda: explore(s), step, lambda counts: left(s, counts))
            if cold:
                s.close()
            else:
                (s.compact_bands_per_scene if fleet else s.compact_bands)(np.zeros(s.count, np.int32)); s.synchronize()
        if not cold:
            s.close()
    elif cell == "outgrow":
        cfg.trajectory.max_samples = 500
        rng = np.random.default_rng(41)
        from teb_local_planner_amd import _abi
        points = _abi.ObstacleTable()
        for k in range(30):
            points.add_point(rng.uniform(0.5, 7.5), rng.choice((-1.0, 1.0)) * rng.uniform(0.4, 2.5), vel=(0.05, -0.08) if k >= 28 else None)
        batch = sine_batch(cfg, 3, 60, 400, 10)
        x, y, th, dt = scenes.sine_band(150, 30.0, 0.2, 1.0, cfg.robot.max_vel_x)   # autoResize halves every interval of 0.75 s: ~ 300 poses
        batch.set_teb(0, x, y, th, dt * 0 + 0.75)
        s = planner.make_solver(cfg, points, [], batch)
        for step in range(warmup + repeats):
            s.upload(batch); s.synchronize()
            timed(lambda: (s.optimize(5, 4, True, 100.0, 1.0, False), s.synchronize()), step, lambda _: digest_of(s, 400, results=True))
        s.close()
    elif cell == "create":
        for step in range(warmup + repeats):
            def once():
                s = planner.TebBatchSolver(cfg, 64, 128, 60, 1, 1)
                cap = s.capacity()
                s.close()
                return cap
            timed(once, step, lambda cap: hashlib.sha256(repr(tuple(int(v) for v in cap)).encode()).hexdigest()[:16])
    else:
        sys.exit("unknown cell %s" % cell)
    out["ms"] = float(np.median(ts[warmup:]))
    print(json.dumps(out), flush=True)


def line(r):
    t = r["this"]
    return "%-8s %-8s | %9.3f %9.3f %9.3f | %-6s | %s %s %s" % (
        t["cell"], t["arg"], r["parent1"]["ms"], t["ms"], r["parent2"]["ms"], "level" if RB.level(r) else "ABOVE", t["digest"], r["parent1"]["digest"],
        "equal" if RB.same(r) else "DIFFERENT")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", nargs=2, metavar=("CELL", "ARG"))
    ap.add_argument("--parent-lib", default=None, help="libteb_amd.so of the parent commit")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "handle_refactor_times.txt"))
    a = ap.parse_args()
    if a.worker:
        return worker(*a.worker)
    if not a.parent_lib:
        sys.exit("--parent-lib is required")

    def report(rows, again, note):
        lib = lambda k: rows[0][k]["library"] if rows else "-"
        out = ["# tools/handle_refactor_bench.py: this build (library %s) against %s (library %s)." % (lib("this"), os.path.basename(a.parent_lib), lib("parent1")),
               "# Every figure from a process of its own, in the order parent, this, parent; ms: median wall ms of %d calls after %d warm-ups on one" % (REPEATS, WARMUP),
               "# handle, in the cold cells of %d after %d with a handle of its own per call. The cells: the docstring of the tool. level: this build" % (COLD_REPEATS, COLD_WARMUP),
               "# no further above the parent's slower run than the parent's two runs lie apart.",
               "%-8s %-8s | %9s %9s %9s | %-6s | %-16s %-16s" % ("cell", "", "parent", "this", "parent", "", "digest this", "digest parent")]
        out += [line(r) for r in rows]
        if again:
            out.append("# second pass of the cells above the margin, fresh processes:")
            out += [line(r) for r in again]
        if rows:
            out.append(RB.summary(rows, again))
        if note:
            out.append("# " + note)
        return "\n".join(out) + "\n"
    RB.three_way(__file__, CELLS, a.parent_lib, a.out, CELL_TIMEOUT_S, line, report)


if __name__ == "__main__":
    main()
