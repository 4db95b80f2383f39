"""The four costmap-to-obstacles entry points on this build against ANOTHER build of the library (--parent-lib: the parent commit's
libteb_amd.so, loaded through TEB_AMD_LIB): same inputs through both, a digest of what comes out and the wall time of the call.

Inputs: the maps of tools/fleet_polygons_bench.py (structured 120^2 and 400^2, random 2 % 120^2; 5 cm cells, the robot in the middle,
behind-robot distance 1.5 m, tile 8 on the polygon route); the single-scene calls on the map of robot 0, the set calls at 1, 8 and 64
scenes. Every cell (entry point, map, scenes) runs three times, each in a process of its own under a time limit: the parent's library,
this one, the parent's again. Per run:
  digest  sha256 over the counts, the out arrays and the installed table(s) as the device sees them - the 3-D H-signature of one short
          band per scene (one value per row: its centroid) and, for the single scene, the distance of a pose to every row;
  ms      median wall ms of the binding's call over REPEATS repeats after WARMUP warm-ups, each ended by a stream synchronisation.
A cell is level if this build lies no further above the parent's slower run than the parent's two runs lie apart; every cell that is
not runs a second pass in fresh processes, written out under the table. A process that fails or passes its limit ends the run.
    python tools/costmap_refactor_bench.py --parent-lib PATH [--out profiles/costmap_refactor_times.txt]"""
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

REPEATS, WARMUP, CELL_TIMEOUT_S, STRIDE, DIST, TILE = 10, 3, 180, 16, 1.5, 8
MAPS = (("structured", 120), ("structured", 400), ("random_0.02", 120))
ENTRIES = (("obstacles_from_costmap", (0,)), ("obstacles_from_costmap_polygons", (0,)), ("scenes_from_costmaps", (1, 8, 64)),
           ("scenes_from_costmap_polygons", (1, 8, 64)))   # scenes 0: the single scene


def worker(entry, kind, N, n):
    import numpy as np
    from fleet_polygons_bench import workload
    from teb_local_planner_amd import _abi, planner, scenes
    ns = max(n, 1)
    cfg, grids, poses, _, _, _ = workload(kind, N, ns)
    cfg.obstacles.include_dynamic_obstacles = True
    lethal = sum(int(np.count_nonzero(g.cells[:-1, :-1] == 254)) for g in grids)   # an upper bound of the kept cells of both routes
    out = dict(entry=entry, map=kind, grid=N, scenes=n, library=planner.TebBatchSolver.build_info()[1])
    h = hashlib.sha256()

    def add(*arrays):
        for a in arrays:
            a = np.ascontiguousarray(a)
            h.update(str((a.dtype, a.shape)).encode()); h.update(a.tobytes())
    try:
        s = planner.TebBatchSolver(cfg, ns, STRIDE, lethal + 1, 2 * lethal + 1, 1)
        if n == 0:
            s.set_costmap(grids[0].cells, grids[0].resolution, grids[0].origin_x, grids[0].origin_y)
        else:
            s.set_costmaps(grids)
        if entry == "obstacles_from_costmap":
            call = lambda: s.set_obstacles_from_costmap(poses[0], DIST)
            flat = lambda r: [np.array(r[0]), r[1], r[2]]
        elif entry == "obstacles_from_costmap_polygons":
            call = lambda: s.set_obstacles_from_costmap_polygons(poses[0], DIST, TILE)
            flat = lambda t: [np.asarray(getattr(t, k)) for k in ("type", "ax", "ay", "bx", "by", "vert_offset", "vert_x", "vert_y")]
        elif entry == "scenes_from_costmaps":
            call = lambda: s.set_scenes_from_costmaps(poses, DIST)
            flat = lambda r: [r[0]] + [a for p in r[1] for a in p]
        else:
            call = lambda: s.set_scenes_from_costmap_polygons(poses, DIST, TILE)
            flat = lambda ts: [np.asarray(getattr(t, k)) for t in ts for k in ("type", "ax", "ay", "bx", "by", "vert_offset", "vert_x", "vert_y")]
        got = flat(call())
        add(*got)
        out["rows"] = int(s._n_obst) if n == 0 else int(got[0].sum()) if entry == "scenes_from_costmaps" else int(sum(len(a) for a in got[0::8]))
        # the installed table(s): one short band per scene from the robot on, its 3-D H-signature has one value per row
        batch = _abi.TebBatchHost(ns, STRIDE)
        for b in range(ns):
            px, py, th, dt = scenes.sine_band(12, 2.0, 0.1, 1.0, cfg.robot.max_vel_x)
            batch.set_teb(b, px + poses[b][0], py + poses[b][1], th, dt)
        s.upload(batch)
        if n == 0:
            add(s.h_signatures())
            M = min(int(s._n_obst), 4096)
            if M:
                add(*s.debug_distance(np.arange(M), np.full(M, poses[0][0]), np.full(M, poses[0][1]), np.full(M, 0.3)))
        else:
            s.set_band_scenes(np.arange(ns))
            add(*s.h_signatures_per_scene())
        ts = []
        for step in range(WARMUP + REPEATS):
            s.synchronize()
            t0 = time.perf_counter(); call(); s.synchronize()
            if step >= WARMUP:
                ts.append((time.perf_counter() - t0) * 1e3)
        out["ms"] = float(np.median(ts))
        s.close()
    except planner.TebAmdError as e:   # (a handle with room for the rows cannot be created, or the call refuses: the same for both builds)
        h.update(("refused: %s" % e).encode())
        out["refused"] = str(e)
    out["digest"] = h.hexdigest()[:16]
    print(json.dumps(out), flush=True)


def run(cell, lib):
    """One process: its JSON line, or None when it failed or passed its limit (the run ends then)."""
    entry, kind, N, n = cell
    env = dict(os.environ)
    if lib:
        env["TEB_AMD_LIB"] = os.path.abspath(lib)
    try:
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", entry, "--map", kind, "--grid", str(N), "--scenes", str(n)],
                           capture_output=True, text=True, timeout=CELL_TIMEOUT_S, env=env)
    except subprocess.TimeoutExpired:
        return None, "passed its limit of %d s" % CELL_TIMEOUT_S
    done = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    if p.returncode != 0 or not done:
        sys.stderr.write(p.stderr)
        return None, "ended with status %d" % p.returncode
    return json.loads(done[-1]), None


def level(r):
    p1, t, p2 = r["parent1"].get("ms"), r["this"].get("ms"), r["parent2"].get("ms")
    return t is None or p1 is None or p2 is None or t <= max(p1, p2) + abs(p1 - p2)


def line(r):
    ms = lambda d: "%9.3f" % d["ms"] if d.get("ms") is not None else "  refused"
    same = r["this"]["digest"] == r["parent1"]["digest"] == r["parent2"]["digest"]
    return "%-32s %-12s %5d %6d %9s | %s %s %s | %-6s | %s %s %s" % (
        r["this"]["entry"], r["this"]["map"], r["this"]["grid"], r["this"]["scenes"], r["this"].get("rows", "-"), ms(r["parent1"]), ms(r["this"]),
        ms(r["parent2"]), "level" if level(r) else "ABOVE", r["this"]["digest"], r["parent1"]["digest"], "equal" if same else "DIFFERENT")


def report(rows, again, note, parent_lib):
    out = ["# tools/costmap_refactor_bench.py: this build (library %s) against %s (library %s)."
           % (rows[0]["this"]["library"] if rows else "-", os.path.basename(parent_lib), rows[0]["parent1"]["library"] if rows else "-"),
           "# Every figure from a process of its own, in the order parent, this, parent; ms: median wall ms of %d calls of the Python binding after %d"
           % (REPEATS, WARMUP),
           "# warm-ups; digest: sha256 over counts, out arrays and the installed table(s); scenes 0: the single-scene call. level: this build no further",
           "# above the parent's slower run than the parent's two runs lie apart.",
           "%-32s %-12s %5s %6s %9s | %9s %9s %9s | %-6s | %-16s %-16s %s" % ("entry point (teb_amd_set_..)", "map", "grid", "scenes", "rows", "parent", "this",
                                                                            "parent", "", "digest this", "digest parent", "")]
    out += [line(r) for r in rows]
    if again:
        out.append("# second pass of the cells above the margin, fresh processes:")
        out += [line(r) for r in again]
    if note:
        out.append("# " + note)
    return "\n".join(out) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker"); ap.add_argument("--map"); ap.add_argument("--grid", type=int); ap.add_argument("--scenes", type=int)
    ap.add_argument("--parent-lib", default=None, help="libteb_amd.so of the parent commit")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "costmap_refactor_times.txt"))
    a = ap.parse_args()
    if a.worker:
        return worker(a.worker, a.map, a.grid, a.scenes)
    if not a.parent_lib:
        sys.exit("--parent-lib is required")
    cells = sorted(((e, k, N, n) for e, counts in ENTRIES for k, N in MAPS for n in counts), key=lambda c: c[2] * c[2] * max(c[3], 1))   # lightest first
    rows, again, note = [], [], None

    def three(cell, into):
        r = {}
        for key, lib in (("parent1", a.parent_lib), ("this", None), ("parent2", a.parent_lib)):
            r[key], why = run(cell, lib)
            if why:
                return "%s (%s) %s: nothing more was started" % (cell, key, why)
        into.append(r)
        print(line(r), flush=True)
        with open(a.out, "w") as fh:   # what is measured so far survives a later failure
            fh.write(report(rows, again, None, a.parent_lib))
        return None
    for cell in cells:
        note = three(cell, rows)
        if note:
            break
    if not note:
        for r in [r for r in rows if not level(r)]:
            note = three((r["this"]["entry"], r["this"]["map"], r["this"]["grid"], r["this"]["scenes"]), again)
            if note:
                break
    text = report(rows, again, note, a.parent_lib)
    with open(a.out, "w") as fh:
        fh.write(text)
    print(text)
    if note:
        sys.exit(note)


if __name__ == "__main__":
    main()
