"""teb_amd_optimize_batch on this build against ANOTHER build of the library (--parent-lib: the parent commit's libteb_amd.so, loaded
through TEB_AMD_LIB): the same small batches through both, what comes out, what the host decided and the wall time of the call. The host
side of the launch (csrc/teb_launch_host.hpp and its driver in teb_amd.hip) is what differs between the two; the kernels are the same.

Cells: B = 1, 3, 16 bands of 20 - 60 poses against a point-like scene (30 points, point footprint) and a polygon scene (12 polygons +
8 points, polygon footprint), 5 inner x 4 outer iterations, on handles of 60 and 224 poses (blocks in LDS), 300 (band in LDS, launched
optimistically in blocks), 400 (band in HBM, launched optimistically in blocks) and 400 with band 0 made to outgrow the optimistic
layout (150 poses whose time differences call for a split of every interval: the launch is repeated in the handle's own layout);
the default configuration, and: via-points (the *_WIDE kinds), numeric Jacobians, a fleet launch over both scenes. multi_cu stays at
its default. Every cell runs three times, each in a process of its own under a time limit: the parent's library, this one, the
parent's again. Per run:
  digest    sha256 over the downloaded bands (pose counts, poses, time differences) and the results of the first call;
  decision  teb_amd_debug_last_instantiation, teb_amd_debug_last_config_profile, solver / distance helpers per band of
            teb_amd_last_launch_info; its "repeated" flag is printed, not compared (it is timing);
  ms        median wall ms of upload-free optimize() + synchronize() over REPEATS calls after WARMUP, every call from the same bands.
A cell is level if this build lies no further above the parent's slower run than the parent's two runs lie apart; every cell that is
not runs a second pass in fresh processes, written out under the table. A process that fails or passes its limit ends the run.
    python tools/launch_refactor_bench.py --parent-lib PATH [--out profiles/launch_refactor_times.txt]"""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPEATS, WARMUP, CELL_TIMEOUT_S, INNER, OUTER = 15, 3, 120, 5, 4
CAPS = ("60", "224", "300", "400", "400grow")
CELLS = ([("default", scene, cap, B) for cap in CAPS for scene in ("points", "polygon") for B in (1, 3, 16)]
         + [("via", "points", "224", 3), ("via", "points", "400", 16), ("numeric", "polygon", "224", 3), ("fleet", "both", "224", 16)])


def tables(cfg):
    """The two obstacle tables: 30 points (2 of them moving); 12 triangles / quadrilaterals + 8 points. Clear of the x axis by 0.4 m."""
    import numpy as np
    from teb_local_planner_amd import _abi
    rng = np.random.default_rng(41)
    side = lambda: rng.choice((-1.0, 1.0)) * rng.uniform(0.4, 2.5)
    points, polygons = _abi.ObstacleTable(), _abi.ObstacleTable()
    for k in range(30):
        points.add_point(rng.uniform(0.5, 7.5), side(), vel=(0.05, -0.08) if k >= 28 else None)
    for k in range(12):
        cx, cy, r, m, rot = rng.uniform(0.5, 7.5), side() * 1.3, rng.uniform(0.1, 0.3), int(rng.integers(3, 5)), rng.uniform(0.0, 6.28)
        polygons.add_polygon([(cx + r * np.cos(rot + 6.283185307179586 * j / m), cy + r * np.sin(rot + 6.283185307179586 * j / m)) for j in range(m)])
    for k in range(8):
        polygons.add_point(rng.uniform(0.5, 7.5), side())
    return points, polygons


def worker(config, scene, cap, B):
    import numpy as np
    from teb_local_planner_amd import _abi, planner, scenes
    from teb_local_planner_amd.config import RobotFootprintModel, TebConfig
    cfg = TebConfig()
    cfg.obstacles.include_dynamic_obstacles = True
    cfg.trajectory.max_samples = 500
    if scene == "polygon":
        cfg.robot_model = RobotFootprintModel.polygon([(-0.2, -0.15), (0.4, -0.15), (0.4, 0.15), (-0.2, 0.15)])
    if config == "numeric":
        cfg.jacobian_mode = _abi.JACOBIAN_G2O_NUMERIC
    via = []
    if config == "via":
        cfg.optim.weight_viapoint = 1.0
        via = [(2.0, 0.2), (4.0, -0.15), (6.0, 0.2)]
    points, polygons = tables(cfg)
    stride = int(cap[:3])
    batch = _abi.TebBatchHost(B, stride)
    rng = np.random.default_rng(100 + B)
    for b in range(B):
        n = 20 + (b * 13) % 41   # 20 .. 60 poses
        batch.set_teb(b, *scenes.sine_band(n, 8.0, rng.uniform(-0.3, 0.3), float(rng.integers(1, 4)), cfg.robot.max_vel_x))
        batch.has_vel_goal[b] = 1
    if cap.endswith("grow"):   # autoResize halves every interval of 0.75 s: ~ 300 poses, more than the blocks hold
        x, y, th, dt = scenes.sine_band(150, 30.0, 0.2, 1.0, cfg.robot.max_vel_x)
        batch.set_teb(0, x, y, th, dt * 0 + 0.75)
    out = dict(config=config, scene=scene, cap=cap, B=B, library=planner.TebBatchSolver.build_info()[1])
    if config == "fleet":
        s = planner.TebBatchSolver(cfg, B, stride, len(points) + len(polygons), len(polygons.vert_x) + 1, 1)
        s.set_scenes([points, polygons])
        s.upload(batch)
        s.set_band_scenes(np.arange(B) % 2)
    else:
        s = planner.make_solver(cfg, points if scene == "points" else polygons, via, batch)
    ts = []
    for step in range(WARMUP + REPEATS):
        s.upload(batch)
        s.synchronize()
        t0 = time.perf_counter(); s.optimize(INNER, OUTER, True, 100.0, 1.0, False); s.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
        if step == 0:
            res, got = s.results(), s.download(batch.copy())
            h = hashlib.sha256()
            for a in [got.n, res.status, res.lm_iterations, res.lm_trials, res.chi2, res.cost, res.lambda_] + [v for b in range(B) for v in got.get_teb(b)]:
                a = np.ascontiguousarray(a)
                h.update(str((a.dtype, a.shape)).encode()); h.update(a.tobytes())
            out["digest"] = h.hexdigest()[:16]
            out["n_max"] = int(got.n.max())
            D, K, repeated = s.last_launch_info()
            out["decision"] = "inst %d/%d/%d profile %d K %d D %d" % (s.last_instantiation() + (s.last_config_profile(), K, D))
            out["repeated"] = int(repeated)
    out["ms"] = float(np.median(ts[WARMUP:]))
    s.close()
    print(json.dumps(out), flush=True)


def run(cell, lib):
    """One process: its JSON line, or None when it failed or passed its limit (the run ends then)."""
    config, scene, cap, B = cell
    env = dict(os.environ)
    if lib:
        env["TEB_AMD_LIB"] = os.path.abspath(lib)
    try:
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", config, "--scene", scene, "--cap", cap, "--bands", str(B)],
                           capture_output=True, text=True, timeout=CELL_TIMEOUT_S, env=env)
    except subprocess.TimeoutExpired:
        return None, "passed its limit of %d s" % CELL_TIMEOUT_S
    done = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    if p.returncode != 0 or not done:
        sys.stderr.write(p.stderr)
        return None, "ended with status %d" % p.returncode
    return json.loads(done[-1]), None


def level(r):
    p1, t, p2 = r["parent1"]["ms"], r["this"]["ms"], r["parent2"]["ms"]
    return t <= max(p1, p2) + abs(p1 - p2)


def same(r):
    return all(r["this"][k] == r["parent1"][k] == r["parent2"][k] for k in ("digest", "decision"))


def line(r):
    t = r["this"]
    return "%-8s %-8s %-8s %3d %5d | %8.3f %8.3f %8.3f | %-6s | %-34s %d%d%d | %s %s %s" % (
        t["config"], t["scene"], t["cap"], t["B"], t["n_max"], r["parent1"]["ms"], t["ms"], r["parent2"]["ms"], "level" if level(r) else "ABOVE",
        t["decision"], r["parent1"]["repeated"], t["repeated"], r["parent2"]["repeated"], t["digest"], r["parent1"]["digest"], "equal" if same(r) else "DIFFERENT")


def report(rows, again, note, parent_lib):
    out = ["# tools/launch_refactor_bench.py: this build (library %s) against %s (library %s)."
           % (rows[0]["this"]["library"] if rows else "-", os.path.basename(parent_lib), rows[0]["parent1"]["library"] if rows else "-"),
           "# Every figure from a process of its own, in the order parent, this, parent; ms: median wall ms of optimize(%d, %d) + synchronize() over %d"
           % (INNER, OUTER, REPEATS),
           "# calls after %d warm-ups; n max: the longest band afterwards; decision: (layout / Jacobian mode / scene kind) of the instantiation, configuration"
           % WARMUP,
           "# profile, solver (K) and distance (D) helpers per band; rep: the launch was repeated for late helpers (parent, this, parent - timing, not",
           "# compared); digest: sha256 over bands and results; equal: digest AND decision as both parent runs. level: this build no further above the",
           "# parent's slower run than the parent's two runs lie apart.",
           "%-8s %-8s %-8s %3s %5s | %8s %8s %8s | %-6s | %-34s %-3s | %-16s %-16s" % ("config", "scene", "capacity", "B", "n max", "parent", "this", "parent", "",
                                                                                  "decision", "rep", "digest this", "digest parent")]
    out += [line(r) for r in rows]
    if again:
        out.append("# second pass of the cells above the margin, fresh processes:")
        out += [line(r) for r in again]
    if rows:
        out.append("# %d cells, %d with digest and decision equal to the parent's, %d level in the first pass%s" % (
            len(rows), sum(same(r) for r in rows), sum(level(r) for r in rows), (", %d of %d level in the second" % (sum(level(r) for r in again), len(again))) if again else ""))
    if note:
        out.append("# " + note)
    return "\n".join(out) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker"); ap.add_argument("--scene"); ap.add_argument("--cap"); ap.add_argument("--bands", type=int)
    ap.add_argument("--parent-lib", default=None, help="libteb_amd.so of the parent commit")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "launch_refactor_times.txt"))
    a = ap.parse_args()
    if a.worker:
        return worker(a.worker, a.scene, a.cap, a.bands)
    if not a.parent_lib:
        sys.exit("--parent-lib is required")
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
    for cell in CELLS:
        note = three(cell, rows)
        if note:
            break
    if not note:
        for r in [r for r in rows if not level(r)]:
            note = three((r["this"]["config"], r["this"]["scene"], r["this"]["cap"], r["this"]["B"]), again)
            if note:
                break
    text = report(rows, again, note, a.parent_lib)
    with open(a.out, "w") as fh:
        fh.write(text)
    print(text)
    if note:
        sys.exit(note)
    if not all(same(r) for r in rows + again):
        sys.exit("a digest or a decision differs from the parent's")


if __name__ == "__main__":
    main()
