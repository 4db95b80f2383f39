"""The first half of a planner tick - renewAndAnalyzeOldTebs - on this build against ANOTHER build of the library (--parent-lib: the
parent commit's libteb_amd.so, loaded through TEB_AMD_LIB), for the single scene and for scene sets. The host side of the four steps
(csrc/teb_hcp_host.hpp: SignatureSet, BandGroups, compaction_map, and their callers in teb_amd.hip) is what differs; the kernels are
the same.

Cells: one single-scene handle with 4 and with 16 bands; fleet handles of 1 / 8 / 64 scenes x 4 bands; 100 poses and 60 point
obstacles per scene (tests/fleet_cases.py: oracle_point_fleet); HSignature3d (3-D) and HSignature (2-D). One sequence, as
exploreEquivalenceClassesAndInitTebs issues it: compute signatures, class filter (max_number_plans_in_current_class 1 and 2), detour
filter, compaction with a best band per planner (its second band), then one feasibility call for every planner's best band against a
120 x 120 grid. Per process:
  digest  sha256 over the signature values; keep / valid / reasonable of both class filters; the detour keep; n_kept, new_best and the
          band -> scene map; the downloaded bands after the compaction; the feasibility answers - of the first sequence;
  ms      median wall ms of REPEATS sequences after WARMUP; every sequence starts from the uploaded bands (upload outside the clock).
Three processes per cell, the level rule and the second pass: tools/refactor_bench.py.
    python tools/renew_refactor_bench.py --parent-lib PATH [--out profiles/renew_refactor_times.txt]"""
import argparse
import hashlib
import json
import os
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import refactor_bench as RB  # noqa: E402

REPEATS, WARMUP, CELL_TIMEOUT_S = 20, 5, 120
CELLS = [(kind, n, mode) for mode in (3, 2) for kind, n in (("single", 4), ("single", 16), ("fleet", 1), ("fleet", 8), ("fleet", 64))]
FOOTPRINT, INSCRIBED = [(-0.2, -0.15), (0.4, -0.15), (0.4, 0.15), (-0.2, 0.15)], 0.15


def grid(origin, seed):
    """120 x 120 cells of 0.1 m round a scene's bands (10 m along x from its origin), about one cell in 200 lethal"""
    import numpy as np
    cells = np.where(np.random.default_rng(seed).random((120, 120)) < 0.005, 254, 0).astype(np.uint8)
    return types.SimpleNamespace(cells=cells, resolution=0.1, origin_x=origin[0] - 1.0, origin_y=origin[1] - 6.0)


def worker(kind, n, mode):
    import numpy as np
    import fleet_cases
    from teb_local_planner_amd import _abi, planner
    fleet = kind == "fleet"
    f = fleet_cases.oracle_point_fleet(n_scenes=n) if fleet else fleet_cases.oracle_point_fleet(n_scenes=1, per_scene=n)
    cfg, B = f.cfg, f.batch.count
    cfg.obstacles.include_dynamic_obstacles = mode == 3
    hp = cfg.hcp
    mo, mv, mw = f.capacities()
    s = planner.TebBatchSolver(cfg, B, f.batch.stride, mo, mv, mw)
    grids = [grid(f.origins[sc], 900 + sc) for sc in range(f.n_scenes)]
    if fleet:
        s.set_scenes(f.tables, f.vias)
        s.set_costmaps(grids)
        best = np.array([f.bands_of(sc)[1] for sc in range(f.n_scenes)], np.int32)
    else:
        s.set_obstacles(f.tables[0])
        s.set_costmap(grids[0].cells, grids[0].resolution, grids[0].origin_x, grids[0].origin_y)
        best = 1
    out = dict(kind=kind, n=n, mode=mode, B=B, library=planner.TebBatchSolver.build_info()[1])
    ts = []
    for step in range(WARMUP + REPEATS):
        s.upload(f.batch)
        if fleet:
            s.set_band_scenes(f.scene_of)
        s.set_optimized_flags(np.ones(B, np.int32))
        s.synchronize()
        t0 = time.perf_counter()
        if fleet:
            sig = s.h_signatures_per_scene(hp.h_signature_prescaler)
            c1 = s.filter_equivalence_classes_per_scene(hp.h_signature_threshold, best, 1)
            c2 = s.filter_equivalence_classes_per_scene(hp.h_signature_threshold, best, 2)
            kd = s.filter_detours_per_scene(c2[0], best)
            kept, nb = s.compact_bands_per_scene(kd, best)
            feas = s.is_trajectory_feasible_per_scene(nb, FOOTPRINT, INSCRIBED)
        else:
            sig = s.h_signatures(hp.h_signature_prescaler)
            c1 = s.filter_equivalence_classes(hp.h_signature_threshold, best, 1)
            c2 = s.filter_equivalence_classes(hp.h_signature_threshold, best, 2)
            kd = s.filter_detours(c2[0], best)
            kept, nb = s.compact_bands(kd, best)
            feas = s.is_trajectory_feasible(max(nb, 0), FOOTPRINT, INSCRIBED)
        ts.append((time.perf_counter() - t0) * 1e3)
        if step == 0:
            got = s.download(_abi.TebBatchHost(kept, f.batch.stride))
            parts = (list(sig) + list(c1) + list(c2) + [kd, [kept], np.atleast_1d(nb), s.band_scenes() if fleet else [0]]
                     + [got.n] + [v for b in range(kept) for v in got.get_teb(b)] + [np.asarray(a, np.int32) for a in feas])
            h = hashlib.sha256()
            for a in parts:
                a = np.ascontiguousarray(a)
                h.update(str((a.dtype, a.shape)).encode()); h.update(a.tobytes())
            out["digest"] = h.hexdigest()[:16]
            out["kept"] = "%d/%d/%d/%d" % (int(c1[0].sum()), int(c2[0].sum()), int(kd.sum()), int(np.sum(np.asarray(feas[0], np.int32) == 1)))
    out["ms"] = float(np.median(ts[WARMUP:]))
    s.close()
    print(json.dumps(out), flush=True)


def line(r):
    t = r["this"]
    return "%-7s %3d %3d-D %4d | %8.3f %8.3f %8.3f | %-6s | %-14s | %s %s %s" % (
        t["kind"], t["n"], t["mode"], t["B"], r["parent1"]["ms"], t["ms"], r["parent2"]["ms"], "level" if RB.level(r) else "ABOVE", t["kept"],
        t["digest"], r["parent1"]["digest"], "equal" if RB.same(r) else "DIFFERENT")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", nargs=3, metavar=("KIND", "N", "MODE"))
    ap.add_argument("--parent-lib", default=None, help="libteb_amd.so of the parent commit")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "renew_refactor_times.txt"))
    a = ap.parse_args()
    if a.worker:
        return worker(a.worker[0], int(a.worker[1]), int(a.worker[2]))
    if not a.parent_lib:
        sys.exit("--parent-lib is required")

    def report(rows, again, note):
        lib = lambda k: rows[0][k]["library"] if rows else "-"
        out = ["# tools/renew_refactor_bench.py: this build (library %s) against %s (library %s)." % (lib("this"), os.path.basename(a.parent_lib), lib("parent1")),
               "# n: bands of the single scene / scenes x 4 bands of a fleet, 100 poses and 60 point obstacles per scene. Every figure from a process of",
               "# its own, in the order parent, this, parent; ms: median wall ms of %d sequences after %d warm-ups - signatures, class filter (1 and 2" % (REPEATS, WARMUP),
               "# plans per class), detour filter, compaction, one feasibility call (120 x 120 grid) -, every sequence from the uploaded bands.",
               "# kept: bands after class filter 1 / class filter 2 / detour filter / feasible best bands. digest: sha256 over signatures, every keep array,",
               "# n_kept, new_best, band -> scene map, the compacted bands and the feasibility answers. level: this build no further above the parent's",
               "# slower run than the parent's two runs lie apart.",
               "%-7s %3s %5s %4s | %8s %8s %8s | %-6s | %-14s | %-16s %-16s" % ("handle", "n", "dim", "B", "parent", "this", "parent", "", "kept", "digest this", "digest parent")]
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
