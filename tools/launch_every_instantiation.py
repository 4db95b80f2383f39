"""Launch EVERY pre-built instantiation of teb_optimize_kernel (layout x Jacobian mode x scene kind, csrc/teb_opt_launch.hpp) on the GPU
and record what each launch returned; tests/test_gpu_every_instantiation.py judges the records.
Why: a miscompiled unit (profiles/fault_bisect_r05.txt: the no-callee-saved call of the out-of-line solve under interprocedural register
allocation; which unit is hit moves with its register allocation) can abort the process with a memory aperture violation at the first
solve, or corrupt a live register and return finite, wrong poses. So every case runs the configuration's own schedule (no_inner_iterations
x no_outer_iterations) on the rarely used paths where a kind has them (cost exponent != 1 -> pow(), shortest path, via-points), and
  - every case that lands on a specialised kind (4 .. 11) is launched again with generic_config_path (its TWIN: same scene, layout pin and
    helper options; the generic kinds are built on the plain convention, -DTEB_AMD_SOLVE_CSR) - the test wants the twin's bits;
  - the scenes of the layouts with helper workgroups run with helpers (small-batch kind) and without (full-batch kind) - the test wants
    the same bits from both; distance helpers (multi_cu) only on single-band scenes (the known multi-band defect);
  - the test compares every case with the CPU oracle in the case's own Jacobian mode.
Each launch is written to <out>/<layout>_<case index>.npz (<..>_twin.npz for the twin): the bands (n, x, y, theta, dt), the results
(status, lm_iterations, lm_trials, chi2, cost), debug_overflow_flags(), the instantiation and last_launch_info().
Usage (GPU box):  python tools/launch_every_instantiation.py [--out DIR]            every layout, each in a process of its own
                  python tools/launch_every_instantiation.py <layout> [--out DIR]   the cases of one layout (blocks | band | bandg) in this
                                                                                    process (a GPU fault ends it: its last line names the case)"""
import argparse
import collections
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
LAYOUTS = {"band": 0, "blocks": 1, "bandg": 2}
# scene kinds (csrc/teb_kernel.hpp): 0 points, 1 generic, 2 / 3 their small-batch twins, 4 .. 7 the same four on the TebConfig defaults,
# 8 / 9 wide, 10 / 11 light
# (band in HBM, layout 2, runs without solver helpers - mcu_helpers_for, csrc/teb_amd.hip - so its point-like small-batch kinds 2, 5, 9, 11
#  cannot be launched and are not built: build.py, csrc/teb_opt_launch.hpp)
EXPECTED = ({(lay, 0, k) for lay in range(3) for k in range(12)} | {(lay, 1, k) for lay in range(3) for k in (0, 1, 4)}) - {(2, 0, k) for k in (2, 5, 9, 11)}
# the generic kind a specialised kind's twin runs: same size class (full batch 0 / 1, small batch 2 / 3) and scene shape
TWIN_KIND = {4: 0, 5: 2, 6: 1, 7: 3, 8: 0, 9: 2, 10: 0, 11: 2}
# odd pose counts equal to the capacity (Nt = 4 n, Nt % 8 == 4: the padding of the normal matrix), autoResize off: {layout: ((poses,
# (kind with helpers, kind without)), ..)}. A 337-pose band in LDS leaves no room for the LDS cache of the 500 point obstacles
# (set_obstacles: fast_points = 0), so they take the generic-shape kinds.
ODD_CAPACITY = {"band": ((287, (5, 4)), (337, (7, 6))), "blocks": ((207, (5, 4)),), "bandg": ((401, (5, 4)), (513, (5, 4)))}
NO_HELPERS = {"speculative_trials": -1, "multi_cu": -1}

# label: unique in the layout; opts: _abi.Options keywords (layout pin included); expected: (Jacobian mode, kind); twin: launch it again with
# generic_config_path; pair: label of the case that runs the same scene without helpers (set on the run with helpers)
Case = collections.namedtuple("Case", "label cfg obst via batch opts expected twin pair")


def cases(layout):
    """The launches of one layout (CPU only: the test rebuilds this list to judge what the tool recorded)."""
    from teb_local_planner_amd import scenes, _abi
    lay = {"band": "band", "blocks": "cr", "bandg": "bandg"}[layout]
    stride = {"band": 288, "blocks": 208, "bandg": 400}[layout]
    helpers = layout != "bandg"   # (band in HBM: no solver helpers; its scenes with distance helpers are the generic-shape ones)

    def pts(**optim):
        c, o, v, b = scenes.scene_c4(B=8, n=120, stride=stride)
        if layout == "blocks":
            c.trajectory.teb_autosize = False
        for k, val in optim.items():
            setattr(c.optim, k, val)
        return c, o, v, b

    def pts_via():
        c, o, v, b = pts(weight_viapoint=1.0)
        b.via_points_enabled[:] = 1
        return c, o, [(5.0, 0.3), (10.0, -0.2)], b

    def poly(B, with_via=True, **optim):
        c, o, v, b = scenes.scene_small_mixed(B=B, n=40, stride=stride, footprint="polygon", with_via=with_via)
        for k, val in optim.items():
            setattr(c.optim, k, val)
        return c, o, v, b

    def odd(S):
        c, o, v, b = scenes.scene_c4(B=4, n=S, stride=S)
        c.trajectory.teb_autosize = False
        c.trajectory.max_samples = 1000
        return c, o, v, b

    def numeric(scene):
        scene[0].jacobian_mode = _abi.JACOBIAN_G2O_NUMERIC
        return scene

    out = []

    def add(label, scene, opts, expected, twin, pair=None):
        out.append(Case(label, *scene, dict(opts, layout=lay, fixed_layout=True), expected, twin, pair))

    def both(label, make, kinds, twin, with_helpers, opts=None):
        """the same scene with helpers (small-batch kind kinds[0]) where the layout has them, and without (full-batch kind kinds[1])"""
        opts = opts or {}
        if with_helpers is not None:
            add(label + " +helpers", make(), dict(opts, **with_helpers), (0, kinds[0]), twin, pair=label + " -helpers")
        add(label + " -helpers", make(), dict(opts, **NO_HELPERS), (0, kinds[1]), twin)

    # point-like scenes (solver helpers): defaults, wide (via-points), light (shortest path + cost exponent), generic (forced, cost exponent)
    sh = {} if helpers else None
    both("points defaults", pts, (5, 4), True, sh)
    both("points wide (via-points)", pts_via, (9, 8), True, sh)
    both("points light (shortest path, exponent)", lambda: pts(weight_shortest_path=1.0, obstacle_cost_exponent=1.5), (11, 10), True, sh)
    both("points generic (forced, exponent)", lambda: pts(obstacle_cost_exponent=1.5), (2, 0), False, sh, {"generic_config_path": True})
    # generic shapes on ONE band with two DISTANCE helpers (multi_cu = 2; + solver helpers where the layout has them): the only way to the
    # band-in-HBM layout's small-batch kinds; (via-points are not folded by the profile of the defaults)
    dh = {"multi_cu": 2}
    both("polygon defaults, one band", lambda: poly(1, with_via=False), (7, 6), True, dh)
    both("polygon generic (forced, exponent), one band", lambda: poly(1, obstacle_cost_exponent=1.5), (3, 1), False, dh,
         {"generic_config_path": True})
    # ... and on three bands without helpers (distance helpers on several bands: DESIGN.md section 8)
    add("polygon defaults, three bands -helpers", poly(3, with_via=False), NO_HELPERS, (0, 6), True)
    add("polygon generic (forced, exponent), three bands -helpers", poly(3, obstacle_cost_exponent=1.5),
        dict(NO_HELPERS, generic_config_path=True), (0, 1), False)
    # odd pose counts at the capacity, autoResize off
    for S, kinds in ODD_CAPACITY[layout]:
        both("points defaults, %d poses at capacity %d" % (S, S), lambda S=S: odd(S), kinds, True, sh)
    # the reference's own linearisation scheme (g2o central differences): full-batch kinds 0, 1, 4 (no helpers in this mode)
    add("numeric points defaults", numeric(pts()), {}, (1, 4), True)
    add("numeric points generic (forced, exponent)", numeric(pts(obstacle_cost_exponent=1.5)), {"generic_config_path": True}, (1, 0), False)
    add("numeric polygon", numeric(poly(3)), {}, (1, 1), False)
    return out


def launch(case, generic=False):
    """One optimize() of the case on the configuration's own schedule; generic: its twin. Returns the record (a dict of arrays)."""
    import numpy as np
    from teb_local_planner_amd import planner, _abi
    cfg = case.cfg
    opts = dict(case.opts, generic_config_path=True) if generic else case.opts
    s = planner.make_solver(cfg, case.obst, case.via, case.batch, options=_abi.Options(**opts))
    s.optimize(cfg.optim.no_inner_iterations, cfg.optim.no_outer_iterations, True, cfg.hcp.selection_obst_cost_scale,
               cfg.hcp.selection_viapoint_cost_scale, cfg.hcp.selection_alternative_time_cost)
    s.synchronize()
    inst = s.last_instantiation()
    info = s.last_launch_info()
    res = s.results()
    out = s.download(case.batch.copy())
    flags = s.debug_overflow_flags()
    s.close()
    rec = dict(label=np.array(case.label), generic=np.array(bool(generic)), instantiation=np.array(inst, np.int32),
               launch_info=np.array(info, np.int32), overflow=flags)
    for f in ("n", "x", "y", "theta", "dt"):
        rec[f] = getattr(out, f)
    for f in ("status", "lm_iterations", "lm_trials", "chi2", "cost"):
        rec[f] = getattr(res, f)
    return rec


def run_layout(layout, out_dir=None):
    import numpy as np
    from teb_local_planner_amd import _abi
    seen = set()
    for i, case in enumerate(cases(layout)):
        for generic in ((False, True) if case.twin else (False,)):
            what = "%s | %s%s" % (layout, case.label, " | generic twin" if generic else "")
            print("%s .." % what, flush=True)    # (a GPU fault ends the process: the last line says where)
            rec = launch(case, generic)
            if out_dir:
                np.savez(os.path.join(out_dir, "%s_%02d%s.npz" % (layout, i, "_twin" if generic else "")), **rec)
            ok = bool((rec["status"] == _abi.TEB_OK).all()) and all(np.isfinite(rec[f]).all() for f in ("x", "y", "theta", "dt", "cost"))
            print("%s -> instantiation %s helpers %s one-CU repeat %d rejected trials %d %s" % (
                what, tuple(rec["instantiation"].tolist()), tuple(rec["launch_info"][:2].tolist()), rec["launch_info"][2],
                int((rec["lm_trials"] - rec["lm_iterations"]).sum()), "ok" if ok else "BAD RESULT"), flush=True)
            if not generic:
                seen.add(tuple(rec["instantiation"].tolist()))
    missing = sorted(k for k in EXPECTED if k[0] == LAYOUTS[layout] and k not in seen)
    print("%s: launched %d instantiations; not reached: %s" % (layout, len(seen), missing), flush=True)
    return 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("layout", nargs="?", choices=sorted(LAYOUTS))
    ap.add_argument("--out", help="directory for the records (one .npz per launch)")
    a = ap.parse_args()
    if a.out:
        os.makedirs(a.out, exist_ok=True)
    if a.layout:
        sys.exit(run_layout(a.layout, a.out))
    rc = 0
    for layout in LAYOUTS:
        r = subprocess.run([sys.executable, __file__, layout] + (["--out", a.out] if a.out else []), capture_output=True, text=True, timeout=900)
        print(r.stdout.strip(), flush=True)
        if r.returncode != 0:
            rc = 1
            print("rc %d FAULT or failure in layout %s: %s" % (r.returncode, layout, ([l for l in r.stderr.splitlines() if "HSA_STATUS" in l or "Error" in l] or [""])[-1][-160:]), flush=True)
    sys.exit(rc)
