#!/usr/bin/env python3
"""teb_amd_plan_windows (every robot's plan window, local goal, via-points and pruning cursor from the resident global plans, one launch)
for 1 / 8 / 64 robots with global plans of 1 000 and 10 000 poses (5 cm apart) and a window of about 100 poses. Per cell the median
ms per call of the C call (call_ms: poses in, records and windows out, synchronous) and of the Python binding (binding_ms: + the per-robot lists)
in the steady state - the cursor already stands a prune distance behind the robot, what every tick but the first sees - and of the
first call after teb_amd_set_global_plans (cold_ms: the prune walks half the plan). host_numpy_ms is the same window cut on the host with
numpy, vectorised (what a caller did before: it then uploads the window with plan()); the sequential decisions are the device's, the
arithmetic is not held to its bits. Beside each figure stands the whole fleet tick of the same fleet size from
profiles/fleet_tick_times.txt (tick (a)), and the call's share of it. One JSON line per cell, then the table; --out writes the table.

    python tools/plan_window_times.py [--reps 21] [--batch 50] [--out profiles/plan_window_times.txt]"""
import argparse
import ctypes as C
import json
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from teb_local_planner_amd import _abi, planner  # noqa: E402
from teb_local_planner_amd.config import TebConfig  # noqa: E402

STEP, WINDOW = 0.05, 100


def _median_ms(fn, reps, before=None, batch=1):
    """median and minimum ms per call over `reps` samples after three warm-up samples; a sample is `batch` calls back to back, so that
    the timed window (a few ms) is long against the timer and the scheduler. before: run ahead of every call, untimed - then a sample
    is one call."""
    ts = []
    for k in range(reps + 3):   # three warm-ups (first launch, allocations)
        if before is not None:
            before()
            t0 = time.perf_counter(); fn(); t = time.perf_counter() - t0
        else:
            t0 = time.perf_counter()
            for _ in range(batch):
                fn()
            t = (time.perf_counter() - t0) / batch
        if k >= 3:
            ts.append(t)
    return 1e3 * float(np.median(ts)), 1e3 * float(np.min(ts))


def _tick_totals():
    """{scenes: wall ms} of 'tick (a)' in profiles/fleet_tick_times.txt"""
    out = {}
    p = os.path.join(ROOT, "profiles", "fleet_tick_times.txt")
    if os.path.exists(p):
        for line in open(p):
            m = re.match(r"tick\s+\(a\).*?\s(\d+)\s+([\d.]+)\s+[\d.]+\s+\d+\s*$", line)
            if m:
                out[int(m.group(1))] = float(m.group(2))
    return out


def _host_numpy(plan, begin, pose, thr, prune):
    """the same cut with numpy: prune match, closest pose with the early break, distance cut, identity transform"""
    x, y, yaw = (a[begin:] for a in plan)
    d = (pose[0] - x) ** 2 + (pose[1] - y) ** 2
    hit = np.nonzero(d < prune * prune)[0]
    if len(hit):
        x, y, yaw, d = x[hit[0]:], y[hit[0]:], yaw[hit[0]:], d[hit[0]:]
    m = np.minimum.accumulate(d)
    new = np.concatenate([[d[0] < 1e10], d[1:] < m[:-1]])
    reach = np.nonzero(new & (d < 0.05))[0]
    end = len(d)
    if len(reach):
        later = np.nonzero(d[reach[0] + 1:] > m[reach[0]:-1])[0]
        if len(later):
            end = reach[0] + 1 + later[0]
    i = int(np.argmin(d[:end]))
    cut = np.nonzero(d[i:] > thr * thr)[0]
    k = i + cut[0] + 1 if len(cut) else len(d)
    return x[i:k].copy(), y[i:k].copy(), yaw[i:k].copy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--batch", type=int, default=50, help="calls per timed sample")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    ticks = _tick_totals()
    binary_hash = planner.TebBatchSolver.build_info()[0]
    print(json.dumps(dict(binary_hash=binary_hash, reps=args.reps, batch=args.batch)), flush=True)
    rows = []
    wp = _abi.PlanWindowParams(max_global_plan_lookahead_dist=0.0, global_plan_viapoint_sep=1.0)
    for n_poses in (1000, 10000):
        for robots in (1, 8, 64):
            s = planner.TebBatchSolver(TebConfig(), robots, 32, 1, 1, 1)
            k = np.arange(n_poses, dtype=np.float64)
            plans = [(STEP * k + 3.0 * r, np.full(n_poses, 2.0 * r), np.zeros(n_poses)) for r in range(robots)]
            at = n_poses // 2
            poses = np.array([(p[0][at], p[1][at] + 0.01, 0.1) for p in plans])
            thr = np.full(robots, STEP * (WINDOW - 1) + 0.5 * STEP)
            s.set_global_plans(plans)
            first = s.plan_windows(poses, thr, wp)
            assert (first["window_count"] == WINDOW + 1).all() and (first["cursor"] == at - 19).all(), (first["window_count"], first["cursor"])
            cap = int(first["offset"][-1])
            o = {q: np.zeros(robots, np.int32) for q in ("w", "g", "c", "p", "v")}
            off = np.zeros(robots + 1, np.int32); voff = np.zeros(robots + 1, np.int32)
            goal = np.zeros(3 * robots); gg = np.zeros(3 * robots)
            wx, wy, wyaw, vx, vy = (np.zeros(cap) for _ in range(5))
            I = lambda a: _abi._ptr(a, C.c_int32)
            D = lambda a: _abi._ptr(a, C.c_double)
            f = planner.lib().teb_amd_plan_windows
            cargs = (s._h, robots, C.byref(wp), D(poses), None, D(thr), I(o["w"]), I(o["g"]), I(o["c"]), I(o["p"]), D(goal), D(gg), I(o["v"]), I(off),
                     D(wx), D(wy), D(wyaw), cap, I(voff), D(vx), D(vy), cap)

            def call():
                if f(*cargs) != _abi.OK:
                    raise RuntimeError(planner.lib().teb_amd_last_error())
            call_ms, call_min = _median_ms(call, args.reps, batch=args.batch)
            binding_ms, _ = _median_ms(lambda: s.plan_windows(poses, thr, wp), args.reps, batch=args.batch)
            cold_ms, _ = _median_ms(call, args.reps, before=lambda: s.set_global_plans(plans))
            cur = s.plan_cursors()
            host_ms, _ = _median_ms(lambda: [_host_numpy(plans[r], int(cur[r]), poses[r], thr[r], 1.0) for r in range(robots)], args.reps,
                                    batch=args.batch)
            tick = ticks.get(robots)
            row = dict(poses=n_poses, robots=robots, window=int(o["w"][0]), call_ms=round(call_ms, 4), call_min_ms=round(call_min, 4),
                       binding_ms=round(binding_ms, 4), cold_ms=round(cold_ms, 4), host_numpy_ms=round(host_ms, 4), tick_ms=tick,
                       share_of_tick=None if not tick else round(call_ms / tick, 4))
            print(json.dumps(row), flush=True)
            rows.append(row)
            s.close()
    head = ("# tools/plan_window_times.py: teb_amd_plan_windows, plans of N poses 5 cm apart, the robot at the middle, a window of %d poses,\n"
            "# one via-point per metre; ms per call: median over %d samples of %d calls back to back, after 3 warm-up samples (the call is\n"
            "# synchronous); cold: the first call after teb_amd_set_global_plans (the prune walks N / 2 poses), ONE call per sample - a 0.1 ms\n"
            "# window, read it to +- 0.01 ms; host numpy: the same cut vectorised on the host, robot by robot;\n"
            "# tick: 'tick (a)' of profiles/fleet_tick_times.txt at the same fleet size; library %s\n" % (WINDOW + 1, args.reps, args.batch, binary_hash))
    table = head + "%7s %7s %10s %10s %10s %10s %12s %9s %7s\n" % ("poses", "robots", "call ms", "min ms", "binding ms", "cold ms", "host numpy", "tick ms", "share")
    for r in rows:
        table += "%7d %7d %10.3f %10.3f %10.3f %10.3f %12.3f %9s %7s\n" % (
            r["poses"], r["robots"], r["call_ms"], r["call_min_ms"], r["binding_ms"], r["cold_ms"], r["host_numpy_ms"],
            "-" if r["tick_ms"] is None else "%.3f" % r["tick_ms"], "-" if r["share_of_tick"] is None else "%.1f %%" % (100 * r["share_of_tick"]))
    print(table)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(table)


if __name__ == "__main__":
    main()
