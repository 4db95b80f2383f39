"""Writes tests/golden/hp_strip_<family>.npz: what the restatement of the band producers and read-outs (tests/hp_strip.py, fp64 op by op
beside mpmath at 80 digits) gives on every case of tests/strip_threshold_cases.py. Run from the repository root:

    python tests/golden/make_hp_strip.py [substring of the case names to print; all files are always rewritten]

A case is written only if
  - the op-by-op fp64 run alone ("float") gives the same numbers as the fp64 half of the run with both evaluations;
  - every output that a libm result feeds is within ADMISSIBLE = 1e-13 of its 80-digit value and every output is below 100 in magnitude, so
    that the 1e-12 of the device tests keeps a tenfold margin over the reference alone;
  - the CPU oracle and, where oracle/_ref is built and the case is one the reference's code can run, the reference's own functions give
    the same band or read-out: bit for bit on the `exact` outputs, within 1e-13 on the others.
The generator stops otherwise. The fixtures hold data only: per file one array per field with the cases one after the other
(hp_strip.pack / unpack; "names" lists them). Per case:
  op [1]                         0 line, 1 plan, 2 path, 3 prune, 4 read-outs;  cap [1]: the pose capacity of the handle
  fargs, iargs                   the scalar arguments (see ARGS below; NaN: an optional argument that is absent)
  in_x, in_y, in_th, in_dt       the plan / path points or the band the case starts from
  status [1], n [1]              0 and the pose count; 1: refused by the kernel with the capacity error, pose count 0; 2: refused before
                                 the launch with the capacity error
  out_x, out_y, out_th, out_dt   the band afterwards (producers and prune);  ex_*: True where no libm result feeds the value
  cmd [4] (vx, vy, omega, ok), profile [(n + 1) * 3], traj [n * 7] with ex_cmd [3], ex_profile, ex_traj (read-outs; no traj for n = 1)
  summary [kinds, 8]             per kind (hp_strip.KINDS): comparisons, SEPARATED, EXACT, RUNG, ties in fp64, outcome true / false, the
                                 smallest separated margin
hp_strip_fleet.npz also holds, per fleet of strip_threshold_cases.FLEETS, "fleet_<name>" (its members, scene s = band s) and
"fleet_<name>_<key>" for what the call shares.
ARGS  line: fargs start[3] goal[3] diststep max_vel_x, iargs min_samples guess_backwards      plan: fargs max_vel_x max_vel_theta, iargs
      estimate_orient min_samples guess_backwards      path: fargs max_vel_x max_vel_theta max_acc_x start_orient goal_orient, iargs
      min_samples guess_backwards      prune: fargs new_start[3] new_goal[3], iargs min_samples      read-outs: fargs max_vel_y dt_ref
      vel_start[3] vel_goal[3], iargs look_ahead_poses prevent_look_ahead_poses_near_goal
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import hp_strip as HS  # noqa: E402
import strip_threshold_cases as SC  # noqa: E402

MAX_FILE_BYTES = 100 * 1000
STEM = "hp_strip_"
ADMISSIBLE = 1e-13
OPS = ["line", "plan", "path", "prune", "cons"]
BAND = ("out_x", "out_y", "out_th", "out_dt")
NAN3 = (np.nan, np.nan, np.nan)


def group_of(name):
    fam = name.split("_")[0]
    return STEM + (fam if fam != "lanes" else "lanes_" + {"line": "build", "plan": "build", "path": "build", "prune": "prune", "cons": "readout"}[SC.CASES[name]["op"]])


def groups():
    out = {}
    for name in SC.CASES:
        out.setdefault(group_of(name), []).append(name)
    return out


def load(stem):
    return HS.unpack(np.load(os.path.join(HERE, stem + ".npz")))


def _opt(v):
    return np.nan if v is None else float(v)


def inputs(c):
    op = c["op"]
    z = np.zeros(0)
    d = {"op": np.array([OPS.index(op)], np.int32), "cap": np.array([c["cap"]], np.int32), "in_x": z, "in_y": z, "in_th": z, "in_dt": z}
    if op == "line":
        d["fargs"] = np.array(c["start"] + c["goal"] + (c["diststep"], c["max_vel_x"]))
        d["iargs"] = np.array([c["min_samples"], c["back"]], np.int32)
    elif op == "plan":
        d.update(in_x=c["px"], in_y=c["py"], in_th=c["pyaw"], fargs=np.array([c["max_vel_x"], c["max_vel_theta"]]),
                 iargs=np.array([c["estimate"], c["min_samples"], c["back"]], np.int32))
    elif op == "path":
        d.update(in_x=c["px"], in_y=c["py"], fargs=np.array([c["max_vel_x"], c["max_vel_theta"], _opt(c["acc"]), _opt(c["so"]), _opt(c["go"])]),
                 iargs=np.array([c["min_samples"], c["back"]], np.int32))
    elif op == "prune":
        x, y, th, dt = c["band"]
        d.update(in_x=x, in_y=y, in_th=th, in_dt=dt, fargs=np.array((c["new_start"] or NAN3) + (c["new_goal"] or NAN3)),
                 iargs=np.array([c["min_samples"]], np.int32))
    else:
        x, y, th, dt = c["band"]
        d.update(in_x=x, in_y=y, in_th=th, in_dt=dt, fargs=np.array((c["max_vel_y"], c["dt_ref"]) + c["vs"] + c["vg"]),
                 iargs=np.array([c["look"], c["prevent"]], np.int32))
    return d


def outputs(r, hp):
    """the result of strip_threshold_cases.evaluate as arrays; with hp also the ex_* masks and (largest error of a libm-fed output, largest
    magnitude)"""
    d, worst = {}, [0.0, 0.0]

    def put(key, rows):
        d[key] = HS.values(rows).ravel() if len(rows) else np.zeros(0)
        if hp:
            d["ex_" + key.replace("out_", "")] = HS.exact_mask(rows).ravel() if len(rows) else np.zeros(0, bool)
            e, m = HS.worst_error(rows)
            worst[0], worst[1] = max(worst[0], e), max(worst[1], m)

    if r[0] == "refused":
        d["status"], d["n"] = np.array([2 if r[1] == "host" else 1], np.int32), np.array([0], np.int32)
    elif r[0] == "band":
        d["status"], d["n"] = np.array([0], np.int32), np.array([len(r[1])], np.int32)
        for key, rows in zip(BAND, r[1:]):
            put(key, rows)
    else:
        _, cmd, prof, traj = r
        d["status"], d["n"] = np.array([0], np.int32), np.array([len(prof) - 1], np.int32)
        put("cmd", list(cmd[1:]))
        d["cmd"] = np.append(d["cmd"], float(cmd[0]))
        put("profile", prof)
        put("traj", traj if traj is not None else [])
    return d, worst


def reference(name):
    """(case, expected arrays, [n, 8] records, events)"""
    c = SC.CASES[name]
    r, k = SC.evaluate(c, "both")
    want, (err, mag) = outputs(r, True)
    plain, _ = outputs(SC.evaluate(c, "float")[0], False)
    for key in plain:
        assert np.array_equal(plain[key], want[key]), (name, key)
    if not (err <= ADMISSIBLE and mag < 100.0):
        raise HS.InadmissibleError("%s: fp64 is %.3g from the 80-digit value, the largest magnitude is %.3g" % (name, err, mag))
    return c, want, k.record_array(), k.events


# ---- the oracle and the reference's own code on a case ------------------------------------------------------------------------------------------
def _batch(c):
    from teb_local_planner_amd import _abi
    x, y, th, dt = c["band"]
    b = _abi.TebBatchHost(1, max(len(x), 4))
    b.set_teb(0, x, y, th, dt)
    b.vel_start[0], b.vel_goal[0] = c["vs"], c["vg"]
    return b


def _cfg(c):
    from teb_local_planner_amd.config import TebConfig
    cfg = TebConfig()
    cfg.robot.max_vel_y, cfg.trajectory.dt_ref = c["max_vel_y"], c["dt_ref"]
    return cfg


def others(c, module, is_ref=False):
    """what oracle.oracle_py or oracle.ref_py gives, in the layout of outputs(); None where it cannot run the case. For a plan the reference
    reads the yaw back from a quaternion: the second value is that plan, to run the restatement on, where it differs."""
    op, seen = c["op"], None
    if op == "line":
        b = module.init_trajectory_line(c["start"], c["goal"], c["diststep"], c["max_vel_x"], c["min_samples"], c["back"])
    elif op == "plan":
        b = module.init_trajectory_plan(c["px"], c["py"], c["pyaw"], c["max_vel_x"], c["max_vel_theta"], c["estimate"], c["min_samples"], c["back"])
        if is_ref:
            b, seen = b
    elif op == "path":
        b = module.init_trajectory_path(c["px"], c["py"], c["max_vel_x"], c["max_vel_theta"], c["acc"], c["so"], c["go"], c["min_samples"], c["back"])
    elif op == "prune":
        if len(c["band"][0]) == 0:
            return None, None
        b = module.update_and_prune(*c["band"], c["new_start"], c["new_goal"], c["min_samples"])
    else:
        if len(c["band"][0]) < 2:
            return None, None
        r = module.consumers(_cfg(c), _batch(c), 0, c["look"], c["prevent"])
        return {"status": np.array([0], np.int32), "n": np.array([len(c["band"][0])], np.int32), "cmd": np.append(r["cmd"], float(r["ok"])),
                "profile": r["profile"].ravel(), "traj": r["trajectory"].ravel()}, None
    n = len(b[0])
    if op in ("plan", "path") and len(c["px"]) > c["cap"] + 1:
        return {"status": np.array([2], np.int32), "n": np.array([0], np.int32)}, seen
    if op != "prune" and n > c["cap"]:
        return {"status": np.array([1], np.int32), "n": np.array([0], np.int32)}, seen
    d = {"status": np.array([0], np.int32), "n": np.array([n], np.int32)}
    d.update(zip(BAND, b))
    return d, seen


def disagreement(want, got, is_ref=False):
    """None, or what differs: bit for bit on the exact outputs, ADMISSIBLE on the others (the reference's trajectory headings went through
    a quaternion: 4e-15, modulo 2 pi)"""
    for key, g in got.items():
        w = want[key]
        if w.shape != np.shape(g):
            return "%s: %r against %r entries" % (key, w.shape, np.shape(g))
        ex = want.get("ex_" + key.replace("out_", ""))
        if ex is None:
            if not np.array_equal(w, g):
                return key
            continue
        ex = np.append(ex, True) if key == "cmd" else ex
        tol = np.where(ex, 0.0, ADMISSIBLE)
        if is_ref and key == "traj":
            tol = tol.reshape(-1, 7)
            tol[:, 2] = 4e-15
            tol = tol.ravel()
        diff = np.abs(w - g)
        if is_ref and key == "traj":
            diff.reshape(-1, 7)[:, 2] = np.abs(np.remainder(diff.reshape(-1, 7)[:, 2] + np.pi, 2 * np.pi) - np.pi)
        bad = diff > tol
        if bad.any():
            return "%s[%d]: %r against %r" % (key, int(np.argmax(bad)), w[bad][0], np.asarray(g)[bad][0])
    return None


def check_against(name, c, want, module, is_ref):
    """None, or what the module gives differently on the case"""
    got, seen = others(c, module, is_ref)
    if got is None:
        return None
    if seen is not None and not np.array_equal(seen, c["pyaw"]):   # the plan as the reference saw it: the op-by-op run on that plan
        c2 = dict(c, pyaw=np.array(seen))
        want = dict(want)
        want.update(outputs(SC.evaluate(c2, "float")[0], False)[0])
    return disagreement(want, got, is_ref)


def fleet_extras(stem):
    extra = {}
    for fleet, f in SC.FLEETS.items():
        if group_of(f["members"][0]) != stem:
            continue
        extra["fleet_" + fleet] = np.array(f["members"])
        for key, v in f.items():
            if key != "members":
                extra["fleet_%s_%s" % (fleet, key)] = np.array(v)
    return extra


def main():
    from oracle import oracle_py, ref_py
    ref_py.build()
    oracle_py.build()
    show = sys.argv[1] if len(sys.argv) > 1 else None
    total = np.zeros((len(HS.KINDS), 8))
    for stem, names in groups().items():
        data = {}
        for name in names:
            c, want, rec, _ = reference(name)
            for who, module, is_ref in (("oracle", oracle_py, False), ("reference's code", ref_py, True)):
                if is_ref and not c["ref"]:
                    continue
                diff = check_against(name, c, want, module, is_ref)
                if diff is not None:
                    raise SystemExit("%s: the %s differs from the restatement in %s - nothing written" % (name, who, diff))
            data[name] = dict(inputs(c), **want, summary=HS.summary(rec))
            total[:, :7] += data[name]["summary"][:, :7]
            if show is not None and show in name:
                print("%-60s status %d n %d" % (name, want["status"][0], want["n"][0]), flush=True)
        path = os.path.join(HERE, stem + ".npz")
        np.savez_compressed(path, **HS.pack(data), **fleet_extras(stem))
        size = os.path.getsize(path)
        assert size < MAX_FILE_BYTES, (path, size)
        print("%-30s %3d cases %6d bytes" % (stem + ".npz", len(names), size), flush=True)
    print("%-12s %8s %9s %6s %5s" % ("kind", "all", "SEPARATED", "EXACT", "RUNG"))
    for k, kind in enumerate(HS.KINDS):
        print("%-12s %8d %9d %6d %5d" % (kind, total[k, 0], total[k, 1], total[k, 2], total[k, 3]))


if __name__ == "__main__":
    main()
