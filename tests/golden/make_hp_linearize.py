"""Writes tests/golden/hp_linearize_*.npz: the high-precision reference linearisation (tests/hp_linearize.py, mpmath at 80 digits) of
every case of tests/hp_linearize_cases.py, rounded to float64. Run from the repository root:

    python tests/golden/make_hp_linearize.py [substring of the case names to print; all files are always rewritten]

Per case and weight multiplier with a fixture of its own ("<case>/wm<multiplier>/<key>"):
  Hband [4n][11]   lower band of H, column d = H[a, a - d] (the generator asserts that nothing lies outside it)
  b [4n], chi2 [4] per category {obstacle-type, via-point, time-optimal, other}
  rows [k][6]      (edge type, row, rows, non-zero rows, rows on the + side, rows on the - side) of every row kind
  ring [2]         inflated obstacle edges in the inflation ring only / inside min_obstacle_dist
  margin           the smallest branch margin (the reference raises below 1e-7)
  oracle_err [2]   H and b error of the CPU oracle's closed forms against this reference in the metric of hp_linearize.errors: the fp64
                   noise floor of the same closed forms the device evaluates; the GPU test's bound is max(256 eps, 16 x this)
  scene, edges     sha256 of the inputs (hp_linearize.input_hash / edges_hash)
and per case "<case>/state" [4][n]: x, y, theta, dt of the band (what the cases next to a kink were moved to).
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import hp_linearize as hp  # noqa: E402
import hp_linearize_cases as HC  # noqa: E402
from teb_local_planner_amd import _abi  # noqa: E402

MAX_FILE_BYTES = 500 * 1000
PER_FILE = 16


def groups():
    """{file stem: [case names]}: a long case has a file of its own, the others share files of PER_FILE cases"""
    out, count = {}, {"short": 0, "near": 0}
    for name in HC.CASES:
        if name.startswith("long_"):
            out["hp_linearize_" + name] = [name]
            continue
        kind = "near" if HC.is_near(name) else "short"
        out.setdefault("hp_linearize_%s_%d" % (kind, count[kind] // PER_FILE), []).append(name)
        count[kind] += 1
    return out


def group_of(name):
    for stem, names in groups().items():
        if name in names:
            return stem
    raise KeyError(name)


def edges_of(oracle):
    return lambda c: oracle.edges(c["cfg"], c["obst"], c["via"], c["batch"], 0, 1.0)[0]


def reference_record(name, oracle, case=None):
    """(case, {key: array}) - the reference of one case, recomputed"""
    c = HC.build(name, edges_of=edges_of(oracle)) if case is None else case
    cfg, obst, via, batch = c["cfg"], c["obst"], c["via"], c["batch"]
    cfg.jacobian_mode = _abi.JACOBIAN_ANALYTIC
    rec = {name + "/state": np.stack([np.append(a, 0.0) if len(a) < int(batch.n[0]) else a for a in batch.get_teb(0)])}
    for wm in c["wms"]:
        ir, _ = oracle.edges(cfg, obst, via, batch, 0, wm)
        R = hp.linearize(cfg, obst, via, batch, 0, wm, ir, c["kink_delta"])
        Hb, bv, chi2 = hp.to_band(R)
        A = oracle.linearize(cfg, obst, via, batch, 0, wm)
        eH, eb = hp.errors(hp.band_of_dense(A["H"]), A["b"], Hb, bv, chi2)
        k = "%s/wm%g/" % (name, wm)
        rec[k + "Hband"], rec[k + "b"], rec[k + "chi2"] = Hb, bv, chi2
        rec[k + "rows"] = np.array([[t, r] + st for (t, r), st in sorted(R["rows"].items())], np.int64).reshape(-1, 6)
        rec[k + "ring"] = np.array([R["ring_only"], R["inside"]], np.int64)
        rec[k + "margin"] = np.float64(R["margin"])
        rec[k + "oracle_err"] = np.array([eH, eb])
        rec[k + "scene"] = np.array(hp.input_hash(cfg, obst, via, batch, 0))
        rec[k + "edges"] = np.array(hp.edges_hash(ir))
    return c, rec


def load(name):
    return np.load(os.path.join(HERE, group_of(name) + ".npz"))


def main():
    from oracle import oracle_py
    oracle_py.build()
    show = sys.argv[1] if len(sys.argv) > 1 else None
    worst = {}
    for stem, names in groups().items():
        data = {}
        for name in names:
            c, rec = reference_record(name, oracle_py)
            data.update(rec)
            for wm in c["wms"]:
                e = rec["%s/wm%g/oracle_err" % (name, wm)]
                fam = name.split("_")[0] if not name.startswith(("near", "long")) else "_".join(name.split("_")[:2])
                worst[fam] = np.maximum(worst.get(fam, np.zeros(2)), e)
                if show is not None and show in name:
                    print("%-60s wm %g  oracle error H %.2e b %.2e  margin %.2e" % (name, wm, e[0], e[1], rec["%s/wm%g/margin" % (name, wm)]))
        path = os.path.join(HERE, stem + ".npz")
        np.savez_compressed(path, **data)
        size = os.path.getsize(path)
        assert size < MAX_FILE_BYTES, (path, size)
        print("%-50s %3d cases %7d bytes" % (stem + ".npz", len(names), size), flush=True)
    print("largest error of the CPU oracle's closed forms per family (H, b), in units of eps:")
    for fam, e in sorted(worst.items()):
        print("  %-28s %8.1f %8.1f" % (fam, e[0] / np.finfo(float).eps, e[1] / np.finfo(float).eps))


if __name__ == "__main__":
    main()
