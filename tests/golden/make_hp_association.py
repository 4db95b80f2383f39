"""Writes tests/golden/hp_association_*.npz (one file per case family): what the exact reference of the graph build's decisions
(tests/hp_association.py, mpmath at 80 digits) gives on every case of tests/association_cases.py. Run from the repository root:

    python tests/golden/make_hp_association.py [substring of the case names to print; all files are always rewritten]

Per case ("<case>/<key>"):
  assoc_pose, assoc_obst   the obstacle edges in the order of oracle.associate / debug_linearize (the legacy cases: obstacle-major, the
                           GPU test compares them as a sorted multiset - hp_association.canonical)
  via_pose                 the pose of every via-point, -1: no edge
  scene                    sha256 of the inputs (hp_linearize.input_hash)
  margins [4]              comparisons recorded, exact ones, ties among them, the smallest relative margin of the well separated ones
and for the cases with `hcheck` the high-precision linearisation at weight multiplier 1, as in tests/golden/make_hp_linearize.py:
  Hband, b, chi2, rows, margin, oracle_err
and, where the case also runs in the numeric Jacobian mode, Hband_numeric, b_numeric, oracle_err_numeric: the central-difference
quotient at delta = 1e-9 (g2o's) evaluated at 80 digits, and the CPU oracle's numeric mode against it
(the edges whose penalty argument sits on its threshold by construction are exempted from the branch-margin check under the
conditions of hp_linearize._check_exempt).
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import hp_linearize as hp  # noqa: E402
import hp_association as HA  # noqa: E402
import association_cases as AC  # noqa: E402
from teb_local_planner_amd import _abi  # noqa: E402

MAX_FILE_BYTES = 500 * 1000


def groups():
    out = {}
    for name in AC.CASES:
        out.setdefault("hp_association_" + name.split("_")[0], []).append(name)
    return out


def group_of(name):
    return "hp_association_" + name.split("_")[0]


def load(name):
    return np.load(os.path.join(HERE, group_of(name) + ".npz"))


def exempt_pairs(c, irec):
    """the (index into irec, argument name) pairs of the case's exemptions (edge type, pose, obstacle, argument name)"""
    at = {(int(r[0]), int(r[2]), int(r[9])): e for e, r in enumerate(irec)}
    return {(at[(ty, pose, ob)], name) for ty, pose, ob, name in c["exempt"]}


def reference(name, case=None):
    """(case, Reference, dict(assoc_pose, assoc_obst, via_pose, + what associate() / legacy() record))"""
    c = AC.build(name) if case is None else case
    R = HA.Reference(c["cfg"], c["obst"], c["via"], c["batch"])
    if c["legacy"]:
        ap, ao, closest = R.legacy()
        A = dict(assoc_pose=ap, assoc_obst=ao, closest=closest)
    else:
        A = R.associate()
    A["via_pose"] = R.via_points() if c["via"] and float(c["cfg"].optim.weight_viapoint) != 0 else np.zeros(0, np.int32)
    return c, R, A


def reference_record(name, oracle, ref=None):
    c, R, A = reference(name) if ref is None else ref
    cfg, obst, via, batch = c["cfg"], c["obst"], c["via"], c["batch"]
    cfg.jacobian_mode = _abi.JACOBIAN_ANALYTIC
    k = name + "/"
    rec = {k + "assoc_pose": A["assoc_pose"], k + "assoc_obst": A["assoc_obst"], k + "via_pose": A["via_pose"],
           k + "scene": np.array(hp.input_hash(cfg, obst, via, batch, 0)), k + "margins": np.array(R.summary(), np.float64)}
    if c["hcheck"]:
        ir, _ = oracle.edges(cfg, obst, via, batch, 0, 1.0)
        L = hp.linearize(cfg, obst, via, batch, 0, 1.0, ir, exempt=exempt_pairs(c, ir))
        Hb, bv, chi2 = hp.to_band(L)
        G = oracle.linearize(cfg, obst, via, batch, 0, 1.0)
        eH, eb = hp.errors(hp.band_of_dense(G["H"]), G["b"], Hb, bv, chi2)
        rec[k + "Hband"], rec[k + "b"], rec[k + "chi2"] = Hb, bv, chi2
        rec[k + "rows"] = np.array([[t, r] + st for (t, r), st in sorted(L["rows"].items())], np.int64).reshape(-1, 6)
        rec[k + "margin"] = np.float64(L["margin"])
        rec[k + "oracle_err"] = np.array([eH, eb])
        if c["numeric"]:   # the numeric Jacobian mode: g2o's central differences at delta = 1e-9, the same quotient at 80 digits
            L = hp.linearize(cfg, obst, via, batch, 0, 1.0, ir, kink_delta="1e-9", exempt=exempt_pairs(c, ir))
            Hn, bn, chi2n = hp.to_band(L)
            assert np.array_equal(chi2n, chi2)
            cfg.jacobian_mode = _abi.JACOBIAN_G2O_NUMERIC
            G = oracle.linearize(cfg, obst, via, batch, 0, 1.0)
            cfg.jacobian_mode = _abi.JACOBIAN_ANALYTIC
            rec[k + "Hband_numeric"], rec[k + "b_numeric"] = Hn, bn
            rec[k + "oracle_err_numeric"] = np.array(hp.errors(hp.band_of_dense(G["H"]), G["b"], Hn, bn, chi2))
    return c, rec


def main():
    from oracle import oracle_py
    oracle_py.build()
    show = sys.argv[1] if len(sys.argv) > 1 else None
    eps = np.finfo(float).eps
    for stem, names in groups().items():
        data, worst, smallest = {}, np.zeros(2), np.inf
        for name in names:
            c, rec = reference_record(name, oracle_py)
            data.update(rec)
            m = rec[name + "/margins"]
            smallest = min(smallest, m[3])
            if c["hcheck"]:
                worst = np.maximum(worst, rec[name + "/oracle_err"])
            if show is not None and show in name:
                print("%-44s comparisons %6d exact %3d ties %3d smallest margin %.3g" % (name, m[0], m[1], m[2], m[3]), flush=True)
        path = os.path.join(HERE, stem + ".npz")
        np.savez_compressed(path, **data)
        size = os.path.getsize(path)
        assert size < MAX_FILE_BYTES, (path, size)
        print("%-32s %3d cases %7d bytes, smallest separated margin %.3g, oracle error H %.1f b %.1f eps" %
              (stem + ".npz", len(names), size, smallest, worst[0] / eps, worst[1] / eps), flush=True)


if __name__ == "__main__":
    main()
