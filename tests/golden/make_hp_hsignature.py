"""Writes tests/golden/hp_hsignature_*.npz (one file per case family): what the exact reference of the H-signatures and of the class
decisions (tests/hp_hsignature.py, mpmath at 80 digits) gives on every case of tests/hsignature_cases.py. Run from the repository root:

    python tests/golden/make_hp_hsignature.py [substring of the case names to print; all files are always rewritten]

Per case ("<case>/<key>"; B bands, M obstacles):
  obst [M, 4], n [B], x, y, dt [B, stride]   the inputs
  2-D:  H2 [B, 2, 2]     (re, im) x (hi, lo): the exact value rounded to fp64 and the next 53 bits
        S2 [B, 2]        the scale S as (mantissa, binary exponent): it may lie outside the fp64 range
        absA [B, M, 2]   |A_l| as (mantissa, exponent);  L [B, M, 2]: L_l = sum_i log_value (re, im)
        skip [k, 2]      the obstacle pairs closer than 0.05;  small_map [B]: |end - start| < 3.0
        winners [B, 5]   how often each of the five proposals won;  skipped2 [k, 3]: (band, segment, obstacle) with a pose on the obstacle
  3-D:  H3 [B, M, 2]     (hi, lo), hi = nan where the reference is not finite;  T3 [B, M]: the scale T_l
        skipped3 [k, 2]  (band, segment) below 1e-15;  not_finite [k, 2]: (band, obstacle)
  cls<mode> [lists, 3, B]   keep / valid / reasonable per class list of the case (threshold, best, plans per class)
  margins<mode> [5]      comparisons recorded, exact ones, ties among them, the smallest relative margin of the separated ones, the
                         smallest margin of a class decision in units of the error it is allowed
  oracle_err<mode> [B]   the CPU oracle's error on the band in the units of hp_hsignature (3-D: the largest over the obstacles)
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import hp_hsignature as HS  # noqa: E402
import hsignature_cases as HC  # noqa: E402

MAX_FILE_BYTES = 500 * 1000   # the cap of the association fixtures (make_hp_association.MAX_FILE_BYTES)


def group_of(name):
    return "hp_hsignature_" + name.split("_")[0]


def groups():
    out = {}
    for name in HC.CASES:
        out.setdefault(group_of(name), []).append(name)
    return out


def load(name):
    return np.load(os.path.join(HERE, group_of(name) + ".npz"))


def reference(name, mutate=None, band=None, modes=None):
    """(case, {mode: dict(rec: Recorder, bands: [signature_2d / signature_3d result per band], cls: [(keep, valid, reas) per class list])})
    mutate / band: the mutation (hp_hsignature) applied to that one band; no class lists then"""
    c = HC.build(name)
    ob = np.array(c["obst"], np.float64).reshape(-1, 4)
    out = {}
    for mode in (c["modes"] if modes is None else modes):
        rec = HS.Recorder()
        res = []
        for b, (x, y, dt) in enumerate(c["bands"]):
            if band is not None and b != band:
                res.append(None)
                continue
            mu = mutate if b == band else None
            if mode == 2:
                res.append(HS.signature_2d(ob[:, 0], ob[:, 1], x, y, c["prescaler"], rec, b, mu))
            else:
                res.append(HS.signature_3d(ob[:, 0], ob[:, 1], ob[:, 2], ob[:, 3], x, y, dt, rec, b, mu))
        cls = []
        if mutate is None and band is None:
            for k, (thr, best, plans) in enumerate(c["class_lists"]):
                if mode == 2:
                    cls.append(HS.class_decisions(2, [r["H"] for r in res], [r["S"] for r in res], thr, best, plans, rec, "%s list %d" % (name, k)))
                else:
                    cls.append(HS.class_decisions(3, [r["H"] for r in res], [r["T"] for r in res], thr, best, plans, rec, "%s list %d" % (name, k)))
        out[mode] = dict(rec=rec, bands=res, cls=cls)
    return c, out


def exact_arrays(mode, res, M):
    """the arrays of error_2d / error_3d for one band's reference result"""
    if mode == 2:
        return np.array([HS.split(res["H"].real), HS.split(res["H"].imag)]), np.array(HS.mant_exp(res["S"]))
    return np.array([HS.split(v) for v in res["H"]], np.float64).reshape(M, 2), np.array([float(v) for v in res["T"]], np.float64)


def oracle_errors(c, mode, R, oracle):
    """the CPU oracle's error per band, in the units of hp_hsignature (and whether its finite pattern is the reference's)"""
    want = oracle.h_signatures(HC.config(mode), c["table"], c["batch"], mode, c["prescaler"])
    errs, same = [], True
    for b, res in enumerate(R[mode]["bands"]):
        ex, sc = exact_arrays(mode, res, len(c["obst"]))
        if mode == 2:
            errs.append(HS.error_2d(want[b], ex, sc))
        else:
            e, s = HS.error_3d(want[b], ex, sc)
            errs.append(e); same = same and s
    return np.array(errs), same, want


def reference_record(name, oracle, ref=None):
    c, R = reference(name) if ref is None else ref
    k = name + "/"
    M, B = len(c["obst"]), len(c["bands"])
    bt = c["batch"]
    rec = {k + "obst": np.array(c["obst"], np.float64).reshape(-1, 4), k + "n": bt.n.copy(), k + "x": bt.x.copy(), k + "y": bt.y.copy(), k + "dt": bt.dt.copy()}
    for mode, r in R.items():
        m = str(mode)
        cm = [q[2] for q in r["rec"].records if q[0].startswith("class ")]
        rec[k + "margins" + m] = np.array(list(r["rec"].summary(("2d", "3d")[mode - 2])) + [min(cm) if cm else np.inf], np.float64)
        if r["cls"]:
            rec[k + "cls" + m] = np.array([[q for q in kvr] for kvr in r["cls"]], np.int32)
        if mode == 2:
            rec[k + "H2"] = np.array([exact_arrays(2, q, M)[0] for q in r["bands"]]).reshape(B, 2, 2)
            rec[k + "S2"] = np.array([HS.mant_exp(q["S"]) for q in r["bands"]], np.float64).reshape(B, 2)
            rec[k + "absA"] = np.array([[HS.mant_exp(v) for v in q["absA"]] for q in r["bands"]], np.float64).reshape(B, M, 2)
            rec[k + "L"] = np.array([[(float(v.real), float(v.imag)) for v in q["L"]] for q in r["bands"]], np.float64).reshape(B, M, 2)
            rec[k + "skip"] = np.array(r["bands"][0]["skipped_pairs"], np.int32).reshape(-1, 2)
            rec[k + "small_map"] = np.array([-1 if q["small_map"] is None else int(q["small_map"]) for q in r["bands"]], np.int32)
            rec[k + "winners"] = np.array([np.bincount(list(q["selections"].values()), minlength=5) for q in r["bands"]], np.int64).reshape(B, 5)
            rec[k + "skipped2"] = np.array([(b, i, l) for b, q in enumerate(r["bands"]) for i, l in q["skipped_segments"]], np.int32).reshape(-1, 3)
        else:
            rec[k + "H3"] = np.array([exact_arrays(3, q, M)[0] for q in r["bands"]], np.float64).reshape(B, M, 2)
            rec[k + "T3"] = np.array([exact_arrays(3, q, M)[1] for q in r["bands"]], np.float64).reshape(B, M)
            rec[k + "skipped3"] = np.array([(b, i) for b, q in enumerate(r["bands"]) for i in q["skipped"]], np.int32).reshape(-1, 2)
            rec[k + "not_finite"] = np.array([(b, l) for b, q in enumerate(r["bands"]) for l in sorted(q["not_finite"])], np.int32).reshape(-1, 2)
        rec[k + "oracle_err" + m] = oracle_errors(c, mode, R, oracle)[0]
    return c, rec


def main():
    from oracle import oracle_py
    oracle_py.build()
    show = sys.argv[1] if len(sys.argv) > 1 else None
    for stem, names in groups().items():
        data, worst, smallest, cls_margin = {}, {2: 0.0, 3: 0.0}, np.inf, np.inf
        for name in names:
            c, rec = reference_record(name, oracle_py)
            data.update(rec)
            for mode in c["modes"]:
                m = rec[name + "/margins%d" % mode]
                smallest, cls_margin = min(smallest, m[3]), min(cls_margin, m[4])
                worst[mode] = max(worst[mode], rec[name + "/oracle_err%d" % mode].max(initial=0.0))
                if show is not None and show in name:
                    print("%-28s mode %d: comparisons %7d exact %4d ties %4d smallest margin %.3g, class margin %.3g x allowed, oracle error %s" %
                          (name, mode, m[0], m[1], m[2], m[3], m[4], np.array2string(rec[name + "/oracle_err%d" % mode], precision=1)), flush=True)
        path = os.path.join(HERE, stem + ".npz")
        np.savez_compressed(path, **data)
        size = os.path.getsize(path)
        assert size < MAX_FILE_BYTES, (path, size)
        print("%-28s %3d cases %7d bytes, smallest separated margin %.3g, smallest class margin %.3g x allowed, oracle error 2-D %.1f 3-D %.1f" %
              (stem + ".npz", len(names), size, smallest, cls_margin, worst[2], worst[3]), flush=True)


if __name__ == "__main__":
    main()
