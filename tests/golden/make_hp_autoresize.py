"""Writes tests/golden/hp_autoresize_*.npz (one file per case family; the `sizes` family one per layout group, its band-in-HBM sizes one per T): what the plain
restatement of TimedElasticBand::autoResize with 80-digit headings (tests/hp_autoresize.py) gives on every case of
tests/autoresize_cases.py. Run from the repository root:

    python tests/golden/make_hp_autoresize.py [substring of the case names to print; all files are always rewritten]

Per case ("<case>/<key>"):
  hash                     sha256 of the inputs of every member and of the case's parameters (hp_autoresize.input_hash)
and per member j of the case (one; the batch case: eight) under "<case>/m<j>/":
  bands                    number of stored bands: fast mode one per call that was not stopped by the capacity, full mode 1 (the final band)
  stopped                  1: the next sweep would leave more poses than the handle holds - the band stays as it is
  b<k>/dt, x, y            the expected band after call k: EXACT (bit equality)
  b<k>/th_hi, th_lo        the 80-digit heading of every pose rounded to two doubles (input poses: the input heading, 0)
  b<k>/err_ref             the fp64 restatement's own heading error per pose against the 80-digit value (rad; 0 for input poses)
  b<k>/new                 pose was created by a split (in this or an earlier sweep)
  records [sweeps,5,4,4]   the comparisons of every sweep: threshold x provenance of the operand x relation (hp_autoresize.THR_*, P_*, R_*)
  classes [sweeps,2]       autoresize_cases.sweep_class of every sweep (which machine the sweep belongs to), longest member chain
  modified [sweeps]        the reference's `modified` flag after the sweep
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import hp_autoresize as HA  # noqa: E402
import autoresize_cases as AC  # noqa: E402

MAX_FILE_BYTES = 500 * 1000   # as the other pins
BAND_KEYS = ("dt", "x", "y", "th_hi", "th_lo", "err_ref", "new")
_OPEN = {}


def groups():
    out = {}
    for name in AC.CASES:
        out.setdefault(AC.group_of(name), []).append(name)
    return out


def load(name):
    g = AC.group_of(name)
    if g not in _OPEN:
        _OPEN[g] = np.load(os.path.join(HERE, g + ".npz"))
    return _OPEN[g]


def case_hash(c):
    arrays = [np.concatenate([m[k] for m in c["members"]]) for k in ("x", "y", "theta", "dt")]
    return HA.input_hash(*arrays, params=AC.params_of(c) + tuple(len(m["x"]) for m in c["members"]))


def reference_record(name, case=None):
    """(case, dict of the fixture's entries for it)"""
    c = AC.build(name) if case is None else case
    rec = {name + "/hash": np.array(case_hash(c))}
    for j, m in enumerate(c["members"]):
        r = AC.reference(c, j)
        k = "%s/m%d/" % (name, j)
        bands = r["sweeps"] if c["fast"] else [r["final"]]
        rec[k + "bands"] = np.int32(len(bands))
        rec[k + "stopped"] = np.int32(r["stopped"])
        for q, b in enumerate(bands):
            for key in BAND_KEYS:
                rec["%sb%d/%s" % (k, q, key)] = b[key]
        ins = [m["dt"]] + [b["dt"] for b in r["sweeps"]]
        ns = len(r["sweeps"])
        rec[k + "records"] = np.array(r["records"], np.int32).reshape(ns, 5, 4, 4)
        rec[k + "classes"] = np.array([AC.sweep_class(ins[q], c, r["fired"][q]) for q in range(ns)], np.int32).reshape(ns, 2)
        rec[k + "modified"] = np.array(r["modified"], np.int32)
        rec[k + "conditioning"] = np.float64(r["conditioning"])
    return c, rec


def expected(fx, c, member, call):
    """(band the device must hold after call `call` (0-based) of the case on member `member`, overflow expected in that call)"""
    k = "%s/m%d/" % (c["name"], member)
    nb, stopped = int(fx[k + "bands"]), bool(fx[k + "stopped"])
    q = min(call, nb - 1)
    if q < 0:   # stopped before the first sweep: the band as uploaded
        m = c["members"][member]
        n = len(m["x"])
        band = dict(n=n, x=m["x"], y=m["y"], dt=m["dt"], th_hi=m["theta"], th_lo=np.zeros(n), err_ref=np.zeros(n), new=np.zeros(n, bool))
    else:
        band = {key: fx["%sb%d/%s" % (k, q, key)] for key in BAND_KEYS}
        band["n"] = len(band["x"])
    return band, stopped and call >= nb


def main():
    show = sys.argv[1] if len(sys.argv) > 1 else None
    for stem, names in groups().items():
        data, worst, cond = {}, 0.0, np.inf
        for name in names:
            c, rec = reference_record(name)
            data.update(rec)
            errs = [float(v.max()) for key, v in rec.items() if key.endswith("/err_ref") and len(v)]
            worst = max([worst] + errs)
            cond = min([cond] + [float(v) for key, v in rec.items() if key.endswith("/conditioning")])
            if show is not None and show in name:
                print("%-34s n %s classes %s" % (name, [len(rec[key]) for key in rec if key.endswith("/x")],
                                                [rec[key][:, 0].tolist() for key in rec if key.endswith("/classes")]), flush=True)
        path = os.path.join(HERE, stem + ".npz")
        np.savez_compressed(path, **data)
        size = os.path.getsize(path)
        assert size < MAX_FILE_BYTES, (path, size)
        print("%-32s %3d cases %7d bytes, restatement's heading error <= %.1f eps, smallest |e^ia + e^ib| %.2f" %
              (stem + ".npz", len(names), size, worst / HA.EPS, cond), flush=True)


if __name__ == "__main__":
    main()
