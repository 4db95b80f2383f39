"""Writes tests/golden/hp_feasibility_<family>.npz: what the restatement of isTrajectoryFeasible (tests/hp_feasibility.py, fp64 op by op
beside mpmath at 80 digits) gives on every case of tests/feasibility_threshold_cases.py. Run from the repository root:

    python tests/golden/make_hp_feasibility.py [substring of the case names to print; all files are always rewritten]

A case is written only if the reference planner's own function (oracle/_ref through oracle.ref_py.is_trajectory_feasible) and the CPU
oracle give the same (feasible, first_infeasible) for every band; the generator stops otherwise. The fixtures hold data only: per family
one array per field with the cases one after the other (hp_feasibility.pack / unpack; "names" lists them). Per case:
  poses [sum n, 3], band_n [B]   the bands: x, y, theta
  cells (uint8), grid [2]        the costmap: size_x, size_y;  geom [3]: resolution, origin_x, origin_y
  fp [nf, 2]                     the footprint
  params [4]                     inscribed_radius, min_resolution_collision_check_angular, look_ahead_idx, lookahead_distance
  expected [B, 2]                (feasible, first_infeasible) per band; (-9, -9): the call is refused with the capacity error
  summary [kinds, 8]             per kind of comparison (hp_feasibility.KINDS): comparisons, exact ones, ties in fp64, rungs with the fp64
                                 value above / not above the exact one, separated ones true / false, the smallest separated margin
and per fleet of feasibility_threshold_cases.FLEETS "fleet_<name>": its scenes in order, "fleetbands_<name>": the bands of the call.

The two capacity cases of the limits family (2^22 footprint tests: answered; 2^22 + 1: refused) are built here: their expectation is the
oracle's and the reference function's, the restatement does not run four million tests.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import hp_feasibility as HF  # noqa: E402
import feasibility_threshold_cases as FC  # noqa: E402
from teb_local_planner_amd import _abi  # noqa: E402

MAX_FILE_BYTES = 100 * 1000
STEM = "hp_feasibility_"
REFUSED = (-9, -9)
CAPACITY = ("limits_capacity_2^22", "limits_capacity_2^22+1")


def groups():
    out = {}
    for name in list(FC.CASES) + list(CAPACITY):
        out.setdefault(STEM + name.split("_")[0], []).append(name)
    return out


def load(family):
    return HF.unpack(np.load(os.path.join(HERE, STEM + family + ".npz")))


def capacity_case(name):
    """944 poses along x, a point footprint, inscribed_radius 2^-16 and segments of 4447 or 4448 radii: 2^22 tests (or one more) in all,
    the lethal cell under the last pose alone"""
    r, n = 2.0 ** -16, FC.MAX_POSES
    longer = 782 + (1 if name.endswith("+1") else 0)
    m = np.array([4448] * longer + [4447] * (n - 1 - longer), np.float64)
    assert int(m.sum()) - (n - 1) + n == 2 ** 22 + (1 if name.endswith("+1") else 0)
    K = 1027                                                        # the last pose is the lower boundary of column K, alone in it
    x = (-0.5 + K * FC.R - m.sum() * r) + np.concatenate([[0.0], np.cumsum(m)]) * r
    assert x[-1] == -0.5 + K * FC.R and x[0] > -0.5
    cells = FC.zeros(K + 2, 3)
    cells[1, K] = 254
    return dict(bands=[(x, np.full(n, FC.centre(-0.5, 1)), np.zeros(n))], grid=HF.Grid(cells, FC.R, -0.5, -0.5), fp=FC.POINT, r=r, ang=FC.PI,
                look=-1, dist=-1.0, rungs=set())


def batch_of(c):
    bands = c["bands"]
    batch = _abi.TebBatchHost(len(bands), max(max(len(b[0]) for b in bands), 4))
    for k, (x, y, th) in enumerate(bands):
        batch.set_teb(k, x, y, th, np.ones(len(x) - 1))
    return batch


def others(c, module):
    """[(feasible, first_infeasible)] per band of oracle.oracle_py or oracle.ref_py"""
    batch = batch_of(c)
    return [module.is_trajectory_feasible(batch, b, c["grid"], c["fp"], c["r"], c["ang"], c["look"], c["dist"]) for b in range(batch.count)]


def reference(name):
    """(case, expected per band, [n, 6] records of all bands, events); the op-by-op fp64 run alone gives the same answers"""
    c = FC.CASES[name]
    want, recs, events = [], [], None
    for b in range(len(c["bands"])):
        k = HF.Check(c, "both")
        want.append(k.run(b))
        assert want[-1] == HF.Check(c, "float").run(b), name
        recs.append(k.record_array())
        events = k.events if events is None else events + k.events
    return c, want, np.concatenate(recs), events


def record(c, want, rec):
    g = c["grid"]
    return {"poses": np.concatenate([np.stack(b, 1) for b in c["bands"]]), "band_n": np.array([len(b[0]) for b in c["bands"]], np.int32),
            "cells": g.cells, "grid": np.array([g.sx, g.sy], np.int32), "geom": np.array([g.res, g.ox, g.oy]),
            "fp": np.array(c["fp"], np.float64).reshape(-1, 2), "params": np.array([c["r"], c["ang"], c["look"], c["dist"]], np.float64),
            "expected": np.array([(int(ok), first) for ok, first in want], np.int32).reshape(-1, 2),
            "summary": HF.summary(rec) if rec is not None else np.zeros((len(HF.KINDS), 8))}


def main():
    from oracle import oracle_py, ref_py
    ref_py.build()
    oracle_py.build()
    show = sys.argv[1] if len(sys.argv) > 1 else None
    for stem, names in groups().items():
        data, extra, n, exact, ties, rungs, smallest = {}, {}, 0, 0, 0, 0, np.inf
        for name in names:
            if name in CAPACITY:
                c = capacity_case(name)
                want = others(c, oracle_py)
                assert want == others(c, ref_py) and want[0][1] in (2 ** 22 - 1, 2 ** 22), (name, want)
                data[name] = record(c, [REFUSED] if name.endswith("+1") else want, None)
                continue
            c, want, rec, _ = reference(name)
            for who, module in (("reference function", ref_py), ("oracle", oracle_py)):
                got = others(c, module)
                if got != want:
                    raise SystemExit("%s: the %s answers %r, the restatement %r - nothing written" % (name, who, got, want))
            data[name] = record(c, want, rec)
            s = data[name]["summary"]
            n += int(s[:, 0].sum()); exact += int(s[:, 1].sum()); ties += int(s[:, 2].sum()); rungs += int(s[:, 3:5].sum()); smallest = min(smallest, s[:, 7].min())
            if show is not None and show in name:
                print("%-60s %r" % (name, want), flush=True)
        for fleet, (members, bands) in FC.FLEETS.items():
            if STEM + members[0].split("_")[0] == stem:
                extra["fleet_" + fleet] = np.array(members)
                extra["fleetbands_" + fleet] = np.array(bands, np.int32)
        path = os.path.join(HERE, stem + ".npz")
        np.savez_compressed(path, **HF.pack(data), **extra)
        size = os.path.getsize(path)
        assert size < MAX_FILE_BYTES, (path, size)
        print("%-26s %3d cases %6d bytes, %7d comparisons, %6d exact, %5d ties, %4d rungs, smallest separated margin %.3g"
              % (stem + ".npz", len(names), size, n, exact, ties, rungs, smallest), flush=True)


if __name__ == "__main__":
    main()
