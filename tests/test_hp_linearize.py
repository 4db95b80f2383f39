"""Every cost term's closed-form linearisation against a high-precision reference of its residual (CPU side).

tests/hp_linearize.py restates the residual of every edge class over mpmath at 80 digits and differentiates it by central differences at
delta = 1e-30: the true derivative to ~ 1e-50, with no Jacobian formula of its own. tests/hp_linearize_cases.py isolates one cost-term
family per case (every other weight 0) on states where its penalties are active on both sides, next to every kink (+-1e-6), and on long
bands. For every case this file
  - recomputes the reference and compares it with the fixture under tests/golden/ EXACTLY (a stale fixture fails), checks the hashes of
    the scene and of the edge list;
  - asserts the activation conditions from the reference alone: each row kind of the family non-zero on >= 25 % of its rows, each
    two-sided penalty active on each side on >= 2 rows, obstacle rows inside min_obstacle_dist and in the inflation ring only, the
    argument of a near-kink case 1e-6 from its switch point on the named side; the smallest branch margin >= 1e-7 (the reference
    raises below it);
  - compares oracle.linearize in ANALYTIC mode with the reference: H and b error <= 256 eps = 5.7e-14 in the floored local metric of
    hp_linearize.errors (at most ~ 60 rows summed into an entry + ~ 20 roundings in each Jacobian factor ~ 100 eps, times 2.5),
    chi^2 per category relative <= (rows + 16) eps. The scale is local to a variable kind within ONE family, so a light term cannot
    hide behind the weight-1000 kinematics edge as it does in tests/test_oracle_jacobians.py (2e-6 of max|H| over the whole graph).

Found with it: the slope of the exact-arc-length factor, (sin h - h cos h) / (2 sin^2 h), was evaluated as the difference it is written
as and lost 3 / h^2 of its digits - 1.4e-12 (6500 eps) in velocity_exact_arc; summed from its series it is at 3 eps (csrc/teb_edges.hpp
and oracle/teb_oracle.cpp: arc_factor_slope).

Largest observed error of the oracle's closed forms per family, in eps (H / b): velocity 2.8 / 2.3, holonomic velocity 1.4 / 0.6,
acceleration 3.1 / 1.2, diff-drive 23 / 3.8, car-like 2.1 / 1.2 (documented kink 1.8 / 0.6), time-optimal 0 / 0, shortest path
1.3 / 0.2, prefer-rotdir 0 / 0.5, via-points 1.5 / 0, static obstacles by footprint: point 8.6 / 2.5, circular 24 / 2.0, two circles
25 / 2.1, line 194 / 13, polygon 215 / 53; dynamic obstacles 56 / 3.4, velocity-obstacle ratio 3.0 / 1.1, legacy association
4.6 / 1.6, next to a kink 215 / 21 (the polygon-footprint case; 23 / 3.8 otherwise), long bands 25 / 1.5. Bound: 256.
Measured run time of this file: 66 s on one core (the three 600-pose bands and the polygon footprints are most of it).
"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import hp_linearize as hp  # noqa: E402
import hp_linearize_cases as HC  # noqa: E402
import make_hp_linearize as MK  # noqa: E402

from teb_local_planner_amd import _abi  # noqa: E402

EPS = np.finfo(np.float64).eps
BOUND = 256 * EPS


def check_chi2(chi2, chi2_ref, rows):
    """relative (rows + 16) eps per category; a category without residual is exactly 0"""
    per_cat = np.zeros(4)
    for t, r, count, nonzero, pos, neg in rows:
        per_cat[hp._CATEGORY.get(int(t), hp.CAT_OTHER)] += count
    for k in range(4):
        if chi2_ref[k] == 0:
            assert chi2[k] == 0
        else:
            rel = abs(chi2[k] - chi2_ref[k]) / chi2_ref[k]
            assert rel <= (per_cat[k] + 16) * EPS, (k, rel / EPS, per_cat[k])


def test_the_case_table_covers_every_family_and_layout():
    names = set(HC.CASES)
    kinds = set()
    for name in names:
        fx = MK.load(name)
        for key in fx.files:
            if key.startswith(name + "/") and key.endswith("/rows"):
                kinds |= {int(t) for t, r, count, nonzero, pos, neg in fx[key] if nonzero > 0}
    assert kinds == set(range(18)), "edge types without an active row in any case: %s" % sorted(set(range(18)) - kinds)
    for layout in ("band", "cr", "bandg"):
        assert sum(n.startswith("long_%s_" % layout) for n in names) == 5
    every = sorted(n for names_ in MK.groups().values() for n in names_)
    assert every == sorted(names)
    have = sorted(f for f in os.listdir(os.path.join(HERE, "golden")) if f.startswith("hp_linearize_") and f.endswith(".npz"))
    assert have == sorted(stem + ".npz" for stem in MK.groups())
    for f in have:
        assert os.path.getsize(os.path.join(HERE, "golden", f)) < MK.MAX_FILE_BYTES


@pytest.mark.parametrize("name", list(HC.CASES))
def test_oracle_closed_forms_against_the_reference(oracle, name):
    fx = MK.load(name)
    c, rec = MK.reference_record(name, oracle)
    # the fixture is what the reference gives today, bit for bit (the oracle's own error aside: it is compared below, not pinned)
    keys = sorted(k for k in fx.files if k.startswith(name + "/"))
    assert keys == sorted(rec)
    for k in keys:
        if not k.endswith("/oracle_err"):
            assert np.array_equal(fx[k], rec[k]), k
    cfg, obst, via, batch = c["cfg"], c["obst"], c["via"], c["batch"]
    for wm in c["wms"]:
        p = "%s/wm%g/" % (name, wm)
        rows = {(int(t), int(r)): (int(count), int(nonzero), int(pos), int(neg)) for t, r, count, nonzero, pos, neg in rec[p + "rows"]}
        # ---- activation and margins, from the reference alone
        assert rec[p + "margin"] >= hp.MARGIN
        for kind in c["active"]:
            count, nonzero, pos, neg = rows[kind]
            assert count > 0 and 4 * nonzero >= count, (kind, rows[kind])
        for kind in c["two_sided"]:
            count, nonzero, pos, neg = rows[kind]
            assert pos >= 2 and neg >= 2, (kind, rows[kind])
        if c["ring"]:
            assert rec[p + "ring"][0] >= 2 and rec[p + "ring"][1] >= 2, rec[p + "ring"]
        for kind in c["silent"]:
            assert rows[kind][0] > 0 and rows[kind][1] == 0, (kind, rows[kind])
        if 2.0 not in c["wms"]:   # one fixture serves both multipliers: no row that carries the multiplier may be alive
            for kind in ((hp.E_OBST, 0), (hp.E_INFL, 0)):
                assert rows.get(kind, (0, 0))[1] == 0
        if c["near"] is not None:
            spec, side, key = c["near"]
            gap = HC.near_gap(c, MK.edges_of(oracle), spec, key)[0]
            assert abs(gap - side * HC.NEAR_OFFSET) <= 1e-3 * HC.NEAR_OFFSET, gap
        # ---- the oracle's closed forms
        cfg.jacobian_mode = _abi.JACOBIAN_ANALYTIC
        A = oracle.linearize(cfg, obst, via, batch, 0, wm)
        eH, eb = hp.errors(hp.band_of_dense(A["H"]), A["b"], rec[p + "Hband"], rec[p + "b"], rec[p + "chi2"])
        print("%s wm %g: H error %.1f eps, b error %.1f eps" % (name, wm, eH / EPS, eb / EPS))
        assert eH <= BOUND and eb <= BOUND, (eH / EPS, eb / EPS)
        assert (fx[p + "oracle_err"] <= BOUND).all()
        check_chi2(A["chi2"], rec[p + "chi2"], rec[p + "rows"])
    if 2.0 not in c["wms"]:
        A = oracle.linearize(cfg, obst, via, batch, 0, 2.0)
        p = name + "/wm1/"
        eH, eb = hp.errors(hp.band_of_dense(A["H"]), A["b"], rec[p + "Hband"], rec[p + "b"], rec[p + "chi2"])
        assert eH <= BOUND and eb <= BOUND, (eH / EPS, eb / EPS)
