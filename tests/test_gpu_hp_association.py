"""The device's decisions of the graph build - which pose carries which obstacle / via-point edge - against the exact reference
(tests/test_hp_association.py is the CPU side and describes the reference, the admissibility condition and the case families).

For every case of tests/association_cases.py: planner.make_solver(...).debug_linearize(0, n, wm) with wm in {1, 2}, in the host's own
layout pick and in every pinned layout the pose count admits, in the numeric Jacobian mode as well where the case says so;
assoc_pose / assoc_obst must EQUAL the fixture under tests/golden/ (no mpmath and no oracle needed here; the legacy lists as a sorted
multiset per pose), debug_overflow_flags() must be clear and last_instantiation() must name the layout, the Jacobian mode and the
distance path (point-like against generic) the case was built for. Where the decisions show in H - the static threshold ladder, the
far-field culling of the dynamic obstacles, the via-point attachment - H, b and chi^2 of the analytic mode are compared with the
80-digit linearisation under the metric and bound of tests/test_gpu_hp_linearize.py, max(256 eps, 16 x the CPU oracle's error on the
case): an edge culled inside its threshold, or a via-point attached to the later of two equidistant poses, is a wrong entry of the
size of the weight. In the numeric mode (its culling radius is 1e-6 wider) H and b are compared with the central-difference quotient
at delta = 1e-9 evaluated at 80 digits, under association_cases.numeric_bound (the fp64 noise of such a quotient, 1e-4 .. 1e-3; an
edge culled next to its threshold is an error of the order of 1). No case and no entry is skipped.

The tie, forced-cluster and generic-shape cases also run one optimize(1, 1) of their single band on the generic distance path with the
multi-CU mode off and with helper workgroups (the SHARED instantiation of associate_range: always sliced, forced lists staged in LDS):
bands, chi^2, lambda and trial counts must be bit-identical. One band per launch.

Found with it on an MI355X: nothing - in every case, layout and Jacobian mode the device's lists equal the reference's, also with helper
workgroups. Largest device error on the H cases over every layout, in eps (H / b, bound 256): ladder 1.8 / 0.1, dynamic culling
0.8 / 0.6, via-points 1.0 / 0; numeric mode against the central differences at 80 digits: ladder 7.4e-6 (bound 7.7e-4), dynamic culling
4.5e-7 (bound 1.1e-4 .. 1.1e-3). The whole file (106 tests) takes 3.1 s; the slowest case 0.23 s.
"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import hp_linearize as hp  # noqa: E402
import hp_association as HA  # noqa: E402
import association_cases as AC  # noqa: E402
import make_hp_association as MK  # noqa: E402
from hp_linearize_cases import LAYOUT_INDEX  # noqa: E402
from test_hp_linearize import check_chi2, BOUND, EPS  # noqa: E402

from teb_local_planner_amd import planner, _abi  # noqa: E402

pytestmark = pytest.mark.gpu


def test_the_build_has_the_geometry_the_cases_assume():
    assert planner.TebBatchSolver.build_info()[3] == AC.K_THREADS   # lanes per workgroup: which poses get several lanes


@pytest.mark.parametrize("name", list(AC.CASES))
def test_device_decisions_against_the_reference(name):
    fx = MK.load(name)
    c = AC.build(name)
    cfg, obst, via, batch = c["cfg"], c["obst"], c["via"], c["batch"]
    n = int(batch.n[0])
    p = name + "/"
    cfg.jacobian_mode = _abi.JACOBIAN_ANALYTIC
    assert str(fx[p + "scene"]) == hp.input_hash(cfg, obst, via, batch, 0)
    want_pose, want_obst = fx[p + "assoc_pose"], fx[p + "assoc_obst"]
    for mode in (_abi.JACOBIAN_ANALYTIC, _abi.JACOBIAN_G2O_NUMERIC) if c["numeric"] else (_abi.JACOBIAN_ANALYTIC,):
        cfg.jacobian_mode = mode
        for layout in c["layouts"]:
            s = planner.make_solver(cfg, obst, via, batch, options=None if layout == "auto" else _abi.Options(layout=layout))
            try:
                for wm in (1.0, 2.0):
                    G = s.debug_linearize(0, n, wm)
                    ran = s.last_instantiation()
                    assert ran[1] == mode, ran
                    assert ran[0] == LAYOUT_INDEX[AC.auto_layout(n) if layout == "auto" else layout], (layout, ran)
                    assert (ran[2] in AC.POINTLIKE_KINDS) == c["pointlike"], (ran, c["pointlike"])
                    assert not s.debug_overflow_flags().any()
                    got = HA.canonical(G["assoc_pose"], G["assoc_obst"], c["legacy"])
                    want = HA.canonical(want_pose, want_obst, c["legacy"])
                    np.testing.assert_array_equal(got[0], want[0], err_msg="%s %s mode %d wm %g: poses" % (name, layout, mode, wm))
                    np.testing.assert_array_equal(got[1], want[1], err_msg="%s %s mode %d wm %g: obstacles" % (name, layout, mode, wm))
                    assert HA.same_lists(G["assoc_pose"], G["assoc_obst"], want_pose, want_obst, c["legacy"])
                    if c["hcheck"] and wm == 1.0:
                        check_chi2(G["chi2"], fx[p + "chi2"], fx[p + "rows"])
                        if mode == _abi.JACOBIAN_ANALYTIC:
                            eH, eb = hp.errors(hp.band_of_dense(G["H"]), G["b"], fx[p + "Hband"], fx[p + "b"], fx[p + "chi2"])
                            bound_H, bound_b = np.maximum(BOUND, 16 * fx[p + "oracle_err"])
                            print("%s %s: H error %.1f eps (bound %.0f), b error %.1f eps (bound %.0f)" % (name, layout, eH / EPS, bound_H / EPS, eb / EPS, bound_b / EPS))
                            assert eH <= bound_H and eb <= bound_b, (layout, eH / EPS, eb / EPS)
                        else:   # g2o's central differences against the same quotient at 80 digits (association_cases.numeric_bound)
                            eH, eb = hp.errors(hp.band_of_dense(G["H"]), G["b"], fx[p + "Hband_numeric"], fx[p + "b_numeric"], fx[p + "chi2"])
                            bound = AC.numeric_bound(batch)
                            print("%s %s numeric mode: H error %.2e, b error %.2e (bound %.1e)" % (name, layout, eH, eb, bound))
                            assert eH <= bound and eb <= bound, (layout, eH, eb, bound)
            finally:
                s.close()


def _optimize_once(c, **opt):
    cfg, obst, via, batch = c["cfg"], c["obst"], c["via"], c["batch"]
    s = planner.make_solver(cfg, obst, via, batch, options=_abi.Options(generic_distance_path=True, speculative_trials=-1, **opt))
    try:
        s.optimize(1, 1)
        return s.download(batch.copy()), s.results(), s.last_launch_info(), s.debug_overflow_flags()
    finally:
        s.close()


@pytest.mark.parametrize("name", [n for n in AC.CASES if AC.CASES[n][0] in (AC.ties, AC.straight_ahead, AC.line_centroid_side, AC.forced_clusters,
                                                                             AC.generic_mixed, AC.tight_bound)])
def test_helper_workgroups_leave_the_same_bits(name):
    c = AC.build(name)
    assert c["helpers"] and c["batch"].count == 1
    c["cfg"].jacobian_mode = _abi.JACOBIAN_ANALYTIC
    one, r1, info1, f1 = _optimize_once(c, multi_cu=-1)
    many, rm, infom, fm = _optimize_once(c, multi_cu=8)
    assert info1 == (0, 0, False), info1
    assert infom[0] >= 2 and infom[1] == 0 and not infom[2], infom   # distance helpers ran and were not given up on
    assert not f1.any() and not fm.any()
    np.testing.assert_array_equal(many.n, one.n)
    for k in ("x", "y", "theta", "dt"):
        np.testing.assert_array_equal(getattr(many, k), getattr(one, k))
    for k in ("status", "lm_iterations", "lm_trials", "chi2", "lambda_"):
        np.testing.assert_array_equal(getattr(rm, k), getattr(r1, k))
