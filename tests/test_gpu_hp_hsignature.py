"""The device's H-signatures and class decisions against the exact reference (tests/test_hp_hsignature.py is the CPU side and describes
the reference, the admissibility rule, the error units and the case families of tests/hsignature_cases.py).

Every fixture of tests/golden/hp_hsignature_*.npz goes through teb_amd_compute_h_signatures and teb_amd_filter_equivalence_classes in
the 2-D mode, with the wide 3-D kernel and with the small one (no mpmath needed here):
  values     2-D: max(|dRe|, |dIm|) / (eps S) per BAND, 3-D: |d| / (eps T_l) per band and obstacle, <= max(256, 16 x the CPU oracle's
             error on the same band) - the rule of the linearisation and solve pins; not finite where and only where the reference is;
             3-D also <= 4 ulp x max(1, |want|) of the oracle, as tests/test_gpu_hsignature.py asserts; the two 3-D kernels return
             identical bits on every case;
  decisions  keep / valid / reasonable of every class list of the case (thresholds 2^-3 and 0.1; best none, first, middle; one and
             two plans per class) identical to the exact reference's. A handle remembers its best class: every kernel gets a fresh
             handle and the lists without a best band come first;
  fleet      four scene sets of three cases each (2-D and 3-D; M = 0 / 1 next to 257 and 513, so that workgroups beyond a scene's own
             tiles take the early return; bands interleaved) through teb_amd_compute_h_signatures_per_scene and
             teb_amd_filter_equivalence_classes_per_scene: values bit-equal to the single-scene handles, decisions equal to theirs and
             to the fixture's.

Found with it on an MI355X: nothing - every value under its bound, every decision the reference's, the fleet forms bit-equal. Largest
device error per family (oracle's in brackets; bound max(256, 16 x oracle)): 2-D shapes2d 0.37 (0.14), shapes3d's bands 0.43 (0.10), range
0.04 (0.02), thr2d 0.34 (0.17), thr3d 0.03 (0.03), classes2d 0.07 (0.03); n = 300: below 0.01 - S grows with the segments, and the
floor of 256 needs no replacement by the count of additions (n + ceil(M / 256) + 8 + 16) eps. 3-D: shapes2d 22.1 (22.1), shapes3d 45.7
(45.7), thr2d 9.2 (9.2), thr3d 6.7 (6.7), classes3d 2.8 (2.8): the device returns the oracle's bits in every case. The zero-term question
(a term of mantissa 0 carries its exponent into the alignment of hsig2d_body): nothing is lost - range_corner_cluster 0.01 with the zero
term at the largest product exponent of the table (68, the others down to -55), range_corner_alone 0.02, range_closed_band 0.00; the
shift is an exact ldexp until the exponents are about 970 apart, which no table of <= 520 obstacles reaches.
The whole file (44 tests) takes 1.8 s; the slowest case 0.42 s.
"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import hp_hsignature as HS  # noqa: E402
import hsignature_cases as HC  # noqa: E402
import make_hp_hsignature as MK  # noqa: E402
import fleet_cases  # noqa: E402

from teb_local_planner_amd import planner, _abi  # noqa: E402

pytestmark = pytest.mark.gpu
EPS = np.finfo(float).eps


def test_the_build_has_the_geometry_the_cases_assume():
    assert planner.TebBatchSolver.build_info()[3] == HC.K_THREADS   # lanes per workgroup: obstacles per lane in 2-D, the chunk of the small 3-D kernel


def _solver(c, mode, kern):
    return planner.make_solver(HC.config(mode), c["table"], [], c["batch"], options=_abi.Options(hsig3d_kernel=kern) if kern else None)


def _check_values(name, c, fx, mode, sig, tag):
    """the device's values of one case under the bound; returns the largest error and the largest bound met"""
    p = name + "/"
    oerr = fx[p + "oracle_err%d" % mode]
    worst = 0.0
    for b in range(len(c["bands"])):
        if mode == 2:
            e, same = HS.error_2d(sig[b], fx[p + "H2"][b], fx[p + "S2"][b]), True
        else:
            e, same = HS.error_3d(sig[b], fx[p + "H3"][b], fx[p + "T3"][b])
        print("%s %s band %d: error %.2f (bound %.0f, oracle %.2f)" % (name, tag, b, e, HS.device_bound(oerr[b]), oerr[b]))
        assert same, "%s %s band %d: not finite where the reference is finite, or the other way round: %s" % (name, tag, b, sig[b])
        assert HS.accepts(e, oerr[b], same), "%s %s band %d: error %.1f above the bound %.0f" % (name, tag, b, e, HS.device_bound(oerr[b]))
        worst = max(worst, e)
    return worst


@pytest.mark.parametrize("name", list(HC.CASES))
def test_device_values_and_decisions_against_the_reference(oracle, name):
    fx = MK.load(name)
    c = HC.build(name)
    p = name + "/"
    for key, arr in (("obst", np.array(c["obst"]).reshape(-1, 4)), ("n", c["batch"].n), ("x", c["batch"].x), ("y", c["batch"].y), ("dt", c["batch"].dt)):
        assert np.array_equal(fx[p + key], arr), key   # the fixture is of THESE inputs
        assert arr.dtype.kind != "f" or np.array_equal(np.signbit(fx[p + key]), np.signbit(arr)), key   # ... a -0.0 included
    for mode in c["modes"]:
        bits = []
        want = oracle.h_signatures(HC.config(mode), c["table"], c["batch"], mode, c["prescaler"]) if mode == 3 else None
        for kern in (("wide", "small") if mode == 3 else (None,)):
            s = _solver(c, mode, kern)
            try:
                sig = s.h_signatures(c["prescaler"])
                assert sig.shape == (len(c["bands"]), len(c["obst"]) if mode == 3 else 2)
                _check_values(name, c, fx, mode, sig, "%d-D %s" % (mode, kern or ""))
                if mode == 3:   # the bound of tests/test_gpu_hsignature.py against the oracle stays
                    fin = np.isfinite(want)
                    assert (np.isfinite(sig) == fin).all()
                    assert (np.abs(sig - want)[fin] <= 4 * EPS * max(1.0, np.abs(want[fin]).max(initial=0.0))).all(), np.abs(sig - want)[fin].max()
                for k, (thr, best, plans) in enumerate(c["class_lists"]):
                    got = s.filter_equivalence_classes(thr, best, plans)
                    for what, g, w in zip(("keep", "valid", "reasonable"), got, fx[p + "cls%d" % mode][k]):
                        np.testing.assert_array_equal(g, w, err_msg="%s %d-D %s: %s with threshold %g, best %d, %d plans" % (name, mode, kern, what, thr, best, plans))
                bits.append(sig)
            finally:
                s.close()
        if mode == 3:
            np.testing.assert_array_equal(bits[0], bits[1], err_msg="%s: the wide and the small 3-D kernel differ" % name)


def _fleet(mode, names):
    """the band lists of the cases as ONE batch, interleaved (band k of every case in turn), every case a scene"""
    cs = [HC.build(n) for n in names]
    stride = max(c["batch"].stride for c in cs)
    order = [(s, k) for k in range(max(len(c["bands"]) for c in cs)) for s, c in enumerate(cs) if k < len(c["bands"])]
    batch = _abi.TebBatchHost(len(order), stride)
    for b, (s, k) in enumerate(order):
        x, y, dt = cs[s]["bands"][k]
        batch.set_teb(b, x, y, np.zeros(len(x)), dt)
    return fleet_cases.Fleet(HC.config(mode), [c["table"] for c in cs], [[] for _ in cs], batch, [s for s, _ in order]), cs, order


@pytest.mark.parametrize("mode,names", HC.fleet_sets(), ids=["%d-%s" % (m, "+".join(n)) for m, n in HC.fleet_sets()])
def test_fleet_forms_return_the_bits_of_the_single_scene_handles(mode, names):
    f, cs, order = _fleet(mode, names)
    mo, mv, mw = f.capacities()
    for kern in (("wide", "small") if mode == 3 else ("auto",)):
        s = planner.TebBatchSolver(f.cfg, f.batch.count, f.batch.stride, mo, mv, mw, options=_abi.Options(hsig3d_kernel=kern))
        singles = []
        try:
            s.set_scenes(f.tables, f.vias)
            s.set_band_scenes(f.scene_of)
            s.upload(f.batch)
            sig = s.h_signatures_per_scene(cs[0]["prescaler"])
            for sc, c in enumerate(cs):
                fx = MK.load(names[sc])
                s1 = planner.make_solver(f.cfg, c["table"], [], c["batch"], options=_abi.Options(hsig3d_kernel=kern))
                singles.append(s1)
                one = s1.h_signatures(c["prescaler"])
                idx = f.bands_of(sc)
                assert [order[b][1] for b in idx] == list(range(len(c["bands"])))
                for k, b in enumerate(idx):
                    np.testing.assert_array_equal(sig[b], one[k], err_msg="scene %d (%s), band %d" % (sc, names[sc], k))
                _check_values(names[sc], c, fx, mode, np.array([sig[b] for b in idx]).reshape(one.shape), "%d-D fleet %s" % (mode, kern))
            # the class lists of the set's class case (the other scenes: no best band), lists without a best band first
            lists = max((c["class_lists"] for c in cs), key=len)
            for k, (thr, best, plans) in enumerate(lists):
                per_scene = np.full(len(cs), -1, np.int32)
                for sc, c in enumerate(cs):
                    if best >= 0 and k < len(c["class_lists"]) and c["class_lists"][k] == (thr, best, plans):
                        per_scene[sc] = f.bands_of(sc)[best]
                got = s.filter_equivalence_classes_per_scene(thr, per_scene if best >= 0 else None, plans)
                for sc, c in enumerate(cs):
                    idx = f.bands_of(sc)
                    own = k < len(c["class_lists"]) and c["class_lists"][k] == (thr, best, plans)
                    one = singles[sc].filter_equivalence_classes(thr, best if own else -1, plans)
                    for what, g, h in zip(("keep", "valid", "reasonable"), got, one):
                        np.testing.assert_array_equal(g[idx], h, err_msg="%s, scene %d (%s), list %d against its handle" % (what, sc, names[sc], k))
                    if own:
                        for what, g, w in zip(("keep", "valid", "reasonable"), got, MK.load(names[sc])[names[sc] + "/cls%d" % mode][k]):
                            np.testing.assert_array_equal(g[idx], w, err_msg="%s, scene %d (%s), list %d against the reference" % (what, sc, names[sc], k))
        finally:
            for s1 in singles:
                s1.close()
            s.close()
