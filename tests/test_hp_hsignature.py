"""H-signatures and class decisions - what the planner does with a band - against an exact reference (CPU side).

tests/hp_hsignature.py restates HSignature::calculateHSignature, HSignature3d::calculateHSignature, isEqual / isValid / isReasonable
and the class list over mpmath at 80 digits and records the margin of EVERY comparison: |o_l - o_j| against 0.05, |end - start| against
3.0, the five proposals of the unwrapping, diff against 0, the direction norm against 1e-15, an integration point on the conductor,
and every class decision against the error the device is allowed. tests/hsignature_cases.py places small scenes ON those thresholds,
on the tile / chunk / lane edges of the kernels and at the ends of the exponent range.

This file
  - checks the CASES: every comparison admissible (the reference raises otherwise), the fixture under tests/golden/ equal to the
    recomputed reference, each family contains what it claims - asserted from the reference's own records;
  - checks the ORACLE: its error in the units of the reference (2-D: max(|dRe|, |dIm|) / (eps S) per band, 3-D: |d| / (eps T_l)) is at
    most 4096 on every case - a condition on the INPUTS, which keeps the device's bound max(256, 16 x oracle) from becoming vacuous -
    it is finite where and only where the reference is, and oracle.filter_equivalence_classes on its signatures takes the exact
    reference's keep / valid / reasonable on every class list;
  - checks the CHECKER: mutations of the exact answer must all fail the comparison the GPU test uses (hp_hsignature.accepts): one unwrap
    off by 2 pi on the obstacle with the smallest |A_l| of a few-obstacle case, one product exponent off by one, b = a at odd m, the
    0.05 skip flipped for one pair, the last segment dropped (n = 300), one 3-D integration step dropped, one lane's term dropped at
    M = 257 (the second obstacle of lane 0 and a lone one). a <-> b swapped is NO wrong answer: the text uses a and b only as the
    product a * b (the pow() form is commented out in h_signature.h:151), so the swap leaves H unchanged - asserted here;
  - reads kHsTile, kHsChunk, TEB_AMD_THREADS and the literals 0.05, 3.0, 1e-15, 120 back from the kernel sources.

Observed (oracle error, largest per family, 2-D / 3-D; bound 4096): shapes2d 0.14 / 22.1, shapes3d 0.10 / 45.7, range 0.02 / -, thr2d
0.17 / 9.2, thr3d 0.03 / 6.7, classes2d 0.03 / -, classes3d - / 2.8. The 2-D oracle works in long double: its error is the final
rounding. Smallest relative margin of a comparison that is not exact: shapes2d 4.7e-4 (a chord of the 513-ring next to 0.05), shapes3d
5.2e-4, range 0.2, thr2d 0.051, thr3d 0.11, classes2d 0.25, classes3d 0.051; exact comparisons: 37 (35 of them in thr2d), 13 of them ties;
smallest class margin: 1.0e3 x the allowed error (classes2d: the goal 2^-10 of the threshold inside / outside), 1.5e8 x in 3-D. The
ten-step rule puts a closed loop of 8 segments at H_l = 0.892 (< 1.0: reasonable), one and a half loops at 1.387. Nothing found on the
CPU side: the oracle takes the reference's decision on every class list. Measured run time of this file: 55 s on one core (M = 513:
12 s, the two lattices of 200: 9 s).
"""
import collections
import math
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import hp_hsignature as HS  # noqa: E402
import hsignature_cases as HC  # noqa: E402
import make_hp_hsignature as MK  # noqa: E402

import mpmath  # noqa: E402

_REF = {}


def _ref(name):
    """(case, {mode: reference}) of a case, computed once per session and left unchanged"""
    if name not in _REF:
        _REF[name] = MK.reference(name)
    return _REF[name]


def test_the_case_table_covers_every_family():
    fams = collections.Counter(HC.build(n)["family"] for n in HC.CASES)
    assert set(fams) == set(HC.FAMILIES), fams
    assert all(n.split("_")[0] == HC.build(n)["family"] for n in HC.CASES)
    have = sorted(f for f in os.listdir(os.path.join(HERE, "golden")) if f.startswith("hp_hsignature_") and f.endswith(".npz"))
    assert have == sorted(stem + ".npz" for stem in MK.groups())
    for f in have:
        assert os.path.getsize(os.path.join(HERE, "golden", f)) < MK.MAX_FILE_BYTES
    import make_hp_association
    assert MK.MAX_FILE_BYTES == make_hp_association.MAX_FILE_BYTES
    shapes = {(len(HC.build(n)["obst"]), len(b[0])) for n in HC.CASES for b in HC.build(n)["bands"]}
    assert {M for M, _ in shapes} >= {0, 1, 2, 5, 6, 7, 8, 15, 16, 17, 33, 255, 256, 257, 400, 513}
    assert {n for M, n in shapes if M == 3} >= {2, 3, 257, 300}
    for M in (1, 15, 16, 17, 33):   # the tile edges of the small 3-D kernel x its chunk edges
        assert {n - 1 for m, n in shapes if m == M} >= {1, 15, 16, 17, 33}, M
    assert max(M for M, _ in shapes) <= 520 and max(n for _, n in shapes) <= 300
    assert (2, 300) in shapes and (257, 3) in shapes
    for mode, names in HC.fleet_sets():
        Ms = [len(HC.build(n)["obst"]) for n in names]
        assert len(set(Ms)) == 3 and all(mode in HC.build(n)["modes"] for n in names), (mode, names)
    assert any(min(len(HC.build(n)["obst"]) for n in names) <= 1 and max(len(HC.build(n)["obst"]) for n in names) >= 257 for _, names in HC.fleet_sets())


def test_the_kernel_has_the_geometry_the_cases_assume():
    """hsignature_cases restates the tile, the chunk, the lane count and four literals of the kernel sources: read them back, so that a
    change there fails here instead of leaving the cases beside the edges they were built for."""
    csrc = os.path.join(os.path.dirname(HERE), "teb_local_planner_amd", "csrc")
    hsig = open(os.path.join(csrc, "teb_hsig.hpp")).read()
    device = open(os.path.join(csrc, "teb_device.hpp")).read()
    assert int(re.search(r"#define TEB_AMD_THREADS (\d+)", device).group(1)) == HC.K_THREADS
    assert "constexpr int kThreads = TEB_AMD_THREADS;" in device
    assert re.search(r"constexpr int kHsTile = (\d+), kHsChunk = kThreads / kHsTile;", hsig), "kHsTile / kHsChunk"
    assert int(re.search(r"constexpr int kHsTile = (\d+),", hsig).group(1)) == HC.K_HS_TILE and HC.K_THREADS // HC.K_HS_TILE == HC.K_HS_CHUNK
    assert hsig.count("sqrt(sqn3(dir)) < 1e-15") == 2 and float("1e-15") == HC.COINCIDENT == HS.COINCIDENT          # both 3-D bodies
    assert hsig.count("const double tt = 120;") == 2 and HC.CONDUCTOR_T == HS.CONDUCTOR_T == 120.0
    assert "if (sqrt(dr * dr + di * di) < 0.05) continue;" in hsig and HC.SKIP_DIST == HS.SKIP_DIST == 0.05
    assert "if (sqrt(dx * dx + dy * dy) < 3.0)" in hsig and HC.MAP_DIST == HS.MAP_DIST == 3.0
    assert "for (int l = threadIdx.x; l < M; l += kThreads)" in hsig and "for (int i = threadIdx.x; i < n; i += kThreads)" in hsig
    assert hsig.count("for (int k = 0; k < 10; ++k)") == 3 and HS.STEPS == 10                                          # two loops of terms, one of sums


def _values_of(c, mode, res):
    return MK.exact_arrays(mode, res, len(c["obst"]))


@pytest.mark.parametrize("name", list(HC.CASES))
def test_reference_against_the_oracle_and_the_fixture(oracle, name):
    c, R = _ref(name)
    fx = MK.load(name)
    _, rec = MK.reference_record(name, oracle, ref=(c, R))
    # ---- admissible: the reference raised otherwise; every record says why it is
    for mode, r in R.items():
        for what, idx, rel, exact, lt, eq in r["rec"].records:
            if what.startswith("class "):
                assert rel >= 1.0, (what, idx, rel)
            else:
                assert exact is True or rel >= HS.REL, (what, idx, rel)
                assert not eq or exact is True
    # ---- the fixture is what the reference gives today
    keys = sorted(k for k in fx.files if k.startswith(name + "/"))
    assert keys == sorted(rec)
    for k in keys:
        if "/oracle_err" not in k:
            assert np.array_equal(fx[k], rec[k], equal_nan=True), k
    # ---- the oracle: its condition, its finite pattern, its class decisions
    for mode, r in R.items():
        errs, same, sig = MK.oracle_errors(c, mode, R, oracle)
        print("%s mode %d: oracle error %s (bound %g), margins %s" % (name, mode, np.array2string(errs, precision=2), HS.ORACLE_BOUND,
                                                                       np.array2string(rec[name + "/margins%d" % mode], precision=3)))
        assert same, "the oracle is not finite where and only where the reference is"
        assert (errs <= HS.ORACLE_BOUND).all(), errs
        for (thr, best, plans), want in zip(c["class_lists"], r["cls"]):
            got = oracle.filter_equivalence_classes(mode, sig, thr, best, plans)
            for what, g, w in zip(("keep", "valid", "reasonable"), got, want):
                np.testing.assert_array_equal(g, w, err_msg="%s mode %d, %s with threshold %g, best %d, %d plans" % (name, mode, what, thr, best, plans))
    _check_claims(c, R)


def _check_claims(c, R):
    cl = c["claims"]
    r2 = R.get(2, {}).get("bands")
    r3 = R.get(3, {}).get("bands")
    by = {}
    for r in R.values():
        by.update({(q[0], q[1]): q for q in r["rec"].records})
    M = len(c["obst"])
    if cl.get("ab"):
        m = max(M - 1, 5)
        assert (r2[0]["a"], r2[0]["b"]) == ((m + 1) // 2, m // 2) if M else (0, 0)
    if cl.get("lanes"):   # the circle: every |A_l| within 2^8 of every other, so that ONE lost term is far above the bound
        e = [HS.mant_exp(v)[1] for v in r2[0]["absA"]]
        assert max(e) - min(e) <= 8, (min(e), max(e))
        assert len(r2[0]["skipped_pairs"]) in (2 * M, 4 * M), len(r2[0]["skipped_pairs"])   # the neighbours closer than 0.05 (513: four either side)
    for rname, l, j, skipped in cl.get("skip_rungs", []):
        q = by[("2d skip", (l, j))]
        assert ((l, j) in r2[0]["skipped_pairs"]) == skipped and q[3] is True and q[4] == skipped, (rname, q)
        assert q[5] == (rname == "0")
    for rname, b, small in cl.get("map_rungs", []):
        q = by[("2d map guess", (b,))]
        assert r2[b]["small_map"] == small and q[3] is True and q[5] == (rname == "0"), (rname, q)
    if "map_rungs" in cl:   # the two forms of the guess give different A_l: the decision shows in the value
        assert abs(r2[0]["H"] - r2[2]["H"]) > 1e-3 * abs(r2[0]["H"])
    for b, pose, l in cl.get("on_centroid", []):
        n = len(c["bands"][b][0])
        want = [(i, l) for i in (pose - 1, pose) if 0 <= i < n - 1]
        assert r2[b]["skipped_segments"] == want and by[("2d diff == 0", (b, pose, l))][5], (b, r2[b]["skipped_segments"])
    if "on_centroid" in cl:   # 3-D: a pose on a static obstacle is an integration point on its conductor - but never the LAST pose
        assert [sorted(q["not_finite"]) for q in r3] == [[0], [1], []]
    for b, pose, l, sign in cl.get("ray", []):
        sel = r2[b]["selections"]
        assert (sel[(pose - 1, l)], sel[(pose, l)]) == ((0, 1) if sign > 0 else (1, 0)), (b, sel[(pose - 1, l)], sel[(pose, l)])
    if "ray" in cl:
        assert r2[0]["L"][0] == r2[1]["L"][0]   # +pi or -pi at the end point: the unwrapped sum is the same
    if "straddle" in cl:
        b, seg, l = cl["straddle"]
        assert r2[b]["selections"][(seg, l)] == 1 and abs(r2[b]["L"][l].imag) < 4
    for b, seg, l, win in cl.get("pi_ties", []):
        assert r2[b]["selections"][(seg, l)] == win
        ties = [q for q in R[2]["rec"].records if q[0] == "2d proposal" and q[1][:3] == (b, seg, l) and q[5]]
        assert len(ties) == 1 and ties[0][3] is True, ties   # |arg| = |arg -+ 2 pi|: decided by the order of the proposals
    for b, w in enumerate(cl.get("windings", [])):
        assert int(r2[b]["L"][0].imag / (2 * mpmath.pi)) == w, (b, r2[b]["L"][0].imag)
    for b, skipped in cl.get("coincident", []):
        assert (r3[b]["skipped"] == [2]) == skipped and (skipped or r3[b]["skipped"] == [])
    if "coincident" in cl:
        rels = sorted(q[2] for q in R[3]["rec"].records if q[0] == "3d coincident" and q[1][1] == 2)
        assert 0.1 < rels[0] == rels[1] < 0.12 and 0.4 < rels[2] == rels[3] < 0.45 and rels[4] == 1.0, rels   # 2^-50, 2^-49 and 0 against 1e-15
    if "moving" in cl:
        assert max(math.hypot(o[2], o[3]) for o in c["obst"]) == cl["moving"] and any(o[2] == 0 and o[3] == 0 for o in c["obst"])
    if "not_finite" in cl:
        assert [(b, l) for b, q in enumerate(r3) for l in sorted(q["not_finite"])] == cl["not_finite"]
        for b, l in cl["not_finite"]:
            assert by[("3d |d| == 0", (b, l) + r3[b]["not_finite"][l])][5]
    for b, l in cl.get("above_one", []):
        assert r3[b]["H"][l] > 1
    if "loops" in cl and c["family"] == "thr3d":
        print("the ten-step rule around a static obstacle: closed loop %s, one and a half %s, clockwise %s" %
              tuple(mpmath.nstr(r3[b]["H"][0], 6) for b in cl["loops"]))
        assert [int(k) for k in R[3]["cls"][0][2]] == [int(not r3[b]["H"][0] > 1) for b in cl["loops"]]
    if "zero_terms" in cl:
        for q in r2:
            assert [l for l in range(M) if q["absA"][l] == 0] == cl["zero_terms"] and q["S"] > 0
    if "largest_exponent" in cl or "exponent_spread" in cl:
        e = [HS.mant_exp(v)[1] for v in r2[0]["absP"]]
        print("%s: product exponents %d .. %d, the largest at obstacle %d" % (c["name"], min(e), max(e), int(np.argmax(e))))
        assert max(e) - min(e) >= 40
        if "largest_exponent" in cl:   # the term of mantissa 0 carries the largest exponent of the table into the alignment
            assert int(np.argmax(e)) == cl["largest_exponent"] and sorted(e)[-1] > sorted(e)[-2]
    if cl.get("out_of_range"):
        ob = np.array(c["obst"])
        part = -np.log2(np.hypot(ob[200:, None, 0] - ob[None, :200, 0], ob[200:, None, 1] - ob[None, :200, 1])).sum(axis=1)
        assert part.max() < -1074 - 30, part.max()   # the running product of the second lattice over the first, |f0| <= 2^30 included: below the smallest fp64 number
        for q in r2:
            assert 2.0 ** -1000 < float(q["S"]) < 1 and abs(q["H"]) < q["S"]   # the scale is back in the range (the terms cancel below it)
    if "zero_sum" in cl:
        q = r2[cl["zero_sum"]]
        assert all(abs(v) < 1e-70 for v in q["L"]) and abs(q["H"]) < 1e-70 * q["S"] and q["S"] > 0 and q["small_map"]   # 0 to the digits carried
    thr = 2.0 ** -3
    for p, q, inside in cl.get("near", []):
        d = r2[q]["H"] - r2[p]["H"]
        g = max(abs(d.real), abs(d.imag))
        assert (thr * (1 - 2.0 ** -9) < g < thr) if inside else (thr < g < thr * (1 + 2.0 ** -9)), (p, q, float(g))
    for p, q in cl.get("equal", []):
        assert abs(r2[q]["H"] - r2[p]["H"]) < 1e-9
    for p, q in cl.get("unequal", []):
        assert abs(r2[q]["H"] - r2[p]["H"]) > 1
    for b, l, below in cl.get("near3", []):
        g = abs(r3[b]["H"][l])
        assert (thr * (1 - 2.0 ** -5) < g < thr) if below else (thr < g < thr * (1 + 2.0 ** -5)), (b, l, float(g))
    for p, q, l in cl.get("sides", []):
        assert r3[p]["H"][l] * r3[q]["H"][l] < 0 and min(abs(r3[p]["H"][l]), abs(r3[q]["H"][l])) > 0.25
    if c["family"] == "classes3d":
        for keep, valid, reas in R[3]["cls"]:
            assert valid.tolist() == [1, 1, 1, 1, 0, 1] and reas.tolist() == [1, 1, 1, 1, 1, 0]
        assert len({tuple(k[0]) for k in R[3]["cls"]}) >= 3
    if c["family"] == "classes2d":
        assert len({tuple(k[0]) for k in R[2]["cls"]}) >= 5   # threshold, best and plans per class all change the kept set


def _got2(res):
    return np.array([float(res["H"].real), float(res["H"].imag)])


def test_the_comparison_rejects_wrong_answers():
    def right_and_wrong_2d(name, band, mutate):
        c, R = _ref(name)
        good = R[2]["bands"][band]
        ex, S = _values_of(c, 2, good)
        assert HS.accepts(HS.error_2d(_got2(good), ex, S), 0.0) and HS.error_2d(_got2(good), ex, S) <= 0.5
        bad = MK.reference(name, mutate=mutate(good), band=band, modes=(2,))[1][2]["bands"][band]
        return HS.error_2d(_got2(bad), ex, S), bad, good

    smallest = lambda good: int(np.argmin([float(v) for v in good["absA"]]))
    # one unwrap off by 2 pi on the obstacle with the smallest |A_l|; one product exponent off by one (the same obstacle)
    for mutate in (lambda g: ("unwrap", smallest(g), 0), lambda g: ("exponent", smallest(g))):
        e, _, _ = right_and_wrong_2d("shapes2d_M5", 0, mutate)
        assert not HS.accepts(e, 0.0), e
    # a and b enter only as a * b: the swap is no wrong answer. b = a at odd m (m = 7: 4 * 4 for 4 * 3) is one
    e, bad, good = right_and_wrong_2d("shapes2d_M8", 0, lambda g: ("swap_ab",))
    assert (good["a"], good["b"]) == (4, 3) and (bad["a"], bad["b"]) == (3, 4) and bad["H"] == good["H"] and e <= 0.5
    e, _, _ = right_and_wrong_2d("shapes2d_M8", 0, lambda g: ("b_equals_a",))
    assert not HS.accepts(e, 0.0), e
    # the 0.05 skip flipped for the pair exactly at 0.05
    e, _, _ = right_and_wrong_2d("thr2d_skip", 0, lambda g: ("flip_skip", 0, 1))
    assert not HS.accepts(e, 0.0), e
    # the last of 299 segments dropped
    e, _, _ = right_and_wrong_2d("shapes2d_n300", 0, lambda g: ("drop_last_segment",))
    assert not HS.accepts(e, 0.0), e
    # one lane's term dropped at M = 257: obstacle 256 (the second of lane 0) and obstacle 100 (alone on its lane)
    c, R = _ref("shapes2d_M257")
    good = R[2]["bands"][0]
    ex, S = _values_of(c, 2, good)
    for l in (256, 100):
        with mpmath.workdps(HS.DPS):
            H = good["H"] - good["A"][l] * good["L"][l]
        assert not HS.accepts(HS.error_2d(np.array([float(H.real), float(H.imag)]), ex, S), 0.0)
    # one of 160 integration steps dropped (3-D, every obstacle of the case)
    c, R = _ref("shapes3d_M17")
    good = R[3]["bands"][2]
    ex, T = _values_of(c, 3, good)
    e, same = HS.error_3d(ex[:, 0], ex, T)
    assert same and HS.accepts(e, 0.0) and e <= 0.5
    bad = MK.reference("shapes3d_M17", mutate=("drop_step", 5, 3), band=2, modes=(3,))[1][3]["bands"][2]
    for l in range(len(c["obst"])):
        got = ex[:, 0].copy()
        got[l] = float(bad["H"][l])
        e, same = HS.error_3d(got, ex, T)
        assert same and not HS.accepts(e, 0.0), (l, e)
    # not finite where the reference is finite, and the other way round
    c, R = _ref("thr3d_on_conductor")
    ex, T = _values_of(c, 3, R[3]["bands"][1])
    got = ex[:, 0].copy()
    assert HS.error_3d(got, ex, T)[0] <= 0.5 and HS.error_3d(got, ex, T)[1]
    got[0] = 0.0
    assert not HS.accepts(*HS.error_3d(got, ex, T)[:1], 0.0, HS.error_3d(got, ex, T)[1])
    got = ex[:, 0].copy(); got[1] = np.inf
    assert not HS.accepts(0.0, 0.0, HS.error_3d(got, ex, T)[1])
    # the bound itself
    assert HS.device_bound(0.0) == 256 and HS.device_bound(100.0) == 1600 and HS.accepts(256.0, 0.0) and not HS.accepts(257.0, 0.0)
