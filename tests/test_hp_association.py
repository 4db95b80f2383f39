"""The DECISIONS of the graph build - which pose carries which obstacle / via-point edge - against an exact reference (CPU side).

tests/hp_association.py restates AddEdgesObstacles, AddEdgesViaPoints with findClosestTrajectoryPose and the legacy association over
mpmath at 80 digits, on the distance functions of tests/hp_linearize.py, and records the margin of EVERY comparison it makes. A
comparison is admissible when it is exact in fp64 (every operation rounded to 53 bits gives the 80-digit operands: then it may be a tie
or one ulp off) or separated by a relative 1e-9; anything else raises, nothing is dropped. tests/association_cases.py builds scenes ON the
thresholds (dyadic band, dyadic thresholds, obstacles on the axis through their pose or at Pythagorean offsets): a threshold ladder
(tie, +-1 / +-4 ulp, +-2^-41, +-2^-36 about force, cutoff and the culling radius), every list length and deciding position at which the
device's masks change shape, bit-equal distances decided by list order, forced clusters around the register budget of a slice, pose
counts with 8 / 4 / 2 lanes per pose, generic shapes with a tight and a useless bounding circle, dynamic obstacles either side of the
far-field culling radius, via-points and legacy obstacles equidistant from two poses.

This file
  - checks the ORACLE: on every case the exact reference's lists equal oracle.associate, its via-point poses and the legacy lists equal
    what oracle.edges records (the oracle is pinned to the reference planner's own code: this also says what that code does at a tie);
  - checks the CASES: every comparison admissible (the reference raises otherwise), the fixture under tests/golden/ equal to the
    recomputed reference, and each family contains what it claims - asserted from the reference's own records;
  - for the families whose decisions show in H (static ladder, dynamic culling, via-points) compares oracle.linearize with the 80-digit
    linearisation under the metric and bound of tests/test_hp_linearize.py (the edges ON their penalty threshold exempted from the
    branch-margin check only because their argument is exact in fp64 and >= 4 ulp from the switch point);
  - checks the CHECKER: mutations of the right answer (tie order swapped, the rung-0 candidate dropped, a forced entry moved behind
    left / right, a list reversed within one chunk of 32) are all rejected by the comparison the GPU test uses.

Found with it: nothing on the CPU side - the oracle takes the reference's decision in every case.
Smallest relative margin of a comparison that is NOT exact, per family: ladder 4.3e-3, positions 4.5e-3, ties 5.0e-3, forced 3.4e-3,
generic 1.86e-9 (the +-2^-29 rungs across the 1e-9 guard of the bounding circles; 2.8e-3 otherwise), via-points 0.2, legacy 0.1;
exact comparisons (ties and ulp-distances) per case: 18 on a ladder, one per deciding position, 17 in the straight-ahead case.
Largest error of the oracle's closed forms on the H cases, in eps (H / b): ladder 1.7 / 0.1, dynamic culling 0.9 / 0.6, via-points
1.0 / 0, bound 256; its numeric mode against the central differences at 80 digits <= 7.4e-6 (bound 1.1e-4 .. 1.1e-3). Measured run
time of this file: 80 s on one core (the bands of 260 .. 380 poses against 130 obstacles are half of it).
"""
import collections
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
from test_hp_linearize import check_chi2, BOUND, EPS  # noqa: E402

from teb_local_planner_amd import _abi  # noqa: E402

_REF = {}
EXACT_RUNGS = {"0", "+1ulp", "-1ulp", "+4ulp", "-4ulp", "+2^-41", "-2^-41", "+2^-36", "-2^-36"}


def _ref(name):
    """(case, Reference, association) of a case, computed once per session and left unchanged"""
    if name not in _REF:
        _REF[name] = MK.reference(name)
    return _REF[name]


def _lists(A):
    out = collections.defaultdict(list)
    for p, k in zip(A["assoc_pose"], A["assoc_obst"]):
        out[int(p)].append(int(k))
    return out


def test_the_case_table_covers_every_family():
    fams = collections.Counter(AC.build(n)["family"] for n in AC.CASES)
    assert set(fams) == set(AC.FAMILIES), fams
    have = sorted(f for f in os.listdir(os.path.join(HERE, "golden")) if f.startswith("hp_association_") and f.endswith(".npz"))
    assert have == sorted(stem + ".npz" for stem in MK.groups())
    for f in have:
        assert os.path.getsize(os.path.join(HERE, "golden", f)) < MK.MAX_FILE_BYTES
    lanes = {AC.leftover_lanes(int(AC.build(n)["batch"].n[0])) for n in AC.CASES}
    assert lanes == {1, 2, 4, 8}, lanes   # one lane per pose and the leftover passes with 8, 4 and 2
    assert [AC.leftover_lanes(n) for n in (24, 260, 300, 380)] == [1, 8, 4, 2]


def test_the_kernel_has_the_geometry_the_cases_assume():
    """association_cases restates four things of the kernel sources to know which list positions share a slice and which scene kinds
    are point-like: read them back from the sources, so that a change there fails here instead of leaving the claims stale."""
    import re
    csrc = os.path.join(os.path.dirname(HERE), "teb_local_planner_amd", "csrc")
    kernel = open(os.path.join(csrc, "teb_kernel.hpp")).read()
    device = open(os.path.join(csrc, "teb_device.hpp")).read()
    launch = open(os.path.join(csrc, "teb_opt_launch.hpp")).read()
    assert int(re.search(r"constexpr int kSliceForced = (\d+);", kernel).group(1)) == AC.K_SLICE_FORCED
    assert int(re.search(r"#define TEB_AMD_THREADS (\d+)", device).group(1)) == AC.K_THREADS
    assert "while (G < 8 && 2 * G * poses_left <= kThreads) G *= 2;" in kernel                 # association_cases.lanes_per_pose
    assert "const int chunk = ((sc.n_static + G - 1) / G + 3) & ~3;" in kernel                 # association_cases.slice_width
    assert "(((sc.n_dyn + nsl - 1) / nsl + 3) & ~3)" in kernel                                 # ... and of the dynamic list
    kinds = {int(k): name for k, name in re.findall(r"(\d+) SCENE_(\w+)", launch)}
    assert sorted(kinds) == list(range(12)), kinds
    assert {k for k, name in kinds.items() if name.startswith("POINTS")} == AC.POINTLIKE_KINDS


@pytest.mark.parametrize("name", list(AC.CASES))
def test_reference_against_the_oracle_and_the_fixture(oracle, name):
    c, R, A = _ref(name)
    cfg, obst, via, batch = c["cfg"], c["obst"], c["via"], c["batch"]
    n = int(batch.n[0])
    # ---- admissible: the reference raised otherwise; every record says why it is
    for what, pose, item, rel, exact, lt, eq in R.records:
        assert exact is True or rel >= HA.REL, (what, pose, item, rel)
        assert not eq or exact is True
    # ---- the oracle takes the reference's decisions
    op, oo = oracle.associate(cfg, obst, batch, 0)
    np.testing.assert_array_equal(op, A["assoc_pose"])
    np.testing.assert_array_equal(oo, A["assoc_obst"])
    ir, _ = oracle.edges(cfg, obst, via, batch, 0, 1.0)
    edges = [(int(r[2]), int(r[9])) for r in ir if int(r[0]) in (hp.E_OBST, hp.E_INFL)]
    assert edges == list(zip(A["assoc_pose"].tolist(), A["assoc_obst"].tolist()))
    got_via = {int(r[10]): int(r[2]) for r in ir if int(r[0]) == hp.E_VIA}
    assert got_via == {v: int(p) for v, p in enumerate(A["via_pose"]) if p >= 0}
    if c["claims"].get("dynamic"):   # every pose 1 .. n - 2 carries every dynamic obstacle: nothing is culled in the reference
        dyn = [k for k in range(len(obst)) if obst.dynamic[k]]
        assert sum(int(r[0]) == hp.E_DYN for r in ir) == len(dyn) * (n - 2)
    # ---- the fixture is what the reference gives today
    fx = MK.load(name)
    _, rec = MK.reference_record(name, oracle, ref=(c, R, A))
    keys = sorted(k for k in fx.files if k.startswith(name + "/"))
    assert keys == sorted(rec)
    for k in keys:
        if not k.endswith(("/oracle_err", "/oracle_err_numeric")):
            assert np.array_equal(fx[k], rec[k]), k
    # ---- what the case claims to contain
    _check_claims(c, R, A, ir)
    # ---- H, b, chi^2 of the oracle's closed forms where the decisions show in them
    if c["hcheck"]:
        p = name + "/"
        assert rec[p + "margin"] >= hp.MARGIN
        G = oracle.linearize(cfg, obst, via, batch, 0, 1.0)
        eH, eb = hp.errors(hp.band_of_dense(G["H"]), G["b"], rec[p + "Hband"], rec[p + "b"], rec[p + "chi2"])
        print("%s: H error %.1f eps, b error %.1f eps, smallest branch margin %.3g" % (name, eH / EPS, eb / EPS, rec[p + "margin"]))
        assert eH <= BOUND and eb <= BOUND, (eH / EPS, eb / EPS)
        check_chi2(G["chi2"], rec[p + "chi2"], rec[p + "rows"])
        assert rec[p + "chi2"].sum() > 0 and np.abs(rec[p + "Hband"]).max() > 0, "the decisions of this case do not show in H"
        if c["numeric"]:   # the numeric Jacobian mode against the same central differences at 80 digits
            cfg.jacobian_mode = _abi.JACOBIAN_G2O_NUMERIC
            G = oracle.linearize(cfg, obst, via, batch, 0, 1.0)
            cfg.jacobian_mode = _abi.JACOBIAN_ANALYTIC
            eH, eb = hp.errors(hp.band_of_dense(G["H"]), G["b"], rec[p + "Hband_numeric"], rec[p + "b_numeric"], rec[p + "chi2"])
            bound = AC.numeric_bound(batch)
            print("%s numeric mode: H error %.2e, b error %.2e (bound %.1e)" % (name, eH, eb, bound))
            assert eH <= bound and eb <= bound, (eH, eb, bound)
            if c["family"] == "dynamic":   # ... and the closed forms are NOT that quotient next to the threshold: the check can tell
                assert hp.errors(rec[p + "Hband"], rec[p + "b"], rec[p + "Hband_numeric"], rec[p + "b_numeric"], rec[p + "chi2"])[0] > 0.1


def _check_claims(c, R, A, ir):
    claims, lists = c["claims"], _lists(A)
    by = {(r[0], r[1], r[2]): r for r in R.records}
    for name, p, k, side, forced, associated in claims.get("rungs", []):
        if claims.get("dynamic"):   # the rung is a dynamic obstacle about the culling radius: inside / outside as built, within 2^-35
            e = [q for q, r in enumerate(ir) if int(r[0]) == hp.E_DYN and int(r[2]) == p and int(r[9]) == k]
            args = hp.switch_arguments(c["cfg"], c["obst"], c["via"], c["batch"], 0, 1.0, ir, only=set(e))[e[0]]
            what = {x[3] for x in c["exempt"]}.pop()
            v, lo = [(a[1], a[2]) for a in args if a[0] == what][0]
            assert (v < lo) == associated and v != lo and abs(v - lo) <= 2.0 ** -35 * lo, (name, p, k, v, lo)
            continue
        assert (k in A["forced"][p]) == forced, (name, p, k)
        assert (k in lists[p]) == associated, (name, p, k, lists[p])
        if associated and not forced:
            assert A[side][p] == k, (name, p, k)
        near = [r for r in (by.get(("dist < force", p, k)), by.get(("dist > cutoff", p, k))) if r is not None and r[3] < 1e-8]
        assert near, (name, p, k)
        if name in EXACT_RUNGS:
            assert all(r[4] is True for r in near), (name, p, k)
        if name == "0":
            assert any(r[6] for r in near), "rung 0 is no tie"
    for p, pos in claims.get("deciding", []):
        assert pos in lists[p], (p, pos, lists[p])
        assert by[("dist > cutoff", p, pos)][6], "the deciding obstacle is not exactly at the cutoff"
    for rec in claims.get("ties", []):
        p, kept = rec[0], rec[1]
        assert kept in lists[p]
        for r in rec[2:]:
            assert (p, kept, r) in A["ties"] and r not in lists[p], (rec, A["ties"])
    if "ahead" in claims:
        p, ahead, left = claims["ahead"]
        assert A["right"][p] == ahead and A["left"][p] == left and lists[p] == [left, ahead]
        assert by[("cross > 0", p, ahead)][6] and by[("cross > 0", p, ahead)][4] is True   # exactly 0
    if "centroid_side" in claims:
        p, line, point = claims["centroid_side"]
        assert lists[p] == [point] and A["right"][p] is None
        assert by[("dist < side minimum", p, point)][5], "the point does not beat the line on the left"
    for p, where in claims.get("clusters", []):
        assert A["forced"][p] == where and A["left"][p] is not None and A["right"][p] is not None, (p, A["forced"][p], where)
        assert lists[p][:len(where)] == where and len(lists[p]) == len(where) + 2
    for key in ("kept", "tangential"):
        if key in claims:
            p, kept, rejected = claims[key]
            assert kept in lists[p] and rejected not in lists[p], (key, lists[p])
    if "kept" in claims:
        p, kept, rejected = claims["kept"]
        assert kept < rejected and (p, kept, rejected) in A["ties"]   # (either order of T and E puts the kept one first in the table)
    if "via" in claims:
        assert A["via_pose"].tolist() == claims["via"]
    if claims.get("closest") is not None:
        assert [A["closest"][k] for k in range(len(claims["closest"]))] == claims["closest"]


def test_the_families_contain_what_they_claim():
    per_slice, straddle, rung_sides = [], 0, collections.defaultdict(set)
    for name in AC.CASES:
        c = AC.build(name)
        n, M = int(c["batch"].n[0]), len(c["obst"])
        G = AC.leftover_lanes(n)
        w = AC.slice_width(M, G)
        if c["family"] == "forced" and G > 1:
            for p, where in c["claims"]["clusters"]:
                assert p >= AC.K_THREADS
                per_slice += list(collections.Counter(pos // w for pos in where).values())
        if c["family"] == "ties" and G > 1:
            for rec in c["claims"].get("ties", []):
                assert rec[0] >= AC.K_THREADS
                straddle += rec[1] // w != rec[2] // w
        if c["family"] == "positions" and G > 1:
            pos = sorted(q for _, q in c["claims"]["deciding"])
            assert any(b == a + 1 and a // w != b // w for a, b in zip(pos, pos[1:])), (name, w, pos)
        if c["family"] in ("ladder", "generic", "dynamic"):
            for r in c["claims"].get("rungs", []):
                rung_sides[(name, r[0])].add(r[3])
    # forced entries of one slice: fewer than, exactly and more than the registers that hold them
    assert min(per_slice) < AC.K_SLICE_FORCED and AC.K_SLICE_FORCED in per_slice and max(per_slice) > AC.K_SLICE_FORCED, sorted(per_slice)
    assert straddle >= 6, straddle   # ties whose two obstacles lie in different slices: the merge across slices decides them
    for name in AC.CASES:
        c = AC.build(name)
        if c["claims"].get("rungs"):
            want = AC.RUNGS_DYNAMIC if c["family"] == "dynamic" else AC.RUNGS_GUARD9 if "tight_ladder" in name else AC.RUNGS
            for rname, _ in want:
                assert rung_sides[(name, rname)] == {"left", "right"}, (name, rname)


def test_the_comparison_rejects_wrong_answers():
    def fixture(name):
        fx = MK.load(name)
        return fx[name + "/assoc_pose"], fx[name + "/assoc_obst"]
    # a tie resolved towards the later obstacle
    pose, obst = fixture("ties_n380")
    for rec in AC.build("ties_n380")["claims"]["ties"]:
        assert HA.same_lists(pose, obst, pose, obst)
        assert not HA.same_lists(*HA.mutate_replace(pose, obst, rec[0], rec[1], rec[2]), pose, obst)
    # the candidate exactly at the cutoff dropped, the one exactly at force forced (it then precedes its companion... which stays out)
    pose, obst = fixture("ladder_cutoff_point_point")
    for name, p, k, side, forced, associated in AC.build("ladder_cutoff_point_point")["claims"]["rungs"]:
        if name == "0":
            assert not HA.same_lists(*HA.mutate_drop(pose, obst, p, k), pose, obst)
    pose, obst = fixture("ladder_force_point_point")
    for name, p, k, side, forced, associated in AC.build("ladder_force_point_point")["claims"]["rungs"]:
        if name == "0":   # forced: the companion becomes the candidate of its side and follows
            wrong = (np.insert(pose, np.flatnonzero(pose == p)[-1] + 1, p), np.insert(obst, np.flatnonzero(pose == p)[-1] + 1, k - 1))
            assert not HA.same_lists(*wrong, pose, obst)
    # a forced entry moved behind left / right
    pose, obst = fixture("forced_consecutive_n300")
    for p, where in AC.build("forced_consecutive_n300")["claims"]["clusters"]:
        assert not HA.same_lists(*HA.mutate_swap_within_pose(pose, obst, p, 0, len(where) + 1), pose, obst)
    # the bit order of one chunk of 32 reversed
    for name in ("positions_M65", "positions_M130", "positions_n300"):
        pose, obst = fixture(name)
        M = len(AC.build(name)["obst"])
        changed = 0
        for chunk in range((M + 31) // 32):
            wrong = np.where(obst // 32 == chunk, HA.mutate_reverse_chunk(obst, M), obst)
            if (wrong != obst).any():   # (a last chunk of one position is its own mirror image)
                changed += 1
                assert not HA.same_lists(pose, wrong, pose, obst), (name, chunk)
        assert changed >= 2, name
    # the legacy lists are a multiset per pose: any order of the same entries passes, a changed entry does not
    pose, obst = fixture("legacy_tie")
    perm = np.random.default_rng(0).permutation(len(pose))
    assert HA.same_lists(pose[perm], obst[perm], pose, obst, legacy=True) and not HA.same_lists(pose[perm], obst[perm], pose, obst)
    assert not HA.same_lists(*HA.mutate_drop(pose, obst, int(pose[0]), int(obst[0])), pose, obst, legacy=True)
    moved = pose.copy()
    moved[0] += 1   # the earlier of two equidistant poses replaced by the later
    assert not HA.same_lists(moved, obst, pose, obst, legacy=True)
