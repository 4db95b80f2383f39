"""The DECISIONS of the exploration graph - which obstacles get key points, which is nearest to the start, which ordered vertex pairs
carry an edge - against an exact restatement, on their thresholds (CPU side).

tests/hp_explore_graph.py restates lrKeyPointGraph::createGraph and ProbRoadmapGraph::createGraph with checkLineIntersection of all five
obstacle types and check_line_segments_intersection_2d as plain loops, evaluated op by op in fp64 and, beside it, with mpmath at 80
digits; it records EVERY comparison with its relative margin and classifies it as separated (>= 1e-9), exact (fp64 operands equal the
80-digit ones) or a declared rounded rung (threshold k ulp from the fp64-evaluated quantity, expectation = the op-by-op fp64 outcome);
anything else raises, nothing is dropped. tests/explore_graph_cases.py builds the scenes (families fwd, head, front, disc, seg, lanes,
table, fleet - see there).

This file
  - checks on every case: restatement = the reference planner's own binary (oracle/_ref, where it can be built; the generator of the
    fixtures refuses a case on which it disagrees) = the CPU oracle (which draws its own samples: the generator of the restatement is
    checked with it) on vertices and adjacency, and the committed fixture equals the recomputed one field by field;
  - checks the CASES: the coverage each family claims is asserted from the recorded comparisons - every comparison kind occurs as a
    tie, on both sides of a rung where a rung can exist, and separated; the deciding lanes, waves and table positions are where the
    names say;
  - checks the CHECKER: each of the thirteen mutations of hp_explore_graph.MUTATIONS changes the vertices or the adjacency of at least
    one case, the fused cross product on the few-ulp rungs of the seg family.

Found with it: nothing on the CPU side - the oracle and the reference binary take the restatement's decision in all 202 cases (among
them: an obstacle ON the start gets key points, because 0 / 0 < 0.1 is false; a segment that only touches counts as crossing for one
sign of denom and as clear for the other).
"""
import collections
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import hp_explore_graph as HG  # noqa: E402
import explore_graph_cases as EC  # noqa: E402
import make_hp_explore_graph as MK  # noqa: E402

from teb_local_planner_amd import _abi  # noqa: E402

_REF, _FIX = {}, {}
K = HG.KIND_ID


def _ref(name):
    """(case, Graph, result) of a case, computed once per session and left unchanged"""
    if name not in _REF:
        _REF[name] = MK.reference(name)
    return _REF[name]


def _fixture(name):
    fam = name.split("_")[0]
    if fam not in _FIX:
        _FIX[fam] = MK.load(fam)
    return _FIX[fam][name]


def _binary():
    from oracle import ref_py
    if os.environ.get("TEB_REF_GOLDEN_ONLY") or not ref_py.available():
        return None
    try:
        ref_py.lib()
    except Exception:
        return None
    return ref_py


def _records(names):
    """[n, 6] records of the named cases: kind, class, margin, outcome, tie, sign"""
    return np.concatenate([_ref(n)[1].record_array() for n in names])


def test_the_case_table_covers_every_family_and_the_sources_are_what_the_cases_assume():
    fams = collections.Counter(n.split("_")[0] for n in EC.CASES)
    assert set(fams) == set(EC.FAMILIES), fams
    have = sorted(f for f in os.listdir(os.path.join(HERE, "golden")) if f.startswith(MK.STEM) and f.endswith(".npz"))
    assert have == sorted(stem + ".npz" for stem in MK.groups())
    for f in have:
        assert os.path.getsize(os.path.join(HERE, "golden", f)) < MK.MAX_FILE_BYTES
    assert (HG.OB_POINT, HG.OB_CIRCULAR, HG.OB_LINE, HG.OB_PILL, HG.OB_POLYGON) == \
        (_abi.OBST_POINT, _abi.OBST_CIRCULAR, _abi.OBST_LINE, _abi.OBST_PILL, _abi.OBST_POLYGON)
    csrc = os.path.join(os.path.dirname(HERE), "teb_local_planner_amd", "csrc")
    assert int(re.search(r"#define TEB_AMD_THREADS (\d+)", open(os.path.join(csrc, "teb_device.hpp")).read()).group(1)) == EC.K_THREADS
    graph = open(os.path.join(csrc, "teb_graph.hpp")).read()
    assert "graph_edges_body(sc, g, (long long)blockIdx.x * kThreads + threadIdx.x);" in graph   # one lane per ordered pair, idx = i * N + j
    assert "__builtin_amdgcn_ballot_w64(edge)" in graph                                           # waves of 64 decide the early exit


@pytest.mark.parametrize("name", list(EC.CASES))
def test_restatement_reference_binary_oracle_and_fixture_agree(oracle, name):
    c, g, r = _ref(name)
    rec = g.record_array()
    # ---- admissible: the restatement raised otherwise; every record says why it is
    assert len(rec) >= 1
    for kind, cls, rel, out, tie, sgn in rec:
        assert cls in (HG.SEPARATED, HG.EXACT, HG.RUNG)
        assert cls != HG.SEPARATED or rel >= HG.REL
        assert cls != HG.RUNG or HG.KINDS[int(kind)] in c["rungs"]
    if not MK.libm_exact(c):
        assert not (rec[:, 1] == HG.RUNG).any()
    # ---- the reference planner's own createGraph
    ref = _binary()
    if ref is not None:
        V, A = MK.reference_binary(c, ref)
        np.testing.assert_array_equal(V, r["vertices"])
        np.testing.assert_array_equal(A, r["adjacency"])
    # ---- the oracle, drawing its own samples, and with the restatement's
    V, A, n_paths, n_total = MK.oracle_run(c, oracle)
    np.testing.assert_array_equal(V, r["vertices"])
    np.testing.assert_array_equal(A, r["adjacency"])
    assert n_paths <= c["max_paths"] and n_total <= max(c["max_classes"], 1)
    if g.units:
        V, A, _, _ = MK.oracle_run(c, oracle, units=g.units)
        np.testing.assert_array_equal(V, r["vertices"])
        np.testing.assert_array_equal(A, r["adjacency"])
    # ---- the committed fixture is the recomputed one
    fix, new = _fixture(name), MK.record(name, (c, g, r))[1]
    assert set(fix) == set(new)
    for key in new:
        want = np.asarray(new[key])
        assert fix[key].dtype == want.dtype and np.array_equal(fix[key].ravel(), want.ravel(), equal_nan=True), (name, key)


def test_the_graph_does_not_depend_on_the_bounds_of_the_enumeration(oracle):
    c, g, r = _ref("lanes_n16_keypoint")
    seen = [MK.oracle_run(c, oracle, max_classes=mc, max_paths=mp) for mc, mp in ((1, 8), (3, 64))]
    assert seen[0][2] <= 8 and seen[1][2] <= 64 and seen[1][3] > seen[0][3]   # the second setting does enumerate further
    for V, A, _, _ in seen:
        np.testing.assert_array_equal(V, r["vertices"])
        np.testing.assert_array_equal(A, r["adjacency"])


# ---- the checker is checked -----------------------------------------------------------------------------------------------------------------
def _float_graph(name, mut=None):
    r = HG.Graph(EC.build(name), "float", mut).run()
    return r["vertices"], r["adjacency"]


def _differs(name, mut):
    V0, A0 = _ref(name)[2]["vertices"], _ref(name)[2]["adjacency"]
    V, A = _float_graph(name, mut)
    return V.shape != V0.shape or not np.array_equal(V, V0) or not np.array_equal(A, A0)


EXPECTED_TO_CATCH = {   # mutation -> a case that must notice it (every other case is searched too)
    "fwd_lt": "fwd_perpendicular_thr0", "head_lt": "head_345_0", "dmin_le": "disc_start_keypoint_0", "no_lo_clamp": "disc_before_keypoint_-1ulp",
    "no_hi_clamp": "disc_beyond_roadmap_-1ulp", "no_radius": "disc_radius_larger_than_distance", "denom_ge": "seg_s1_e+o+",
    "denom0_cross": "seg_collinear_e+o+", "no_closing": "seg_triangle_closing_edge_only", "no_half": "disc_before_keypoint_-1ulp",
    "front_le": "front_ladder_0", "near_le": "head_equal_distance", "fma": "seg_nearly_parallel_2^-30"}


@pytest.mark.parametrize("mut", list(HG.MUTATIONS))
def test_every_mutation_of_the_restatement_changes_a_graph(mut):
    assert set(EXPECTED_TO_CATCH) == set(HG.MUTATIONS)
    assert _differs(EXPECTED_TO_CATCH[mut], mut), (mut, HG.MUTATIONS[mut])
    caught = [n for n in EC.CASES if _differs(n, mut)]
    assert EXPECTED_TO_CATCH[mut] in caught
    if mut == "fma":   # the fused cross product shows on the few-ulp rungs and on nothing else
        assert all(n.startswith(("seg_ulp_", "seg_nearly_parallel_")) for n in caught), caught
        assert any(n.startswith("seg_ulp_") for n in caught), caught
    if mut in ("fwd_lt", "head_lt", "front_le", "dmin_le"):   # the rung-0 case of every ladder of that comparison notices
        ladders = {"fwd_lt": ("fwd_345_0", "fwd_roadmap_0"), "head_lt": ("head_345_0",), "front_le": ("front_ladder_0",),
                   "dmin_le": ("disc_before_keypoint_0", "disc_before_roadmap_0", "disc_radius_rung_0", "lanes_idx63_0", "lanes_idx256_0",
                               "table_m130_p129_tie")}[mut]
        assert set(ladders) <= set(caught), (mut, sorted(set(ladders) - set(caught)))


# ---- the coverage the families claim, from the records ---------------------------------------------------------------------------------------
def _has(rec, kind, cls=None, tie=None, sign=None, outcome=None):
    m = rec[:, 0] == K[kind]
    if cls is not None:
        m &= rec[:, 1] == cls
    if tie is not None:
        m &= rec[:, 4] == tie
    if sign is not None:
        m &= rec[:, 5] == sign
    if outcome is not None:
        m &= rec[:, 3] == outcome
    return int(m.sum())


def test_every_comparison_kind_occurs_as_a_tie_on_both_sides_of_a_rung_and_separated():
    rec = _records(EC.CASES)
    assert set(rec[:, 0].astype(int)) == set(range(len(HG.KINDS)))
    for kind in ("fwd", "head", "front", "dmin", "s_lo"):   # thresholds a rounded quantity can sit on: tie, rung above and below, separated
        assert _has(rec, kind, tie=1) >= 1, kind
        assert _has(rec, kind, HG.RUNG, sign=1) >= 1 and _has(rec, kind, HG.RUNG, sign=-1) >= 1, kind
        assert _has(rec, kind, HG.SEPARATED, outcome=1) >= 1 and _has(rec, kind, HG.SEPARATED, outcome=0) >= 1, kind
    assert _has(rec, "norm0", HG.EXACT, tie=1) >= 1 and _has(rec, "norm0", HG.SEPARATED, outcome=1) >= 1   # a squared norm: zero or positive
    for kind in ("t_lo", "s_hi", "t_hi", "tlo", "thi", "near"):   # exact by construction: tie, and separated either way
        assert _has(rec, kind, HG.EXACT, tie=1) >= 1, kind
        assert _has(rec, kind, HG.SEPARATED, outcome=1) >= 1 and _has(rec, kind, HG.SEPARATED, outcome=0) >= 1, kind
    # denom == 0: exact ties (parallel, collinear, a polygon of one vertex), a zero in fp64 that is none at 80 digits, either sign
    assert _has(rec, "denom0", HG.EXACT, tie=1) >= 3 and _has(rec, "denom0", HG.RUNG, tie=1) >= 1
    assert _has(rec, "denom0", sign=1) >= 1 and _has(rec, "denom0", sign=-1) >= 1
    assert _has(rec, "goal_tol", outcome=1) >= 2 and _has(rec, "goal_tol", outcome=0) >= 1
    assert _has(rec, "draw", outcome=1) >= 1
    # the ladders hold all their rungs, on the side their name says
    for stem, kind in (("fwd_345_", "fwd"), ("fwd_roadmap_", "fwd"), ("head_345_", "head"), ("disc_before_keypoint_", "dmin"),
                       ("disc_before_roadmap_", "dmin")):
        for label in EC.LADDER:
            r = _ref(stem + label)[1].record_array()
            on = r[(r[:, 0] == K[kind]) & (r[:, 1] == HG.RUNG)]
            assert len(on) >= 1, (stem, label)
            # threshold above the quantity for '+' (dot <= thr: no edge; d < min_dist: hit), on it for '0', below for '-'
            assert set(on[:, 5]) == {{"0": 0.0, "+": -1.0, "-": 1.0}[label[0]]}, (stem, label)
    sides = {label: _ref("front_ladder_" + label)[2]["vertices"].shape[0] for label in EC.LADDER}
    assert all(n == (2 if label[0] == "-" else 4) for label, n in sides.items()), sides   # q < 0.1: no key points; the tie keeps them


def test_the_seg_family_holds_every_configuration_in_every_orientation():
    names = [n for n in EC.CASES if n.startswith("seg_") and n[4:].split("_")[0] in EC._SEG]
    assert len(names) == 8 * 4
    hits = {n: int(_ref(n)[2]["adjacency"][0, 1] == 0) for n in names}
    for w in ("parallel", "collinear"):
        assert not any(hits[n] for n in names if "_%s_" % w in n)
    assert all(hits[n] for n in names if "_cross_" in n)
    # a segment that only touches (s or t exactly 0 or 1) is a crossing for one sign of denom and clear for the other: the reference's
    # (s_numer < 0) == (denom > 0) with s_numer = 0
    for w in ("s0", "s1", "t0", "t1", "shared"):
        got = sorted(hits[n] for n in names if "_%s_" % w in n)
        assert got == [0, 0, 1, 1], (w, got)
    rec = _records(names)
    for kind in ("s_lo", "t_lo", "s_hi", "t_hi"):
        assert _has(rec, kind, HG.EXACT, tie=1) >= 2, kind
    assert _has(rec, "denom0", sign=1) >= 8 and _has(rec, "denom0", sign=-1) >= 8
    # missed and made by a few ulp, in fp64 and at 80 digits alike or not: both outcomes on both tags
    for tag in ("pi", "sqrt"):
        out = [int(_ref("seg_ulp_%s_%+d" % (tag, k))[2]["adjacency"][0, 1]) for k in range(-3, 4)]
        assert 0 in out and 1 in out, (tag, out)
    assert _ref("seg_nearly_parallel_2^-30")[2]["adjacency"][0, 1] == 1 and _ref("seg_nearly_parallel_2^-26")[2]["adjacency"][0, 1] == 0
    for n, want in (("seg_triangle_closing_edge_only", 0), ("seg_quad_closing_edge_only", 0), ("seg_triangle_first_edge", 0), ("seg_triangle_clear", 1),
                    ("seg_polygon_one_vertex_on_the_edge", 1), ("seg_polygon_two_vertices", 0), ("seg_polygon_two_vertices_clear", 1)):
        assert _ref(n)[2]["adjacency"][0, 1] == want, n


def test_heads_and_hosts_rules_are_where_the_names_say():
    assert _ref("head_equal_distance")[2]["near"] == (1, 2) and _has(_ref("head_equal_distance")[1].record_array(), "near", HG.EXACT, tie=1) == 1
    assert _ref("head_nearest_second")[2]["near"] == (3, 4)
    assert _ref("head_none_in_front")[2]["near"] == (-1, -1) and len(_ref("head_none_in_front")[2]["vertices"]) == 2
    assert _ref("head_cuts_both_keypoints")[2]["adjacency"][0].tolist() == [0, 0, 0, 1] and _ref("head_disabled_thr0")[2]["adjacency"][0].tolist() == [0, 1, 1, 1]
    assert _ref("head_disabled_thr0")[2]["near"] == (-1, -1) and _has(_ref("head_disabled_thr0")[1].record_array(), "head") == 0
    assert len(_ref("front_on_start")[2]["vertices"]) == 4 and len(_ref("front_abeam")[2]["vertices"]) == 2 and len(_ref("front_behind")[2]["vertices"]) == 2
    V, A = _ref("fwd_coincident_negative")[2]["vertices"], _ref("fwd_coincident_negative")[2]["adjacency"]
    assert np.array_equal(V[1], V[3]) and np.array_equal(V[2], V[4]) and np.array_equal(V[5], V[7])
    assert A[1, 3] == 1 and A[3, 1] == 1 and A[5, 7] == 1       # the zero-length edge passes dot = 0 > thr and no obstacle stops it
    A0 = _ref("fwd_coincident_thr0")[2]["adjacency"]
    assert A0[1, 3] == 0 and A0[3, 1] == 0 and A0[5, 7] == 0    # 0 <= 0


def test_lanes_waves_and_tables_are_where_the_names_say():
    Ns = {len(_ref(n)[2]["vertices"]) for n in EC.CASES if n.startswith("lanes_")}
    assert {2, 8, 9, 16, 17, EC.N23, 24} <= Ns
    assert (EC.N23 - 1) ** 2 <= 2 * EC.K_THREADS < EC.N23 ** 2
    assert len(_ref("lanes_n2_no_obstacle")[0]["obst"].type) == 0
    for which, idx in EC.IDX.items():
        A = {l: _ref("lanes_idx%s_%s" % (which, l))[2]["adjacency"].ravel() for l in EC.SHORT}
        i, j = divmod(idx, EC.N23)
        assert A["+1ulp"][idx] == 0 and A["-1ulp"][idx] == 1 and A["0"][idx] == 1
        assert set(np.flatnonzero(A["+1ulp"] != A["-1ulp"])) <= {idx, j * EC.N23 + i}, which   # this lane (and at most its mirror) decides
        assert A["0"][EC.N23 ** 2 - 1] == 0
    w = EC.wave_survivors(EC.build("lanes_empty_wave_beside_single_lane"))
    assert (0, 0) in w[:EC.FULL_WAVES] and (1, 1) in w[:EC.FULL_WAVES], w
    sizes = collections.defaultdict(set)
    for n in EC.CASES:
        if n.startswith("table_"):
            c, g, r = _ref(n)
            M, pos = int(n.split("_")[1][1:]), int(n.split("_")[2][1:])
            assert len(c["obst"].type) == M and c["rows"][pos] == ("p", 4.0, 0.75)
            assert r["adjacency"][0, 1] == (0 if n.endswith("hit") else 1)
            sizes[M].add(pos)
            if M >= 5:
                assert set(c["obst"].type) == set(range(5))
    assert sorted(sizes) == EC.TABLE_SIZES and all(sizes[M] == {0, M // 2, M - 1} for M in sizes)


def test_the_fleets_hold_what_they_claim():
    k = [_ref(n) for n in EC.FLEETS["fleetk"]]
    assert [len(x[2]["vertices"]) for x in k] == [2, 18, 6, 0] and [len(x[0]["obst"].type) for x in k] == [0, 8, 130, 1]
    r = [_ref(n) for n in EC.FLEETS["fleetr"]]
    assert [len(x[2]["vertices"]) for x in r] == [17, 17, 17, 0]
    for members in (k, r):   # one launch shares the parameters
        for key in ("keypoint", "thr", "dist_to_obst", "no_samples", "area_width", "length_scale", "max_classes", "max_paths"):
            assert len({x[0][key] for x in members}) == 1, key
    # the neighbour's table would change the answer: the same vertices, three different adjacencies
    for a in range(3):
        np.testing.assert_array_equal(r[a][2]["vertices"], r[0][2]["vertices"])
        for b in range(a):
            assert not np.array_equal(r[a][2]["adjacency"], r[b][2]["adjacency"])
    fix = MK.load("fleet")
    raw = np.load(os.path.join(HERE, "golden", MK.STEM + "fleet.npz"))
    for fleet, members in EC.FLEETS.items():
        assert [str(m) for m in raw["fleet_" + fleet]] == members and set(members) <= set(fix)
