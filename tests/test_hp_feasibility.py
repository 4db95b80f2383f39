"""The DECISIONS of the feasibility check - which cell a coordinate falls into, which cells an outline edge reads,
which return code wins, how many additional samples a segment gets, where the look-ahead ends - against an exact restatement, on their
thresholds (CPU side).

tests/hp_feasibility.py restates TebOptimalPlanner::isTrajectoryFeasible with the navigation stack's footprintCost / lineCost /
LineIterator / worldToMap and g2o::normalize_theta as plain loops, evaluated op by op in fp64 and, beside it, with mpmath at 80 digits;
it records EVERY comparison with its relative margin and classifies it as separated (>= 1e-9), exact (fp64 operands equal the 80-digit
ones) or a declared rounded rung (expectation = the op-by-op fp64 outcome); anything else raises, nothing is dropped.
tests/feasibility_threshold_cases.py builds the cases (families cell, codes, raster, interp, look, lanes, fleet, limits - see there).

This file
  - checks on every case: restatement = the reference planner's own function (oracle/_ref, where it can be built; the generator of the
    fixtures refuses a case on which it disagrees, so the committed answer stands in for it elsewhere) = the CPU oracle, and the
    committed fixture equals the recomputed one field by field;
  - checks the rasteriser independently: LineIterator visits the cells of a closed form without loop state for every (dx, dy) in [-9, 9]^2;
  - checks the CASES: the coverage the families claim is asserted from the recorded comparisons and events, not from the names;
  - checks the CHECKER: each mutation of hp_feasibility.MUTATIONS changes the answer of at least one case (printed: which) - except
    four that are proven to change nothing inside the scope and are asserted to change nothing:
      '>=' for '>' in either interpolation trigger: at the tie the triggered branch asks for max(ceil(x <= 1), ..) - 1 samples, i.e. for
        what the untriggered branch gives, unless the OTHER trigger holds - and then both forms enter the branch anyway;
      floor for the truncating cast: they differ only for a negative quotient, which the wx < ox guard excludes (asserted from the
        events: no truncated quotient of any case is negative); without the guard the cast decides, and that mutation is caught;
      the tie deltax == deltay taken y-major: there num = den / 2 < den and numadd = den, the minor coordinate steps with every cell,
        and both readings visit (x0 + k, y0 + k) (asserted for every diagonal of [-9, 9]^2).

Found with it: nothing on the CPU side - the oracle and the reference function take the restatement's decision in every case.
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
import hp_feasibility as HF  # noqa: E402
import feasibility_threshold_cases as FC  # noqa: E402
import make_hp_feasibility as MK  # noqa: E402

from teb_local_planner_amd import _abi  # noqa: E402

_REF, _FIX = {}, {}
K = HF.KIND_ID


def _ref(name):
    """(case, expected per band, records, events) of a case, computed once per session and left unchanged"""
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


def _family(fam):
    return [n for n in FC.CASES if n.split("_")[0] == fam]


def test_the_case_table_covers_every_family_and_the_sources_are_what_the_cases_assume():
    fams = collections.Counter(n.split("_")[0] for n in FC.CASES)
    assert set(fams) == set(FC.FAMILIES), fams
    have = sorted(f for f in os.listdir(os.path.join(HERE, "golden")) if f.startswith(MK.STEM) and f.endswith(".npz"))
    assert have == sorted(stem + ".npz" for stem in MK.groups())
    for f in have:
        assert os.path.getsize(os.path.join(HERE, "golden", f)) < MK.MAX_FILE_BYTES
    assert FC.MAX_POSES == _abi.MAX_POSES
    src = open(os.path.join(os.path.dirname(HERE), "teb_local_planner_amd", "csrc", "teb_feasibility.hpp")).read()
    assert int(re.search(r"constexpr int kFeasThreads = (\d+);", src).group(1)) == HF.LANES
    assert int(re.search(r"constexpr int kMaxFeasFootprint = (\d+);", src).group(1)) == 64 == len(FC.CASES["codes_nf64_free"]["fp"])
    assert set(HF.EQUIVALENT) < set(HF.MUTATIONS)


@pytest.mark.parametrize("name", list(FC.CASES))
def test_restatement_reference_function_oracle_and_fixture_agree(oracle, name):
    c, want, rec, _ = _ref(name)
    assert len(rec) >= 1
    for kind, cls, rel, out, tie, sgn in rec:   # admissible: the restatement raised otherwise; every record says why it is
        assert cls in (HF.SEPARATED, HF.EXACT, HF.RUNG)
        assert cls != HF.SEPARATED or rel >= HF.REL
        assert cls != HF.RUNG or (HF.KINDS[int(kind)] in c["rungs"] and HF.KINDS[int(kind)] not in HF.LIBM_KINDS)
    if len(c["fp"]) >= 3 and any(((b[2] != 0) & ~np.isnan(b[2])).any() for b in c["bands"]):   # an outline through cos / sin: nothing may hang on their last bits
        assert not (rec[:, 1] == HF.RUNG).any()
        on = rec[np.isin(rec[:, 0], (K["trunc"], K["w_lt_o"])) & (rec[:, 2] < HF.REL)]
        assert (on[:, 1] == HF.EXACT).all() and len(on) <= 2 * len(c["bands"]) * 3   # at most the pose centre itself
    fix = _fixture(name)
    recorded = [(bool(ok), int(first)) for ok, first in fix["expected"]]
    ref = _binary()
    assert (MK.others(c, ref) if ref is not None else recorded) == want
    assert MK.others(c, oracle) == want
    new = MK.record(c, want, rec)
    for key in new:
        got, w = fix[key], np.asarray(new[key])
        assert got.dtype == w.dtype and np.array_equal(np.asarray(got).ravel(), w.ravel(), equal_nan=True), (name, key)
    for b, (x, y, th) in enumerate(c["bands"]):
        for got, w in zip(fix["bands"][b], (x, y, th)):
            assert np.array_equal(got, w, equal_nan=True)


@pytest.mark.parametrize("name", MK.CAPACITY)
def test_capacity_cases_are_the_oracles(oracle, name):
    c = MK.capacity_case(name)
    fix = _fixture(name)
    want = MK.others(c, oracle)
    total = 2 ** 22 + (1 if name.endswith("+1") else 0)
    assert want == [(False, total - 1)]               # the last of exactly `total` tests, the only one on a lethal cell
    ref = _binary()
    assert ref is None or MK.others(c, ref) == want
    assert tuple(fix["expected"][0]) == (MK.REFUSED if name.endswith("+1") else (0, total - 1))
    assert np.array_equal(fix["bands"][0][0], c["bands"][0][0]) and np.array_equal(fix["cells"], c["grid"].cells)


def test_line_iterator_visits_the_cells_of_the_closed_form():
    for dx in range(-9, 10):
        for dy in range(-9, 10):
            for x0, y0 in ((0, 0), (11, 7)):
                assert HF.line_cells(x0, x0 + dx, y0, y0 + dy) == HF.line_cells_closed_form(x0, x0 + dx, y0, y0 + dy), (dx, dy)
    for d in range(-9, 10):     # the diagonal tie visits the same cells whichever axis is called major
        for sy in (1, -1):
            assert HF.line_cells(0, d, 0, sy * d, "tie_ymajor") == HF.line_cells(0, d, 0, sy * d) == [(k if d >= 0 else -k, sy * (k if d >= 0 else -k)) for k in range(abs(d) + 1)]
    for dx, dy in FC.DIRECTIONS:   # the stamps of the raster family hold what the closed form says
        c0 = (1 + max(0, -dx), 1 + max(0, -dy))
        E = FC.raster_outline(dx, dy, c0)
        assert E[0] == HF.line_cells_closed_form(c0[0], c0[0] + dx, c0[1], c0[1] + dy)
        assert E[2] == HF.line_cells_closed_form(c0[0] + dx, c0[0], c0[1] + dy, c0[1]) and len(E[1]) == 1
        want = _ref("raster_dir_%+d_%+d" % (dx, dy))[1]
        assert want == [(False, 0)] * (len(want) - 1) + [(True, -1)]


# ---- the checker is checked -------------------------------------------------------------------------------------------------------------------
def _answers(name, mut):
    c = FC.CASES[name]
    return [HF.Check(c, "float", mut).run(b) for b in range(len(c["bands"]))]


def _caught(mut):
    if mut == "fleet_neighbour":   # scene s with the grid of scene s + 1
        out = []
        for members, _ in FC.FLEETS.values():
            for s, name in enumerate(members):
                c, g = FC.CASES[name], FC.CASES[members[(s + 1) % len(members)]]["grid"]
                if [HF.Check(c, "float", None, grid=g).run(0)] != _ref(name)[1]:
                    out.append(name)
        return out
    return [n for n in FC.CASES if _answers(n, mut) != _ref(n)[1]]


EXPECTED_TO_CATCH = {   # mutation -> a case that must notice it (every other case is searched too)
    "w2m_recip": "cell_res0.05_reciprocal_differs", "no_guard": "cell_w_below_o_x", "mx_le_sx": "cell_index_size_x",
    "no_closing": "codes_tri_closing_edge_only", "num_round": "raster_dir_-7_+2",
    "253_lethal": "codes_tri_253_on_the_outline", "255_collision": "codes_tri_255_before_254_on_edge0",
    "offmap_collision": "cell_w_below_o_x", "later_lethal": "codes_tri_254_on_edge1_behind_255_on_edge0",
    "closed_form": "interp_recurrence_not_closed_form", "look_sqrt": "look_hypot_does_not_square_cut_at_0",
    "look_no_override": "look_dist_raises_idx", "lane_min": "lanes_600_tests_one_per_pose",
    "bsearch_off": "lanes_pose_on_a_boundary_after_600_samples", "fleet_neighbour": "fleet_a_scene0"}


@pytest.mark.parametrize("mut", list(HF.MUTATIONS))
def test_every_mutation_of_the_restatement_changes_an_answer(mut):
    assert set(EXPECTED_TO_CATCH) | set(HF.EQUIVALENT) == set(HF.MUTATIONS)
    caught = _caught(mut)
    print("%s (%s): %d cases notice: %s" % (mut, HF.MUTATIONS[mut], len(caught), ", ".join(caught[:12]) + (" ..." if len(caught) > 12 else "")))
    if mut in HF.EQUIVALENT:   # see the docstring: no case inside the scope can notice
        assert caught == [], (mut, caught)
        return
    assert EXPECTED_TO_CATCH[mut] in caught, (mut, HF.MUTATIONS[mut], caught)
    if mut == "fleet_neighbour":   # EVERY scene's neighbour's grid gives another answer
        assert sorted(caught) == sorted(m for members, _ in FC.FLEETS.values() for m in members)
    if mut == "w2m_recip":
        assert all(n.startswith("cell_res") for n in caught), caught


def test_floor_and_the_cast_agree_because_no_truncated_quotient_is_negative():
    for name in FC.CASES:
        c = FC.CASES[name]
        k = HF.Check(c, "float")
        seen = []
        orig = k.to_int
        k.to_int = lambda kind, q, fn, orig=orig, seen=seen: (seen.append(q) if kind == "trunc" else None, orig(kind, q, fn))[1]
        for b in range(len(c["bands"])):
            k.run(b)
        assert all(q != q or q >= 0 for q in seen), name


# ---- the coverage the families claim, from the records ---------------------------------------------------------------------------------------
def _records(names):
    return np.concatenate([_ref(n)[2] for n in names])


def _events(names):
    out = collections.Counter()
    for n in names:
        out += _ref(n)[3]
    return out


def _has(rec, kind, cls=None, tie=None, sign=None, outcome=None, near=None):
    m = rec[:, 0] == K[kind]
    if cls is not None:
        m &= rec[:, 1] == cls
    if tie is not None:
        m &= rec[:, 4] == tie
    if sign is not None:
        m &= rec[:, 5] == sign
    if outcome is not None:
        m &= rec[:, 3] == outcome
    if near is not None:
        m &= (rec[:, 2] < HF.REL) == near
    return int(m.sum())


def test_every_threshold_occurs_as_a_tie_on_both_sides_of_a_rung_and_separated():
    rec = _records(FC.CASES)
    assert set(rec[:, 0].astype(int)) == set(range(len(HF.KINDS)))
    for kind in ("w_lt_o", "rot", "dist", "look"):   # exact operands: the tie, one ulp either way (exact, not a tie, nearer than 1e-9), separated
        assert _has(rec, kind, HF.EXACT, tie=1) >= 1, kind
        assert _has(rec, kind, HF.EXACT, tie=0, sign=1, near=True) >= 1 and _has(rec, kind, HF.EXACT, tie=0, sign=-1, near=True) >= 1, kind
        assert _has(rec, kind, HF.SEPARATED, outcome=1) >= 1 and _has(rec, kind, HF.SEPARATED, outcome=0) >= 1, kind
    assert _has(rec, "look", HF.RUNG) == 0
    for kind in ("trunc", "ceil_rot", "ceil_dist"):  # a quotient against the integers: on one in fp64 (exactly so, and with the exact one beside it), rungs either way
        assert _has(rec, kind, HF.EXACT, tie=1) >= 1, kind
        assert _has(rec, kind, HF.RUNG, tie=1, sign=1) >= 1 and _has(rec, kind, HF.RUNG, tie=1, sign=-1) >= 1, kind
        assert _has(rec, kind, HF.RUNG, tie=0) >= 1, kind
        assert _has(rec, kind, HF.SEPARATED) >= 1, kind
    assert _has(rec, "trunc", HF.RUNG, outcome=1) >= 1 and _has(rec, "ceil_dist", HF.RUNG, outcome=1) >= 1   # rounding changed the integer
    for outcome in (0, 1):
        assert _has(rec, "idx", tie=0, outcome=outcome) >= 1 and _has(rec, "max", tie=0, outcome=outcome) >= 1
    assert _has(rec, "idx", tie=1, outcome=0) >= 2 and _has(rec, "max", tie=1) >= 1          # index == size (x and y); both ceils equal
    for kind, outcomes in (("norm_lo", (0, 1)), ("norm_hi", (0, 1)), ("fix_hi", (0, 1)), ("fix_lo", (0,))):   # after the floor, theta >= 0
        for outcome in outcomes:
            assert _has(rec, kind, outcome=outcome) >= 1, (kind, outcome)
    assert _has(rec, "norm_hi", HF.EXACT, tie=1) >= 1 and _has(rec, "fix_hi", HF.EXACT, tie=1) >= 1 and _has(rec, "norm_lo", HF.EXACT, tie=1) >= 1
    assert _has(rec, "norm_floor") >= 4
    # the ladders hold all their rungs on the side their name says: the parameter above the quantity for '+'
    for stem, kind in (("interp_radius_dnorm/1_", "dist"), ("interp_ang_rot/1_", "rot"), ("look_dist_345_", "look"), ("look_dist_51213_", "look")):
        for label in FC.LADDER:
            r = _ref(stem + label)[2]
            on = r[(r[:, 0] == K[kind]) & (r[:, 2] < HF.REL)]
            assert len(on) >= 1 and set(on[:, 5]) == {{"0": 0.0, "+": -1.0, "-": 1.0}[label[0]]}, (stem, label)
    for div in (1, 2, 3):   # the count of samples steps at the rung, and the index of the first infeasible test shows it
        for stem in ("interp_radius_dnorm/%d_" % div, "interp_ang_rot/%d_" % div):
            firsts = {label: _ref(stem + label)[1][0][1] for label in FC.LADDER}
            assert all(firsts[label] == 2 + div - (0 if label[0] == "-" else 1) for label in firsts if div < 3 or label != "0"), (stem, firsts)


def test_codes_precedence_octants_and_both_verdicts_occur():
    ev = _events(FC.CASES)
    for code in ("code:-1", "code:-2", "code:-3", "code:0"):
        assert ev[code] >= 1, code
    for pair in ("-2_hides_-1_same_edge", "-2_hides_-1_later_edge", "-3_hides_-1_later_edge", "-1_hides_-2_same_edge", "-1_hides_-2_later_edge",
                 "-1_hides_-3_later_edge"):
        assert ev["behind:" + pair] >= 1, (pair, sorted(k for k in ev if k.startswith("behind")))
    for sx in "+-":
        for sy in "+-":
            for major in "xy":
                assert ev["octant:%s%s%s" % (sx, sy, major)] >= 1, (sx, sy, major)
    for what in ("zero", "diagonal", "horizontal", "vertical", "off_by_one", "general", "den_odd", "den_even"):
        assert ev["line:" + what] >= 1, what
    assert ev["max:rot"] >= 1 and ev["max:dist"] >= 1 and ev["max:equal"] >= 1
    assert {"nadd:0", "nadd:1", "nadd:2", "nadd:600"} <= set(ev)
    for fam in FC.FAMILIES:
        verdicts = {ok for n in _family(fam) for ok, _ in _ref(n)[1]}
        assert verdicts == {True, False}, fam
    # the diagonal is x-major: the cells of (5, 5) are those of the closed form, and the y-major reading gives other ones for (6, 5) only
    assert ev["octant:++x"] >= 2
    # the lanes: more tests than lanes, the colliding test where the name says
    lanes = _ref("lanes_600_tests_one_per_pose")[1]
    assert [first for _, first in lanes] == [0, 255, 256, 257, 511, 512, 599, 45, 300, 300, 257, -1]
    assert [first for _, first in _ref("lanes_600_samples_between_segments_with_none")[1]] == [3, 602, 603, 604]
    assert _ref("lanes_n944_one_sample_per_segment")[1] == [(False, 2 * 942)] and _ref("lanes_n944_last_pose")[1] == [(False, 943)]
    n1, k = FC.CASES["interp_recurrence_not_closed_form"]["note"]
    assert _ref("interp_recurrence_not_closed_form")[1] == [(False, k)] and 1 <= k < n1
    # x86's cast of a NaN quotient is an off-map index: the poses behind a NaN pose are still tested
    for what in ("nan_x", "nan_y", "nan_heading"):
        assert _ref("limits_%s_hit_behind_it" % what)[1] == [(False, 4)] and _ref("limits_%s_clear" % what)[1] == [(True, -1)]


def test_the_fleets_hold_what_they_claim():
    raw = np.load(os.path.join(HERE, "golden", MK.STEM + "fleet.npz"))
    for fleet, (members, bands) in FC.FLEETS.items():
        assert [str(m) for m in raw["fleet_" + fleet]] == members and list(raw["fleetbands_" + fleet]) == bands
        cs = [FC.CASES[m] for m in members]
        for key in ("fp", "r", "ang", "look", "dist"):   # one launch shares them
            assert all(c[key] == cs[0][key] for c in cs), key
        assert len({(c["grid"].res, c["grid"].ox, c["grid"].oy, c["grid"].sx, c["grid"].sy) for c in cs}) == len(cs)
        assert len({tuple(_ref(m)[1][0]) for m in members}) == len(members)
    assert sum(b < 0 for _, bands in FC.FLEETS.values() for b in bands) == 1
