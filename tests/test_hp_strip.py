"""The DECISIONS of the band producers and read-outs - which samples a band gets, which are inserted, what is
pruned, where the look-ahead ends, which sign and which branch a velocity takes - against an exact restatement, on their thresholds
(CPU side).

tests/hp_strip.py restates initTrajectoryToGoal x3, PoseSE2::average, updateAndPruneTEB, extractVelocity, getVelocityCommand,
getVelocityProfile, getFullTrajectory, g2o::normalize_theta and g2o::sign as plain loops, evaluated op by op in fp64 and, beside it, with
mpmath at 80 digits; it records EVERY comparison with its site, its relative margin and whether a libm result feeds it, and classifies it
as separated (>= 1e-9), exact (fp64 operands equal the 80-digit ones, or a tie in both evaluations) or a declared rounded rung
(expectation = the op-by-op fp64 outcome; never where libm feeds an operand); anything else raises, nothing is dropped.
tests/strip_threshold_cases.py builds the cases (families line, plan, path, prune, cons, lanes, fleet - see there).

This file
  - checks on every case: "float" = the fp64 half of "both"; restatement = the CPU oracle = the reference planner's own functions
    (oracle/_ref, where it is built and the case is one its code can run: it asserts dt > 0), bit for bit on the outputs no libm result
    feeds and within 1e-13 on the others; the committed fixture equals the recomputed one field by field;
  - checks the CASES: the coverage the families claim is asserted from the recorded comparisons and events, per kind AND site, not
    from the names. What cannot be reached is listed with its reason (UNREACHABLE) and asserted NOT to occur;
  - checks the CHECKER: each mutation of hp_strip.MUTATIONS changes an output of at least one named case (printed: which) - except four
    that are proven to change nothing (hp_strip.EQUIVALENT, reasons there) and are asserted to change nothing.

Found with it: nothing on the CPU side - the oracle and the reference's functions take the restatement's decision in every case. One
limit of the reference itself: updateAndPruneTEB with min_samples 1 can delete up to the last pose and then asks deleteTimeDiffs for one
time difference more than the band has (an assertion in the reference, memory corruption in the oracle's restatement of it); the cases
stay at min_samples >= 2.
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
import hp_strip as HS  # noqa: E402
import strip_threshold_cases as SC  # noqa: E402
import make_hp_strip as MK  # noqa: E402

from teb_local_planner_amd import _abi  # noqa: E402

_REF, _FIX = {}, {}
K, S = HS.KIND_ID, HS.SITE_ID


def _ref(name):
    """(case, expected arrays, records, events) of a case, computed once per session and left unchanged"""
    if name not in _REF:
        _REF[name] = MK.reference(name)
    return _REF[name]


def _fixture(name):
    stem = MK.group_of(name)
    if stem not in _FIX:
        _FIX[stem] = MK.load(stem)
    return _FIX[stem][name]


def _binary():
    from oracle import ref_py
    if os.environ.get("TEB_REF_GOLDEN_ONLY") or not ref_py.available():
        return None
    try:
        ref_py.lib()
    except Exception:
        return None
    return ref_py


def test_the_case_table_covers_every_family_and_the_sources_are_what_the_cases_assume():
    fams = collections.Counter(n.split("_")[0] for n in SC.CASES)
    assert set(fams) == set(SC.FAMILIES), fams
    have = sorted(f for f in os.listdir(os.path.join(HERE, "golden")) if f.startswith(MK.STEM) and f.endswith(".npz"))
    assert have == sorted(stem + ".npz" for stem in MK.groups())
    for f in have:
        assert os.path.getsize(os.path.join(HERE, "golden", f)) < MK.MAX_FILE_BYTES
    assert SC.MAX_POSES == _abi.MAX_POSES
    src = open(os.path.join(os.path.dirname(HERE), "teb_local_planner_amd", "csrc", "teb_device.hpp")).read()
    assert int(re.search(r"#define TEB_AMD_THREADS (\d+)", src).group(1)) == HS.LANES == SC.LANES
    assert set(HS.EQUIVALENT) < set(HS.MUTATIONS) and set(HS.RUNG_KINDS) < set(HS.KINDS) and not set(HS.RUNG_KINDS) & set(HS.LIBM_KINDS)
    sizes = {len(c["band"][0]) for c in SC.CASES.values() if "band" in c} | {len(c["px"]) for c in SC.CASES.values() if "px" in c}
    for n in (HS.LANES - 1, HS.LANES, HS.LANES + 1, SC.MAX_POSES):
        assert n in sizes, n
    for name, c in SC.CASES.items():   # small shapes outside the lanes family
        if not name.startswith("lanes_"):
            assert max(len(c.get("px", ())), len(c.get("band", ((),))[0])) <= 40 and c["cap"] <= 64, name


@pytest.mark.parametrize("name", list(SC.CASES))
def test_restatement_oracle_reference_functions_and_fixture_agree(oracle, name):
    c, want, rec, _ = _ref(name)      # (reference() has asserted: "float" equals the fp64 half of "both"; 1e-13 of the 80-digit values; < 100)
    for kind, cls, rel, out, tie, sgn, site, libm in rec:   # admissible: the restatement raised otherwise; every record says why it is
        assert cls in (HS.SEPARATED, HS.EXACT, HS.RUNG)
        assert cls != HS.SEPARATED or rel >= HS.REL
        if cls == HS.RUNG:
            assert HS.KINDS[int(kind)] in c["rungs"] and HS.KINDS[int(kind)] in HS.RUNG_KINDS and not libm
        assert not (HS.KINDS[int(kind)] in HS.LIBM_KINDS and not libm)
    assert set(c["rungs"]) <= set(HS.RUNG_KINDS)
    for kind in c["rungs"]:           # a declared rung is used
        assert ((rec[:, 0] == K[kind]) & (rec[:, 1] == HS.RUNG)).any(), (name, kind)
    assert MK.check_against(name, c, want, oracle, False) is None
    ref = _binary()
    if ref is not None and c["ref"]:
        assert MK.check_against(name, c, want, ref, True) is None
    fix = _fixture(name)
    new = dict(MK.inputs(c), **want, summary=HS.summary(rec))
    assert set(k for k in fix if len(fix[k])) == set(k for k in new if np.size(new[k])), name
    for key, w in new.items():
        w = np.asarray(w).ravel()
        if len(w):
            assert fix[key].dtype == w.dtype and np.array_equal(fix[key], w, equal_nan=True), (name, key)


# ---- the coverage the families claim, from the records ---------------------------------------------------------------------------------------
SITES_OF = {
    "back": ("line", "plan", "path"), "steps_floor": ("line",), "steps_drop": ("line",), "fill": ("line", "plan", "path"),
    "vel_gt0": ("line", "plan"), "theta_gt0": ("plan",), "dt_max": ("plan",), "acc": ("path",), "ts_le0": ("path",),
    "avg_zero": ("line", "plan", "path"), "look": ("prune",), "near": ("prune",), "la_clamp": ("cmd",), "la_time": ("cmd",), "dt_le0": ("cmd",),
    "dt_eq0": ("cmd", "profile", "traj"), "dir_sign": ("cmd", "profile", "traj"), "holo": ("cmd", "profile", "traj")}
for _k in ("norm_lo", "norm_hi", "norm_floor", "fix_hi", "fix_lo"):
    SITES_OF[_k] = ("line", "plan", "path", "cmd", "profile", "traj")
FLIP = ("line", "path")      # sites whose only normalize_theta call is the flip normalize_theta(yaw + M_PI) with yaw in [-pi, pi]
UNREACHABLE = {}             # (kind, site, outcome) -> why no admissible case can show it
for _s in SITES_OF["avg_zero"]:
    UNREACHABLE[("avg_zero", _s, True)] = ("cos a + cos b == 0 and sin a + sin b == 0 in fp64 needs sin(b) == -sin(a) and cos(b) == -cos(a) bit for bit "
                                           "for b = a +- pi rounded: an accident of libm's last bits, never separated and never exact (sin(M_PI) != 0)")
UNREACHABLE[("dt_eq0", "cmd", True)] = "getVelocityCommand has returned on dt <= 0 before extractVelocity asks dt == 0"
for _s in SITES_OF["fix_lo"]:
    UNREACHABLE[("fix_lo", _s, True)] = "after the floor theta is in [0, 2 pi), and theta - 2 pi of a theta >= pi is exact and >= -pi"
    UNREACHABLE[("norm_floor", _s, True)] = "the outcome of norm_floor is 'rounding changed the integer': no angle of a case sits on a multiple of 2 pi"
for _s in FLIP:
    UNREACHABLE[("norm_lo", _s, False)] = "yaw + M_PI >= 0 for a yaw from atan2"
    UNREACHABLE[("fix_hi", _s, False)] = "the flip leaves the range only for yaw >= 0: the floor is 0 and yaw + M_PI >= pi"
INTEGER_KINDS = ("fill", "look", "la_clamp")
NO_TIE = {("avg_zero", s) for s in SITES_OF["avg_zero"]} | {("dt_eq0", "cmd")} | {("norm_floor", s) for s in SITES_OF["norm_floor"]} \
    | {("norm_lo", s) for s in FLIP + ("cmd",)}      # theta == -pi exactly: reachable only through a difference of headings (plan, profile, traj);
#                                                      the command of the cases takes +pi, and its -pi twin would only repeat the profile's


def _all_records():
    return np.concatenate([_ref(n)[2] for n in SC.CASES if len(_ref(n)[2])])


def _count(rec, kind, site, **kw):
    m = (rec[:, 0] == K[kind]) & (rec[:, 6] == S[site])
    for col, v in (("cls", 1), ("outcome", 3), ("tie", 4)):
        if col in kw:
            m &= rec[:, v] == kw[col]
    return int(m.sum())


def test_every_kind_shows_both_outcomes_a_tie_and_separated_cases_on_each_of_its_sites():
    rec = _all_records()
    seen = {(HS.KINDS[int(k)], HS.SITES[int(s)]) for k, s in set(map(tuple, rec[:, [0, 6]]))}
    assert seen == {(k, s) for k, sites in SITES_OF.items() for s in sites}
    for kind, sites in SITES_OF.items():
        for site in sites:
            for outcome in (True, False):
                n = _count(rec, kind, site, outcome=outcome)
                if (kind, site, outcome) in UNREACHABLE:
                    assert n == 0, (kind, site, outcome, UNREACHABLE[(kind, site, outcome)])
                else:
                    assert n >= 1, (kind, site, outcome)
            if kind in INTEGER_KINDS:
                assert _count(rec, kind, site, cls=HS.EXACT) == _count(rec, kind, site) and _count(rec, kind, site, tie=1) >= 1
                continue
            assert _count(rec, kind, site, cls=HS.SEPARATED) >= 1, (kind, site)
            assert (_count(rec, kind, site, tie=1) >= 1) == ((kind, site) not in NO_TIE), (kind, site)
    for kind in ("steps_floor", "near", "la_time", "acc"):      # the rungs the issue names, and the exact twin of each
        site = SITES_OF[kind][0]
        assert _count(rec, kind, site, cls=HS.RUNG) >= 1 and _count(rec, kind, site, cls=HS.EXACT, tie=1) >= 1, kind
    assert _count(rec, "steps_floor", "line", cls=HS.RUNG, outcome=True) >= 1      # fp64 floors to 3 where the exact quotient is below 3
    assert _count(rec, "near", "prune", cls=HS.RUNG, tie=1) >= 1 and _count(rec, "near", "prune", cls=HS.RUNG, tie=0) >= 1
    assert not ((rec[:, 1] == HS.RUNG) & (rec[:, 7] == 1)).any()                    # nothing hangs on libm's last bits
    for kind in HS.LIBM_KINDS:
        assert not ((rec[:, 0] == K[kind]) & (rec[:, 1] == HS.RUNG)).any()
    fed = rec[(rec[:, 0] == K["dt_max"]) & (rec[:, 7] == 1)]                        # dt_max where a yaw was estimated: separated, or exact
    assert (fed[:, 1] == HS.SEPARATED).sum() >= 1 and np.isin(fed[:, 1], (HS.SEPARATED, HS.EXACT)).all()      # (atan2(0, x) = 0 is)
    for kind in ("back", "dt_max", "acc", "la_time", "dt_le0", "ts_le0"):           # exact operands ON the tie
        assert _count(rec, kind, SITES_OF[kind][0], cls=HS.EXACT, tie=1) >= 1, kind


def test_the_named_quotients_and_sums_round_as_the_cases_say():
    for a, b in ((0.3, 0.1), (0.6, 0.2), (1.2, 0.4)):
        assert a / b == 2.9999999999999996
    assert 0.9 / 0.3 == 3.0 and 2.0 / 0.5 == 4.0 and SC._A / SC._B == 3.0
    t = 0.0
    for _ in range(6):
        t += 0.2
    assert t == 1.2 and 0.1 * 12 == 1.2000000000000002 and not t >= 0.1 * 12
    assert _ref("cons_time_rung_six_times_0.2")[1]["cmd"][3] == 1.0
    for name, n in (("line_quotient_0.3_0.1_below_3", 4), ("line_quotient_0.9_0.3_lands_on_3", 4), ("line_quotient_lands_on_3_from_below", 4),
                    ("line_quotient_2.0_0.5_is_4", 5), ("line_quotient_one_ulp_above_3", 5), ("line_quotient_one_ulp_below_3", 4),
                    ("line_no_steps_1_dropped", 3), ("line_tail_40_inserts", 42), ("path_40_halvings", 42), ("line_capacity_goal_in_the_last_slot", 16)):
        assert int(_ref(name)[1]["n"][0]) == n, name
    th = _ref("line_flip_of_dir_0_wraps_to_minus_pi")[1]["out_th"]
    assert (th[1:-1] == -np.pi).all()
    assert _ref("path_repeated_middle_point")[1]["out_dt"][1] == 0.2 and _ref("path_repeated_middle_point")[1]["out_th"][2] == 0.0
    assert _ref("path_repeated_middle_point_backwards")[1]["out_th"][2] == -np.pi
    assert _ref("path_acc_tie")[1]["out_dt"][0] == 2.0 and _ref("path_acc_tie_on_the_goal_segment")[1]["out_dt"][1] == 2.0
    assert SC.NEAR_RUNG_ULPS >= 1 and int(_ref("prune_rung_pose_1_nearer_exactly_equal_in_fp64")[1]["n"][0]) == 8
    assert int(_ref("prune_equidistant_from_pose_0_and_pose_1")[1]["n"][0]) == 8 and int(_ref("prune_nearer_recedes_nearer_still")[1]["n"][0]) == 8
    for d, left in ((-3, 2), (0, 5), (1, 5), (9, 5), (10, 5), (11, 6)):
        assert int(_ref("prune_n_minus_min_samples_%+d" % d)[1]["n"][0]) == left
    assert list(_ref("cons_dir_0_step_along_y")[1]["cmd"]) == [0.0, 0.0, 0.0, 1.0]      # a command of zero that IS a command
    assert list(_ref("cons_first_time_differences_0_look_2")[1]["cmd"]) == [0.0, 0.0, 0.0, 0.0]
    one = _ref("cons_1_pose")[1]
    assert len(one["profile"]) == 6 and len(one["traj"]) == 0 and list(one["profile"]) == list(SC.VS + SC.VG)
    two = _ref("cons_2_poses")[1]
    assert len(two["profile"]) == 9 and list(two["traj"][3:6]) == list(SC.VS) and list(two["traj"][10:13]) == list(SC.VG)


def test_every_event_occurs_and_every_status_too():
    ev = collections.Counter()
    for n in SC.CASES:
        ev += _ref(n)[3]
    for what in ("insert:line", "insert:plan", "insert:path", "drop", "prune:break", "prune:nearest_at_limit", "prune:to_min_samples", "prune:none",
                 "prune:some", "la:cut_by_time", "la:clamped_above", "la:clamped_below", "refuse:sample", "refuse:insert", "refuse:goal"):
        assert ev[what] >= 1, what
    status = collections.Counter((c["op"], int(_ref(n)[1]["status"][0])) for n, c in SC.CASES.items())
    for op in ("line", "plan", "path"):
        assert status[(op, 0)] >= 1 and status[(op, 1)] >= 2, op      # refused at the goal and at a tail insert
    assert status[("plan", 2)] == status[("path", 2)] == 1
    for op in ("line", "plan", "path"):                                # capacity: the goal in the last slot of a handle of 16
        assert int(_ref("%s_capacity_goal_in_the_last_slot" % op)[1]["n"][0]) == 16 == SC.CASES["%s_capacity_goal_in_the_last_slot" % op]["cap"]


# ---- the checker is checked -------------------------------------------------------------------------------------------------------------------
def _plain(name):
    return {k: v for k, v in _ref(name)[1].items() if not k.startswith("ex_")}


def _notices(name, mut):
    got, _ = MK.outputs(SC.evaluate(SC.CASES[name], "float", mut)[0], False)
    want = _plain(name)
    return got.keys() != want.keys() or any(got[k].shape != want[k].shape or not np.array_equal(got[k], want[k]) for k in got)


EXPECTED_TO_CATCH = {   # mutation -> a case that must notice it (every other case is searched too)
    "back_le": "line_back_tie_goal_straight_left", "steps_round": "line_quotient_2.5", "steps_no_drop": "line_quotient_2.0_0.5_is_4",
    "fill_le": "line_tail_n_is_min_samples_minus_1", "tail_timestep_kept": "line_tail_n_is_min_samples_minus_2", "halve_after": "path_1_halving",
    "dt_min": "plan_dt_max_rotation_wins", "ts_lt0": "path_repeated_middle_point", "look_11": "prune_n_minus_min_samples_+11_pose_11_is_nearest",
    "look_no_min_samples": "prune_n_minus_min_samples_+0", "near_le": "prune_equidistant_from_pose_0_and_pose_1",
    "near_no_break": "prune_nearer_recedes_nearer_still", "shift_dt_off_by_one": "prune_start_only", "goal_at_old_index": "prune_start_and_goal",
    "la_no_lower_clamp": "cons_prevent_2_makes_lim_0", "la_prevent_ignored": "cons_prevent_2_lim_5", "la_time_gt": "cons_time_tie_at_an_earlier_counter",
    "la_time_fixed_count": "cons_time_cut_separated", "dt_lt0": "cons_first_time_differences_0_look_2", "sign_pm": "cons_dir_0_step_along_y",
    "holo_eps": "cons_max_vel_y_1e-300", "omega_unnormalised": "cons_angle_differences_on_every_branch", "traj_end_mean": "cons_2_poses",
    "profile_n": "cons_1_pose", "time_pairwise": "cons_time_rung_six_times_0.2"}


@pytest.mark.parametrize("mut", list(HS.MUTATIONS))
def test_every_mutation_of_the_restatement_changes_an_output_or_is_proven_equivalent(mut):
    assert set(EXPECTED_TO_CATCH) | set(HS.EQUIVALENT) == set(HS.MUTATIONS) and not set(EXPECTED_TO_CATCH) & set(HS.EQUIVALENT)
    caught = [n for n in SC.CASES if _notices(n, mut)]
    print("%s (%s): %d cases notice: %s" % (mut, HS.MUTATIONS[mut], len(caught), ", ".join(caught[:12]) + (" ..." if len(caught) > 12 else "")))
    if mut in HS.EQUIVALENT:   # see hp_strip.EQUIVALENT: no case can notice
        assert caught == [], (mut, caught)
        return
    assert EXPECTED_TO_CATCH[mut] in caught, (mut, HS.MUTATIONS[mut], caught)
    if mut in ("look_11", "la_time_gt", "dt_lt0", "sign_pm", "holo_eps", "near_le", "back_le", "ts_lt0"):   # an error ON a threshold shows only there
        assert len(caught) <= 6, (mut, caught)


def test_the_equivalent_mutations_are_equivalent_for_the_reasons_given():
    assert all(float(np.float32(k)) == float(k) for k in (0, 1, 2, 3, 1000, 2 ** 24 - 1, 2 ** 24)) and float(np.float32(2 ** 24 + 1)) != 2 ** 24 + 1
    for name, c in SC.CASES.items():
        if c["op"] == "prune":      # the search never reaches the last pose
            assert c["min_samples"] >= 2, name
    for name in ("path_acc_tie", "path_acc_tie_on_the_goal_segment"):   # on the tie both branches hold the same number
        rec = _ref(name)[2]
        assert ((rec[:, 0] == K["acc"]) & (rec[:, 4] == 1)).any()


def test_the_fleets_hold_what_they_claim():
    raw = np.load(os.path.join(HERE, "golden", MK.STEM + "fleet.npz"))
    assert {SC.FLEETS[f]["entry"] for f in SC.FLEETS} == {"update_and_prune", "update_and_prune_per_scene", "update_and_prune_per_class", "velocity_commands"}
    for fleet, f in SC.FLEETS.items():
        assert [str(m) for m in raw["fleet_" + fleet]] == f["members"]
        for key, v in f.items():
            if key not in ("members", "entry"):
                assert np.array_equal(raw["fleet_%s_%s" % (fleet, key)], np.array(v)), (fleet, key)
        cs = [SC.CASES[m] for m in f["members"]]
        assert len({c["cap"] for c in cs}) == 1 and len(cs) >= 4
    f = SC.FLEETS["per_class"]
    cs = [SC.CASES[m] for m in f["members"]]
    assert [c["min_samples"] for c in cs] == [f["class_min_samples"][k] for k in f["class_of_scene"]]
    assert sorted(len(c["band"][0]) - c["min_samples"] for c in cs[:2]) == [10, 11]      # one class on the limit of the search, one beyond it
    assert sorted(len(c["band"][0]) - c["min_samples"] for c in cs[2:]) == [9, 10]
    assert int(_ref(f["members"][2])[1]["n"][0]) != int(_ref(f["members"][3])[1]["n"][0])
    cs = [SC.CASES[m] for m in SC.FLEETS["all_bands"]["members"]]
    assert len({(c["new_start"], c["new_goal"], c["min_samples"]) for c in cs}) == 1
    f = SC.FLEETS["commands"]
    cs = [SC.CASES[m] for m in f["members"]]
    assert f["class_max_vel_y"][0] == 0.0 != f["class_max_vel_y"][1] and f["class_dt_ref"][0] != f["class_dt_ref"][1]
    assert [(c["max_vel_y"], c["dt_ref"]) for c in cs] == [(f["class_max_vel_y"][k], f["class_dt_ref"][k]) for k in f["class_of_scene"]]
    assert all((c["look"], c["prevent"]) == (f["look"], f["prevent"]) for c in cs)
    assert len({tuple(_ref(m)[1]["cmd"]) for m in f["members"]}) == len(cs)
