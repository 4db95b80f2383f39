"""What one LM iteration does with its solved step - the trial's chi^2 per category, the gain ratio, the lambda update, the band cost -
against an 80-digit reference (CPU side: the reference itself, the conditions on the cases, and the fp64 oracle held to it).

The linearisation, the damped solve and the association lists each have a high-precision reference (tests/test_hp_linearize.py,
tests/test_hp_solve.py, tests/test_hp_association.py). This family pins what the loop does next. tests/hp_lm_trial.py evaluates the
category sums of the graph built at the start state S0 at ANOTHER state (time stamps of the dynamic-obstacle edges from S0's time
differences, everything else at the new state), with the residuals of tests/hp_linearize.py and its branch margins. A fixture
(tests/golden/make_hp_lm_trial.py) holds, at the oracle's state S1 after one iteration, the categories c_k, their gradient g_k and the
second-order constant S_k (sum of |Hessian entries|), so that a test on a machine without mpmath compares the device's numbers at ITS
state S1 + delta with c_k + g_k . delta, tolerance (rows_k + 16) eps c_k + 1/2 ||delta||^2 S_k; the second part may not exceed
1e-10 c_k (a case beyond that fails, "state too far from the oracle's").

Observed through the launches of hp_lm_trial.LAUNCHES, (obst_scale, via_scale, alt_time) = (1,1,F) (0,1,F) (1,0,F) (1,1,T) (100,1,F)
(2.5,0.25,T): the band, chi2 and the log row are bit-equal across them, the log's chi2 is results.chi2, chi2 = ((c0 + c1) + c2) + c3,
every launch's cost is the formula on the corrected reference categories (tolerances combined with the same scales, sum dt exactly
rounded from the downloaded dt within (n + 16) eps), a category whose reference is 0 is exactly 0, k is the oracle's, and lambda
after the iteration lies in the interval image of lambda_k max(1/3, min(2/3, 1 - (2 rho - 1)^3)): lambda_k from the reference's
max |H_ii| (256 eps, the H bound of tests/test_hp_linearize.py), rho from the reference chi^2 at S0, the corrected chi^2 at S1 and the
scale sum dx (lambda_k dx + b) with dx = S1 - S0 +- ulp / 2 per entry and b the reference right-hand side at S0.

Per scene this file asserts
  - the fixture is what the reference gives today, bit for bit, and the hashes of the scene and the edge list (gradient and S_k are
    recomputed for n <= 65; for every scene they are checked on seeded perturbations at 80 digits, of the size of the solve's forward
    bound and of 1e-6, where the second-order part dominates every rounding);
  - branch margins >= 1e-7 at S0, at S1 and at the state of every damping trial;
  - every trial j < k is rejected and trial k accepted BY THE REFERENCE (states S0 + the 60-digit step of tests/hp_solve.py), with
    |chi2_cur - chi2_trial| >= 1e6 eps chi2_cur: no decision sits on its threshold; k >= 2 / >= 3 where a scene is there for it;
  - the cap 1/2 Delta^2 S_k <= 1e-10 c_k for Delta = max(256 eps kappa, 16 fwd_cpu) ||step||_inf, the forward bound that
    tests/test_hp_solve.py grants the solve on the scene;
  - which piece of the lambda factor the scene lands on (hp_lm_trial_cases.KIND), the rho interval clear of the clamp points;
  - the fp64 oracle's own chi2, costs, k and lambda meet the tolerances (delta = 0: only the rounding part applies);
and four deliberately wrong restatements are caught: the obstacle category counted as OTHER, one pose's cos taken at the old heading,
the lambda factor without its upper clamp, the scale without its 1e-3.

The issue's remark that the factor is strictly between the clamps for rho in (0, 0.153) does not hold: 1 - (2 rho - 1)^3 > 4/3 there
and the upper clamp gives 2/3. Strictly between needs rho in (0.8467, 0.9368): 18 of the 35 scenes; clamped at 1/3: 5; at 2/3: 12.

Two outer iterations (n = 17, point and polygon footprint, dynamic obstacles taken as static): the fixture is of the SECOND iteration,
built at the oracle's state after the first. The device builds that graph at its own state, d1 away (<= D1_MAX = 1e-8, above the first
solve's forward bound of 1.4e-9 / 1.1e-10): the CPU asserts that every association decision there is >= 1e-7 relative from its
threshold and that |d rho / d start| <= SENS_MAX = 1e3 in the 1-norm, from (2 |b0| + |2 lambda dx + b0| + |H| |dx|) (1 + chi2 / scale)
/ scale on the reference's H and b (observed 575 and 787); the GPU test widens rho by SENS_MAX d1 and takes lambda_k from the device's
own H at that state.

Observed on the CPU: half-width of the rho interval 8e-15 (n = 3) .. 8.3e-13 (n = 513), almost all of it the +- ulp / 2 of dx; the
interval of lambda after the iteration is 524 eps wide relative (the H bound either side) and up to 1.7e4 eps (3.9e-12) where the
factor is strictly between (n = 256). The oracle's chi2 is within 0.12 of its tolerance (<= 3.1 eps), its costs within 0.18 (<= 4.0
eps). The cap at the solve's forward bound is used to 0.18 at most (n = 238; Delta up to 1.5e-10).

Out of scope: the loop's terminations (ten rejections, rho == 0, non-finite lambda) cannot be reached from a scene without sitting on
a rounding; the categories of a rejected LAST trial are not observable (inner = 1 always ends on an accepted one here); the
numeric-Jacobian mode does not enter evaluate (its step differs, so its categories are those of another state: no bit-equal run).
Measured run time of this file: 109 s on one core (35 scenes; the generator takes 4.5 min).
"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import hp_linearize as hp  # noqa: E402
import hp_solve as HS  # noqa: E402
import hp_association as HA  # noqa: E402
import hp_lm_trial as LT  # noqa: E402
import hp_lm_trial_cases as TC  # noqa: E402
import make_hp_lm_trial as MK  # noqa: E402

EPS = LT.EPS
mpmath, mpf = hp.mpmath, hp.mpf


def oracle_launches(oracle, c):
    """the launches of LT.LAUNCHES with the CPU oracle as the device"""
    L = {}
    for key in LT.LAUNCHES:
        out, res, tr = oracle.optimize_batch(c["cfg"], c["obst"], c["via"], c["batch"], inner=1, outer=c["outer"], compute_cost=True,
                                             obst_cost_scale=key[0], viapoint_cost_scale=key[1], alternative_time_cost=key[2], trace=True)
        assert len(tr[0]) == c["outer"]
        L[key] = dict(after=out.get_teb(0), chi2=float(res.chi2[0]), cost=float(res.cost[0]), row=tr[0][-1].copy())
    return L


def quiet(*a):
    pass


def test_the_case_table_is_the_one_the_issue_sets():
    assert TC.SIZES == (3, 5, 64, 65, 238, 255, 256, 257, 258, 337, 338, 513)
    for n in TC.SIZES:
        runs = {layout for (scene, layout, opt) in TC.RUNS.values() if scene == "n%d" % n}
        want = {lay for lay in TC.LAYOUTS if n <= TC.CAPACITY[lay]} if n != 513 else {"bandg"}
        assert runs == want | ({"auto"} if n <= TC.SHORT else set()), (n, runs)
    assert set(TC.KIND) == set(TC.SCENES) and {"third", "two_thirds", "between"} == set(TC.KIND.values())
    assert set(TC.FAMILY_ACTIVE) == set(TC.FAMILIES)
    for fam in TC.FAMILIES:
        assert TC.SCENES[fam]["n"] <= 33 and fam in TC.RUNS
    for layout in TC.LAYOUTS:
        assert any(TC.REJECTED_LAYOUT[s] == layout and TC.MIN_K[s] >= 2 for s in TC.REJECTED)
    assert any(k >= 3 for k in TC.MIN_K.values())
    for run, (scene, layout, opt) in TC.RUNS.items():
        o = TC.options(run)
        assert scene in TC.SCENES
        if run in TC.HELPERS:   # one rejected case per LDS layout with solver helpers, as hp_solve_cases.HELPERS
            assert (o.multi_cu, o.speculative_trials) == (0, 3) and layout == TC.HELPERS[run][0] and TC.MIN_K[scene] >= 2
        else:
            assert o.multi_cu == -1 and o.speculative_trials == -1
    assert {TC.HELPERS[r][0] for r in TC.HELPERS} == {"cr", "band"}
    assert [TC.SCENES[s]["n"] for s in TC.RAGGED] == [3, 17, 65] and [TC.SCENES[s]["n"] for s in TC.FLEET] == [3, 17, 65]
    assert all(TC.SCENES[s].get("outer") == 2 and TC.SCENES[s]["n"] == 17 for s in TC.OUTER2) and any("footprint" in kw for kw, seed in TC.OUTER2.values())
    have = sorted(f for f in os.listdir(os.path.join(HERE, "golden")) if f.startswith("hp_lm_trial_") and f.endswith(".npz"))
    assert have == sorted(stem + ".npz" for stem in MK.groups())
    for f in have:
        assert os.path.getsize(os.path.join(HERE, "golden", f)) < MK.MAX_FILE_BYTES


def _perturbed(S1, d, n):
    """S1 + d exactly, as mpf"""
    f1 = LT.flat(tuple(S1), n)
    with mpmath.workdps(hp.DPS):
        v = [mpf(float(a)) + mpf(float(b)) for a, b in zip(f1, d)]
    return v[0::4], v[1::4], v[2::4], v[3::4]


@pytest.mark.parametrize("name", list(TC.SCENES))
def test_reference_conditions_and_the_oracle_as_the_device(oracle, name):
    F = MK.load(name)
    n = TC.SCENES[name]["n"]
    short = n <= TC.SHORT
    c, rec = MK.reference_record(name, oracle, derivatives=short)
    cfg, obst, via, batch = c["cfg"], c["obst"], c["via"], c["batch"]
    # ---- the fixture is today's reference; it holds only numbers and two hashes
    assert set(F) == {key[len(name) + 1:] for key in rec} | {"g", "S"}
    for key, v in rec.items():
        assert np.array_equal(F[key[len(name) + 1:]], v), key
    assert str(F["scene"]) == hp.input_hash(cfg, obst, via, batch, 0) and str(F["edges"]) == hp.edges_hash(c["irec"])
    k = int(F["k"])
    for ename, r in TC.FAMILY_ACTIVE.get(name, ()):   # the family's own rows are in the graph and alive
        assert c["row_kinds"][(hp.EDGE_NAMES.index(ename), r)][1] > 0, (name, ename, r)
    if name == "plain_obstacle_edge":
        assert (hp.E_INFL, 0) not in c["row_kinds"]
    # ---- margins, the decisions of every trial, the trial counts
    assert F["margins"].min() >= hp.MARGIN
    cur = float(F["c0"].sum())
    assert len(F["trials"]) == k >= TC.MIN_K.get(name, 1)
    for j, chi in enumerate(F["trials"]):
        assert abs(cur - chi) >= LT.DECISION_GAP * EPS * cur
        assert (chi < cur) == (j == k - 1), (name, "trial", j + 1, chi, cur)
    # ---- the cap, for delta up to the forward bound tests/test_hp_solve.py grants the solve on this scene
    start, wm, outer = c["start"], c["wm"], c["outer"]
    A = oracle.linearize(cfg, obst, via, start, 0, wm)
    G = HS.check(hp.band_of_dense(A["H"]), A["b"], n, k, start.get_teb(0), c["oracle_out"].get_teb(0))
    Delta = G["bound_fwd"] * float(max(abs(v) for v in G["dx_hp"]))
    slack = 0.0
    if outer == 2:   # the first iteration's forward bound comes on top; the device's start state is its own
        A1 = oracle.linearize(cfg, obst, via, batch, 0, 1.0)
        row1 = oracle.optimize_batch(cfg, obst, via, batch, inner=1, outer=1, trace=True)[2][0][0]
        G1 = HS.check(hp.band_of_dense(A1["H"]), A1["b"], n, int(row1[2]), batch.get_teb(0), start.get_teb(0))
        Delta1 = G1["bound_fwd"] * float(max(abs(v) for v in G1["dx_hp"]))
        assert Delta1 <= TC.D1_MAX
        Delta += Delta1
        # the second graph is built at the device's own state: the same edges there (every association decision is >= 1e-7 relative
        # from its threshold, hp_association.Reference raises below 1e-9), and rho moves by at most SENS_MAX per unit of start state
        ref = HA.Reference(cfg, obst, via, start)
        ref.associate()
        assert ref.summary()[3] >= 1e-7, ref.summary()
        lam_k = 1e-5 * float(F["hmax"]) * 2.0 ** ((k - 1) * k // 2)
        dx = LT.flat(c["oracle_out"].get_teb(0), n) - LT.flat(start.get_teb(0), n)
        Hd = np.zeros(4 * n)
        for d in range(hp.BAND + 1):   # |H| |dx| over the band
            Hd[d:] += np.abs(c["Hband"][d:, d]) * np.abs(dx[:4 * n - d])
            if d:
                Hd[:4 * n - d] += np.abs(c["Hband"][d:, d]) * np.abs(dx[d:])
        scale = float(np.sum(dx * (lam_k * dx + F["b0"]))) + 1e-3
        sens = (2 * np.abs(F["b0"]).sum() + np.abs(2 * lam_k * dx + F["b0"]).sum() + Hd.sum()) * (1 + cur / scale) / scale
        print("%s: first-iteration forward bound %.2e, d rho / d start <= %.3g" % (name, Delta1, sens))
        assert sens <= TC.SENS_MAX
        slack = TC.RHO_SLACK_MAX
    second = 0.5 * Delta * Delta * F["S"]
    LT.assert_cap(name, F["c"], second)
    assert max(np.abs(batch.theta[0, :n]).max(), np.abs(c["oracle_out"].theta[0, :n]).max()) <= TC.SC.MAX_THETA
    # ---- g and S on seeded perturbations at 80 digits
    rng = np.random.default_rng(7 + n)
    S1 = F["s1"]
    for size in (Delta, 1e-6):
        d = rng.uniform(-size, size, 4 * n)
        d[:3] = 0; d[4 * (n - 1):] = 0
        T = LT.chi2_at(cfg, obst, via, start, _perturbed(S1, d, n), wm, c["irec"])
        with mpmath.workdps(hp.DPS):
            for q in range(4):
                lin = mpf(float(F["c"][q])) + sum(mpf(float(a)) * mpf(float(b)) for a, b in zip(F["g"][q], d))
                rounding = EPS * (float(F["c"][q]) + float(np.abs(F["g"][q] * d).sum()))   # c and g are rounded to fp64 in the fixture
                bound = 0.5 * float(np.abs(d).max()) ** 2 * float(F["S"][q])
                assert abs(T["chi2"][q] - lin) <= bound + rounding, (name, q, size, float(abs(T["chi2"][q] - lin)), bound, rounding)
                if size == 1e-6 and F["S"][q] > 0:
                    assert bound > 100 * rounding   # at this size the check is about S, not about roundings
    # ---- the fp64 oracle against the reference (delta = 0)
    L = oracle_launches(oracle, c)
    fig = LT.check_launches(name, F, start.get_teb(0), L)
    assert fig["dmax"] == 0.0
    LT.assert_figures(name, fig)
    if slack:   # the kind must hold for every start state the device may have
        assert LT.check_launches(name, F, start.get_teb(0), L, report=quiet, rho_slack=slack)["kind"] == TC.KIND[name]
    assert fig["kind"] == TC.KIND[name], (name, fig["kind"], fig["rho"])
    print("%s: cap %.2e of 1e-10 c_k at Delta %.2e | rho half-width %.1e | lambda interval %.0f eps wide" % (
        name, float((second / np.where(F["c"] > 0, F["c"], np.inf)).max()) / LT.CAP, Delta, 0.5 * (fig["rho"][1] - fig["rho"][0]),
        (fig["lam_after"][1] / fig["lam_after"][0] - 1) / EPS))


# ---- deliberately wrong restatements --------------------------------------------------------------------------------------------------------
def _case(oracle, name):
    F = MK.load(name)
    c = TC.build(name)
    c["irec"] = oracle.edges(c["cfg"], c["obst"], c["via"], c["batch"], 0, 1.0)[0]
    return F, c, oracle_launches(oracle, c)


def _fails(name, F, c, L):
    with pytest.raises(AssertionError):
        LT.assert_figures(name, LT.check_launches(name, F, c["batch"].get_teb(0), L, report=quiet))


def _restated(L, cats):
    """launches whose chi2 and costs are restated from four categories (the band and the lambda stay)"""
    S1 = L[LT.LAUNCHES[0]]["after"]
    sum_dt = float(np.sum(S1[3]))
    out = {}
    chi = ((cats[0] + cats[1]) + cats[2]) + cats[3]
    for key, v in L.items():
        row = v["row"].copy()
        row[0] = chi
        out[key] = dict(v, chi2=chi, cost=LT.cost_of(cats, key[0], key[1], key[2], sum_dt), row=row)
    return out


def test_a_category_counted_in_another_is_caught(oracle):
    name = "shortest_path_velocity_obstacle_ratio"
    F, c, L = _case(oracle, name)
    good = [float(v) for v in F["c"]]
    LT.assert_figures(name, LT.check_launches(name, F, c["batch"].get_teb(0), _restated(L, good), report=quiet))   # the restatement itself passes
    wrong = [0.0, good[1], good[2], good[3] + good[0]]     # obstacle rows counted as OTHER: chi2 is unchanged, the scaled costs are not
    _fails(name, F, c, _restated(L, wrong))
    wrong = [good[0], good[1], 0.0, good[3] + good[2]]     # the time-optimal rows counted as OTHER: only alt_time sees it
    _fails(name, F, c, _restated(L, wrong))


def test_one_cos_at_the_old_heading_is_caught(oracle, monkeypatch):
    name = "n17"
    F, c, L = _case(oracle, name)
    i = 1 + int(np.abs(F["s1"][2][1:-1] - F["s0"][2][1:-1]).argmax())
    old, new = mpf(float(F["s0"][2][i])), mpf(float(F["s1"][2][i]))
    real = mpmath.cos
    monkeypatch.setattr(mpmath, "cos", lambda t: real(old) if t == new else real(t))   # the trig cache of pose i left stale
    T = LT.chi2_at(c["cfg"], c["obst"], c["via"], c["batch"], tuple(F["s1"]), 1.0, c["irec"])
    monkeypatch.undo()
    stale = [float(v) for v in T["chi2"]]
    assert stale != [float(v) for v in F["c"]]
    _fails(name, F, c, _restated(L, stale))


def _with_lambda(L, lam):
    out = {}
    for key, v in L.items():
        row = v["row"].copy()
        row[1] = lam
        out[key] = dict(v, row=row)
    return out


def test_the_lambda_factor_without_its_upper_clamp_is_caught(oracle):
    name = "prefer_rotdir"
    assert TC.KIND[name] == "two_thirds"
    F, c, L = _case(oracle, name)
    fig = LT.check_launches(name, F, c["batch"].get_teb(0), L, report=quiet)
    LT.assert_figures(name, fig)
    rho = 0.5 * (fig["rho"][0] + fig["rho"][1])
    lam_k = 0.5 * (fig["lam"][0] + fig["lam"][1])
    _fails(name, F, c, _with_lambda(L, lam_k * max(1.0 / 3.0, 1.0 - (2.0 * rho - 1.0) ** 3)))


def test_the_scale_without_its_1e_3_is_caught(oracle):
    name = "n17"
    assert TC.KIND[name] == "between"
    F, c, L = _case(oracle, name)
    fig = LT.check_launches(name, F, c["batch"].get_teb(0), L, report=quiet)
    rho = 0.5 * (fig["rho"][0] + fig["rho"][1])
    lam_k = 0.5 * (fig["lam"][0] + fig["lam"][1])
    LT.assert_figures(name, LT.check_launches(name, F, c["batch"].get_teb(0), _with_lambda(L, lam_k * LT.factor(rho)), report=quiet))
    wrong = rho * fig["scale"] / (fig["scale"] - 1e-3)      # fig["scale"] includes the 1e-3
    _fails(name, F, c, _with_lambda(L, lam_k * LT.factor(wrong)))
