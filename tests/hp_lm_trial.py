"""Reference of what one Levenberg-Marquardt iteration does with a solved step: the trial state's chi^2 per category, the gain
ratio rho, the lambda update and the band cost. NOT a test file.

The residuals are those of tests/hp_linearize.py (mpmath, 80 digits): _RESIDUAL, _Graph, _Params, _CATEGORY and the branch-margin
bookkeeping with MARGIN = 1e-7. This module adds only what evaluating chi^2 at a state OTHER than the graph's build state asks for:
  chi2_at     the four category sums at `state` over the edge records of the BUILD state. The time stamps of the dynamic-obstacle edges
              are those accumulated from the build state's time differences (the reference planner fixes them when it adds the edges,
              not per evaluation); every other number of an edge is read at `state`.
  derivatives per category the gradient (central differences of the category sum at 1e-30, over the variables of each edge) and the
              constant S = sum of |entries| of the Hessian of the category sum (second central differences at 1e-20: truncation 1e-40,
              rounding 1e-80 / 1e-40). For any delta, |chi2_k(state + delta) - c_k - g_k . delta| <= 1/2 ||delta||_inf^2 S_k up to third
              order in delta (tests/test_hp_lm_trial.py checks it on seeded perturbations at 80 digits).
No Jacobian formula and no device code enters here.

The fp64 part below the reference (everything the GPU test uses) needs neither mpmath nor the oracle: the corrected categories
c_k + g_k . delta at a state delta away from the fixture's, their tolerances, the cost formula, the interval of rho and of the lambda
an accepted trial leaves. The loop's arithmetic as the reference planner's g2o has it:
  scale  = sum_j dx_j (lambda_k dx_j + b_j)                       (computeScale)
  rho    = (chi2_cur - chi2_trial) / (scale + 1e-3)
  accept (rho > 0): lambda <- lambda_k max(1/3, min(2/3, 1 - (2 rho - 1)^3));  reject: lambda <- lambda ni, ni <- 2 ni
  lambda_0 = 1e-5 max |H_ii| over the free variables, lambda_k = lambda_0 2^(k (k - 1) / 2) for the accepted trial k
  cost   = [sum dt if alt_time] + OBST obst_scale + VIA via_scale + [TIME if not alt_time] + OTHER     (computeCurrentCost)
1 - (2 rho - 1)^3 falls with rho: the factor is 2/3 for rho <= RHO_HI = 0.8467, 1/3 for rho >= RHO_LO = 0.9368, strictly between only
for rho between the two.
"""
import math

import numpy as np

import hp_linearize as hp
from hp_linearize import mpmath, mpf, DPS, MARGIN, CAT_OBST, CAT_VIA, CAT_TIME, CAT_OTHER

EPS = float(np.finfo(np.float64).eps)
CAP = 1e-10            # the second-order part of a category's tolerance may not exceed CAP c_k: a condition on the case, not a tolerance
DECISION_GAP = 1e6     # |chi2_cur - chi2_trial| >= DECISION_GAP eps chi2_cur for every trial: no accept / reject sits on its threshold
H_BOUND = 256 * EPS    # the H bound of tests/test_hp_linearize.py, on the maximal diagonal entry: lambda_0's tolerance
RHO_HI = 0.5 * (1.0 + (1.0 / 3.0) ** (1.0 / 3.0))   # at and below: factor 2/3
RHO_LO = 0.5 * (1.0 + (2.0 / 3.0) ** (1.0 / 3.0))   # at and above: factor 1/3
# the launches every case runs: (obst_scale, via_scale, alt_time). The first four split the categories, the last two are the project's
# defaults and a mixed one, so that nothing is held only through differences
LAUNCHES = ((1.0, 1.0, False), (0.0, 1.0, False), (1.0, 0.0, False), (1.0, 1.0, True), (100.0, 1.0, False), (2.5, 0.25, True))


# ---- the 80-digit reference ------------------------------------------------------------------------------------------------------------
def _m(v):
    return v if isinstance(v, mpmath.mpf) else mpf(float(v))


def chi2_at(cfg, obst, via, batch_build, state, wm, irec, b=0, derivatives=False):
    """The category sums of band b's graph (edge records irec of oracle.edges() at the build state batch_build) at `state` = (x, y,
    theta, dt); entries may be mpf. Returns dict(chi2 [4] mpf, rows [4] residual rows per category, margin, margin_what, n) and with
    derivatives=True also grad [4][4n] mpf and S [4] mpf. A branch margin below MARGIN raises, as in hp_linearize.linearize."""
    with mpmath.workdps(DPS):
        g = hp._Graph(cfg, obst, via, batch_build, b, wm)   # the time stamps of the build state stay in g.stamp
        n, P = g.n, g.P
        x, y, th, dt = state
        assert len(x) == len(y) == len(th) == n and len(dt) >= n - 1
        g.X = [[_m(x[i]), _m(y[i]), _m(th[i]), _m(dt[i]) if i < n - 1 else mpf(0)] for i in range(n)]
        cx = hp._Ctx(False)
        chi2, rows = [mpf(0)] * 4, [0] * 4
        grad = [[mpf(0)] * (4 * n) for _ in range(4)]
        S = [mpf(0)] * 4
        d1, d2 = mpf(10) ** -30, mpf(10) ** -20
        for rec in irec:
            ty, var, fixed, val, aux = g.edge(rec)
            fun, w = hp._RESIDUAL[ty], P.weights[ty]
            cat = hp._CATEGORY.get(ty, CAT_OTHER)
            cx.on = True
            base = fun(cx, P, val, aux)
            cx.on = False
            assert len(base) == len(w) == int(rec[8])
            rows[cat] += len(base)
            f0 = sum(w[k] * e * e for k, (e, side) in enumerate(base))
            chi2[cat] += f0
            if not derivatives or all(wk == 0 for wk in w):
                continue
            free = [q for q in range(len(var)) if not fixed[q]]

            def f(shift):
                v = list(val)
                for q, s in shift:
                    v[q] = v[q] + s
                return sum(w[k] * e * e for k, (e, side) in enumerate(fun(cx, P, v, aux)))

            for i, q in enumerate(free):
                grad[cat][var[q]] += (f([(q, d1)]) - f([(q, -d1)])) / (2 * d1)
                S[cat] += abs(f([(q, d2)]) - 2 * f0 + f([(q, -d2)])) / (d2 * d2)
                for p in free[:i]:
                    mixed = f([(q, d2), (p, d2)]) - f([(q, d2), (p, -d2)]) - f([(q, -d2), (p, d2)]) + f([(q, -d2), (p, -d2)])
                    S[cat] += 2 * abs(mixed) / (4 * d2 * d2)
        if cx.margin < MARGIN:
            raise hp.BranchMarginError("%s: %s < %g" % (cx.what, mpmath.nstr(cx.margin, 5), MARGIN))
        out = dict(chi2=chi2, rows=rows, margin=float(cx.margin), margin_what=cx.what, n=n)
        if derivatives:
            out.update(grad=grad, S=S)
        return out


def free_max_diagonal(R):
    """max |H_ii| over the free variables 3 .. 4 (n - 1) - 1 of a reference linearisation R (hp_linearize.linearize), as a float"""
    n = R["n"]
    return float(max(abs(R["H"].get((r, r), 0)) for r in range(3, 4 * (n - 1))))


def state_plus(state, dx_free, n):
    """the fp64 state after oplus: x += dx, theta = theta + dx (no case lets a heading wrap), dt += dx, each rounded once; dx_free
    runs over the free variables 3 .. 4 (n - 1) - 1 (hp_solve's order)"""
    x, y, th, dt = (np.array(a, dtype=np.float64) for a in state)
    arrs = (x, y, th, dt)
    with mpmath.workdps(DPS):
        for j, d in enumerate(dx_free):
            r = 3 + j
            a = arrs[r & 3]
            a[r >> 2] = float(mpf(float(a[r >> 2])) + mpf(str(d)))
    return x, y, th, dt[:n - 1]


# ---- fp64: what both tests form from a fixture and a launch -------------------------------------------------------------------------------
def flat(state, n):
    """[4n] in the canonical order 4 i + c; the dt slot of the last pose is 0"""
    x, y, th, dt = state
    out = np.zeros(4 * n)
    out[0::4], out[1::4], out[2::4] = np.asarray(x)[:n], np.asarray(y)[:n], np.asarray(th)[:n]
    out[3:4 * (n - 1):4] = np.asarray(dt)[:n - 1]
    return out


def corrected(c, g, S, rows, delta):
    """(c_k + g_k . delta, tolerance (rows_k + 16) eps c_k + 1/2 ||delta||^2 S_k, the second-order part alone) per category"""
    c, S, rows = np.asarray(c, float), np.asarray(S, float), np.asarray(rows, float)
    dmax = float(np.abs(delta).max()) if len(delta) else 0.0
    val = np.array([math.fsum([c[k]] + list(np.asarray(g)[k] * delta)) for k in range(4)])
    second = 0.5 * dmax * dmax * S
    return val, (rows + 16) * EPS * c + second, second


def assert_cap(name, c, second):
    for k in range(4):
        assert second[k] <= CAP * c[k], "%s: state too far from the oracle's (category %d: second-order part %.3g > %g x %.6g)" % (
            name, k, second[k], CAP, c[k])


def cost_of(cats, obst_scale, via_scale, alt_time, sum_dt):
    """computeCurrentCost on four categories (values or tolerances: every coefficient is >= 0)"""
    cst = sum_dt if alt_time else 0.0
    cst += cats[CAT_OBST] * obst_scale
    cst += cats[CAT_VIA] * via_scale
    if not alt_time:
        cst += cats[CAT_TIME]
    cst += cats[CAT_OTHER]
    return cst


def factor(rho):
    return max(1.0 / 3.0, min(2.0 / 3.0, 1.0 - (2.0 * rho - 1.0) ** 3))


def lambda_k_interval(hmax, k):
    """lambda of the accepted trial k from the reference's max |H_ii|: the product kernel forms 1e-5 max|H_ii| from its own H, held to
    H_BOUND on that entry; the doublings are exact"""
    lam = 1e-5 * hmax * float(2 ** ((k - 1) * k // 2))
    return lam * (1 - H_BOUND - 2 * EPS), lam * (1 + H_BOUND + 2 * EPS)


def rho_interval(chi_cur, chi_cur_tol, chi_trial, chi_trial_tol, S0, S1, b0, lam, n):
    """(rho_lo, rho_hi, scale): rho from the reference chi^2 either side (value +- tolerance), dx = S1 - S0 exactly with +- ulp(S1) / 2
    per entry (the rounding of the one addition of the update step), b0 the reference right-hand side at S0, lam = (lo, hi)"""
    f0, f1 = flat(S0, n), flat(S1, n)
    dx = f1 - f0      # (Sterbenz or not: its own rounding is <= ulp(dx) / 2, added to the radius)
    rad = 0.5 * np.spacing(np.abs(f1)) + 0.5 * np.spacing(np.abs(dx))
    fixed = np.ones(4 * n, bool)
    fixed[3:4 * (n - 1)] = False
    assert not dx[fixed].any(), "a fixed variable moved"
    rad[fixed] = 0.0
    lo, hi = [], []
    for L in lam:
        sc = math.fsum(dx * (L * dx + b0))
        r = math.fsum(rad * np.abs(2 * L * dx + b0)) + math.fsum(rad * rad) * L
        lo.append(sc - r); hi.append(sc + r)
    sc_lo, sc_hi = min(lo) + 1e-3, max(hi) + 1e-3
    assert sc_lo > 0, "the scale of the gain ratio is not positive"
    num_lo, num_hi = (chi_cur - chi_cur_tol) - (chi_trial + chi_trial_tol), (chi_cur + chi_cur_tol) - (chi_trial - chi_trial_tol)
    cands = [num_lo / sc_lo, num_lo / sc_hi, num_hi / sc_lo, num_hi / sc_hi]
    return min(cands) * (1 - 4 * EPS * np.sign(min(cands))), max(cands) * (1 + 4 * EPS * np.sign(max(cands))), 0.5 * (sc_lo + sc_hi)


def lambda_after_interval(lam, rho_lo, rho_hi):
    """the image of lambda_k factor(rho): factor falls with rho"""
    return lam[0] * factor(rho_hi) * (1 - 4 * EPS), lam[1] * factor(rho_lo) * (1 + 4 * EPS)


def kind_of(rho_lo, rho_hi):
    """'third' (factor clamped at 1/3), 'two_thirds' (clamped at 2/3), 'between', or None when the interval touches a clamp point"""
    if rho_lo > RHO_LO: return "third"
    if rho_hi < RHO_HI: return "two_thirds"
    if rho_lo > RHO_HI and rho_hi < RHO_LO: return "between"
    return None


def check_launches(name, F, S0, launches, report=print, lam=None, rho_slack=0.0):
    """What the CPU test (the oracle as the device) and the GPU test assert of one case. F: the fixture entries of the case (dict of
    arrays: k, s1, c, g, S, rows, c0, rows0, hmax, b0). S0: the state the last LM iteration started from (x, y, theta, dt).
    launches: {(obst_scale, via_scale, alt_time): dict(after=(x, y, theta, dt), chi2, cost, row=[chi2, lambda, k, n])} for every entry of
    LAUNCHES. lam: (lo, hi) of lambda_k where the reference's max |H_ii| does not apply (a second outer iteration, whose start state is the
    device's own: the caller forms it from the device's H there); rho_slack widens the rho interval (the same cases). Returns the figures."""
    n = int(F["n"])
    first = launches[LAUNCHES[0]]
    S1 = tuple(np.asarray(a, dtype=np.float64) for a in first["after"])
    for key in LAUNCHES:   # only the cost may differ between the launches
        L = launches[key]
        for u, v in zip(L["after"], S1):
            assert np.array_equal(np.asarray(u), v), (name, key, "the band differs between launches")
        assert L["chi2"] == first["chi2"] and np.array_equal(L["row"], first["row"]), (name, key)
    row = first["row"]
    k = int(row[2])
    assert row[2] == k and int(row[3]) == n, row
    assert k == int(F["k"]), "%s: accepted trial %d, the oracle's %d" % (name, k, int(F["k"]))
    assert row[0] == first["chi2"], (name, "log chi2 and results.chi2 differ", row[0], first["chi2"])
    delta = flat(S1, n) - flat(tuple(np.asarray(F["s1"])[q] for q in range(4)), n)
    dmax = float(np.abs(delta).max())
    ref, tol, second = corrected(F["c"], F["g"], F["S"], F["rows"], delta)
    assert_cap(name, np.asarray(F["c"], float), second)
    # ---- chi^2 of the accepted trial: ((c0 + c1) + c2) + c3
    chi_ref = ((ref[0] + ref[1]) + ref[2]) + ref[3]
    chi_tol = float(tol.sum())
    err_chi = abs(first["chi2"] - chi_ref)
    # ---- the cost of every launch against the formula on the corrected reference categories
    dt = np.asarray(S1[3], float)[:n - 1]
    sum_dt = math.fsum(dt)                       # exactly rounded: stands for the sum at 80 digits
    sum_dt_tol = (n + 16) * EPS * sum_dt
    worst_cost, worst_eps = 0.0, 0.0
    costs = {}
    for key in LAUNCHES:
        osc, vsc, alt = key
        want = cost_of(ref, osc, vsc, alt, sum_dt)
        t = cost_of(tol, osc, vsc, alt, sum_dt_tol)
        got = launches[key]["cost"]
        costs[key] = (got, want, t)
        worst_cost = max(worst_cost, abs(got - want) / t if t > 0 else (0.0 if got == want else math.inf))
        worst_eps = max(worst_eps, abs(got - want) / (EPS * want) if want > 0 else 0.0)
    # ---- the categories, recovered from the first four launches (reported; a category that is exactly 0 must be exactly 0)
    ca, cb, cc, cd = (launches[key]["cost"] for key in LAUNCHES[:4])
    rec = np.array([ca - cb, ca - cc, ca - cd + sum_dt, 0.0])
    rec[3] = ca - rec[0] - rec[1] - rec[2]
    cat_err = [abs(rec[q] - ref[q]) / (EPS * ref[q]) if ref[q] != 0 else 0.0 for q in range(4)]
    if F["c"][CAT_OBST] == 0:
        assert ca == cb, (name, "the obstacle category must be exactly 0")
    if F["c"][CAT_VIA] == 0:
        assert ca == cc, (name, "the via-point category must be exactly 0")
    # ---- rho and the lambda the accepted trial leaves
    lam = lambda_k_interval(float(F["hmax"]), k) if lam is None else lam
    c0 = np.asarray(F["c0"], float)
    cur = ((c0[0] + c0[1]) + c0[2]) + c0[3]
    cur_tol = float(((np.asarray(F["rows0"], float) + 16) * EPS * c0).sum())
    rho_lo, rho_hi, scale = rho_interval(cur, cur_tol, chi_ref, chi_tol, S0, S1, np.asarray(F["b0"], float), lam, n)
    rho_lo, rho_hi = rho_lo - rho_slack, rho_hi + rho_slack
    lam_lo, lam_hi = lambda_after_interval(lam, rho_lo, rho_hi)
    fig = dict(k=k, dmax=dmax, chi2=first["chi2"], chi_ref=chi_ref, chi_tol=chi_tol, err_chi=err_chi, worst_cost=worst_cost, worst_eps=worst_eps, cat_err=cat_err,
               rho=(rho_lo, rho_hi), kind=kind_of(rho_lo, rho_hi), lam=lam, lam_after=(lam_lo, lam_hi), lam_got=float(row[1]), scale=scale,
               costs=costs, ref=ref, tol=tol, sum_dt=sum_dt)
    report("%s: k %d |delta| %.2e | chi2 error %.2f of its tolerance (%.1f eps) | worst cost %.2f of its tolerance (%.1f eps) | categories by "
           "difference of costs %s eps | rho [%.12f +- %.1e] %s | lambda %.6e in [%.6e (1 + %.1f eps)]" % (
               name, k, dmax, err_chi / chi_tol, err_chi / (EPS * chi_ref), worst_cost, worst_eps, ["%.1f" % e for e in cat_err], 0.5 * (rho_lo + rho_hi),
               0.5 * (rho_hi - rho_lo), fig["kind"], row[1], lam_lo, (lam_hi / lam_lo - 1) / EPS))
    return fig


def assert_figures(name, fig):
    assert fig["err_chi"] <= fig["chi_tol"], (name, "chi2", fig["chi2"], fig["chi_ref"], fig["err_chi"] / fig["chi_tol"])
    for key, (got, want, t) in fig["costs"].items():
        assert abs(got - want) <= t, (name, "cost of launch", key, got, want, abs(got - want) / t if t else math.inf)
    assert fig["rho"][0] > 0, (name, "the accepted trial's rho", fig["rho"])
    assert fig["lam_after"][0] <= fig["lam_got"] <= fig["lam_after"][1], (name, "lambda after the iteration", fig["lam_got"], fig["lam_after"], fig["rho"])
