"""The LM step of the damped solve against a 60-digit reference (CPU side: the checker itself, and the whole pipeline with the oracle
standing in for the device).

Between the linearisation (pinned to an 80-digit reference, tests/test_hp_linearize.py) and the plain accept / reject arithmetic lies
the damped solve, seen so far only through 1e-8 m after 20 self-correcting LM iterations. tests/test_gpu_hp_solve.py recovers the
product kernel's own step of ONE iteration from hooks that exist (debug_linearize for H and b, the iteration log for the trial count
k, the band either side of the iteration) and holds it to tests/hp_solve.py: lambda_k rebuilt exactly from H, A = H[free, free] +
lambda_k I solved by a banded LDL^T in decimal at 60 digits, row-wise backward error omega and forward error with the rounding of the
state update (ulp(state) / 2 per variable) taken off. This file
  - checks the checker on random SPD banded systems at every pose count of the cases, diagonals spanning 1 .. 1e6: numpy.linalg.solve
    passes at the FLOOR alone (omega <= 256 eps, forward <= 256 eps kappa), the 60-digit solution gives omega = 0 (< 1e-50), and four
    mutations of it FAIL the omega bound: one component off by 1e-11 relative (the largest of each variable kind), lambda off by a
    factor 2, one off-diagonal block entry of A dropped, the system solved with the fixed variables' rows and columns left in;
  - runs every case of tests/hp_solve_cases.py through the code path of the GPU test with oracle.linearize / oracle.optimize_batch
    (inner = outer = 1, trace) as the device: the lambda_k reconstruction (lambda after the iteration / lambda_k must lie in [1/3, 2/3],
    the accepted trial's scale factor), the free mask, the update, the noise model;
  - asserts the conditions on the inputs: the one iteration ends with an accepted trial (no case is skipped), k >= 2 where a case is
    there for a rejected first trial, no heading near +- pi, no fixed variable moves, obstacle rows active, and the noise term
    (|A| noise)_i <= 64 eps ((|A| |step|)_i + |b_i|) on every free row.
Bounds (both tests): omega <= max(256 eps, 16 omega_cpu), forward <= max(256 eps kappa, 16 fwd_cpu), omega_cpu / fwd_cpu = what
numpy.linalg.solve achieves on the same A, b under the same metric, kappa = ||A||_inf ||A^-1||_inf from the 60-digit factorisation
(Hager's estimate, a lower bound: strict side). 256 eps is the floor of tests/test_hp_linearize.py; 16: cyclic reduction reorders the
elimination over log2(n / 2) levels under FMA contraction - as backward-stable as Cholesky on SPD systems, not equal to it.

Observed with the oracle as the device (fp64 banded Cholesky), over all 42 cases: omega <= 0.5 eps; LAPACK's LU on the same systems
0.3 .. 156 eps row-wise (it pivots across the weight scales 1 .. 1000), so the omega bound is 256 .. 2490 eps; forward error <= 4.9e3
eps at kappa 7e2 .. 5.8e5; noise share <= 43 eps; k between 1 and 5. A step wrong at 1e-10 relative is 4.5e5 eps.
Measured run time of this file: 35 s on one core (decimal: 0.4 s to factor and solve the 944-pose system, 3 s for all of its checks,
5 s for the checker's mutations at that size).
"""
import os
import sys
from decimal import Decimal, localcontext

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import hp_linearize as hp  # noqa: E402
import hp_solve as HS  # noqa: E402
import hp_solve_cases as SC  # noqa: E402

EPS = HS.EPS
NOISE_SHARE = 64 * EPS
SIZES = sorted({n for sizes in SC.SIZES.values() for n in sizes})


# ---- the checker against known solves -------------------------------------------------------------------------------------------------
def random_system(n, seed):
    """SPD banded H over all 4 n variables (lower band) and b: diagonal D = 10^U(0, 6) per variable, off-diagonals of at most
    0.04 min(D_i, D_j) (20 per row: strictly diagonally dominant by rows and columns, so LAPACK's partial pivoting exchanges no row and
    its row-wise error is that of a Cholesky; with couplings ~ sqrt(D_i D_j) it pivots across the scales and reaches 2000 eps row-wise)"""
    rng = np.random.default_rng(seed)
    N = 4 * n
    D = 10.0 ** rng.uniform(0.0, 6.0, N)
    D[N - 1] = 0.0   # there is no dt behind the last pose
    Hb = np.zeros((N, hp.BAND + 1))
    Hb[:, 0] = D
    for d in range(1, hp.BAND + 1):
        Hb[d:, d] = rng.uniform(-0.04, 0.04, N - d) * np.minimum(D[d:], D[:N - d])
    return Hb, rng.uniform(-1.0, 1.0, N) * np.sqrt(D)


@pytest.mark.parametrize("n", SIZES)
def test_checker_on_random_banded_systems(n):
    Hb, b = random_system(n, 7000 + n)
    lam, dx, S = HS.reference_step(Hb, b, n, 1, system=True)
    N = S.N
    zero = [Decimal(0)] * N
    omega = lambda x: float(HS.backward_error(Hb, b, n, lam, x, zero, S).max())
    assert omega(dx) < 1e-50
    bo, bf, ocpu, fcpu, kappa = HS.bounds(Hb, b, n, lam, dx, S)
    print("n %d: LAPACK omega %.2f eps, forward %.1f eps, kappa %.3g" % (n, ocpu / EPS, fcpu / EPS, kappa))
    assert ocpu <= HS.FLOOR and fcpu <= HS.FLOOR * kappa     # the fp64 solve passes at the floor alone
    # 1. one component off by 1e-11 relative: the largest of each variable kind
    for kd in HS.KINDS:
        j = max((q for q in range(N) if HS.kind_of(3 + q) == kd), key=lambda q: abs(dx[q]))
        x = list(dx)
        x[j] = x[j] * (1 + Decimal("1e-11"))
        assert omega(x) > bo, (kd, omega(x) / EPS)
    # 2. lambda off by one factor of 2, either way
    for f in (2.0, 0.5):
        assert omega(HS.System(Hb, b, n, lam * f).solve()) > bo
    # 3. one off-diagonal block entry dropped: the largest coupling of a middle pose to the pose before it
    a = 4 * (n // 2) - 3   # x of pose n / 2 among the free variables
    cands = [(a + q, a + q - d) for q in range(3) for d in range(1, hp.BAND + 1) if a + q < N and a + q - d >= 0 and ((3 + a + q) >> 2) != ((3 + a + q - d) >> 2)]
    r, c = max(cands, key=lambda rc: abs(Hb[3 + rc[0], rc[0] - rc[1]]))
    assert omega(HS.System(Hb, b, n, lam, drop=(r, c)).solve()) > bo
    # 4. the full system, fixed variables included
    full = HS.System(Hb, b, n, lam, full=True).solve()
    assert omega(full[3:4 * (n - 1)]) > bo


def test_recovered_step_refuses_what_it_cannot_recover():
    n = 5
    x = np.linspace(-0.2, 0.2, n); y = np.zeros(n); th = np.array([0.0, 0.1, 3.0, 0.2, 0.0]); dt = np.full(n - 1, 0.25)
    step, noise = HS.recovered_step((x, y, th, dt), (x + np.r_[0, 0.01, 0.02, 0.03, 0], y, th, dt + 0.5), n)
    assert len(step) == 4 * n - 7 and step[0] == Decimal(0.75) - Decimal(0.25) and float(noise[0]) == np.spacing(0.75) / 2
    with localcontext() as ctx:
        ctx.prec = HS.DIGITS
        assert step[1] == Decimal(float(x[1] + 0.01)) - Decimal(float(x[1]))      # exact differences of the fp64 states
    with pytest.raises(ValueError, match="fixed variable"):
        HS.recovered_step((x, y, th, dt), (x + np.r_[1e-9, 0, 0, 0, 0], y, th, dt), n)
    with pytest.raises(ValueError, match="fixed variable"):
        HS.recovered_step((x, y, th, dt), (x, y, th + np.r_[0, 0, 0, 0, 1e-12], dt), n)
    wrapped = th.copy(); wrapped[2] = 3.0 + 0.2 - 2 * np.pi
    with pytest.raises(ValueError, match="wrapped"):
        HS.recovered_step((x, y, th, dt), (x, y, wrapped, dt), n)


def test_lambda_of_the_accepted_trial():
    Hb = np.zeros((20, hp.BAND + 1))
    Hb[:, 0] = [9e9, 9e9, 9e9, 1.0, 2.0, 3.0, 7.0, 5.0, 1.0, 1.0, 1.0, 6.5, 1.0, 1.0, 1.0, 1.0, 9e9, 9e9, 9e9, 9e9]   # n = 5: fixed rows do not count
    assert HS.lambda_of(Hb, 5, 1) == 1e-5 * 7.0
    assert HS.lambda_of(Hb, 5, 2) == 1e-5 * 7.0 * 2 and HS.lambda_of(Hb, 5, 3) == 1e-5 * 7.0 * 8 and HS.lambda_of(Hb, 5, 5) == 1e-5 * 7.0 * 1024


# ---- what both tests assert of one LM step --------------------------------------------------------------------------------------------
def run_check(name, c, Hdense, b, row, after):
    """H, b at the start state, the iteration's log row and the band after it -> the figures of hp_solve.check; asserts everything that
    does not depend on who produced the step: the trial count, an accepted trial (the lambda_k reconstruction with it), headings."""
    n, batch = c["n"], c["batch"]
    k = int(row[2])
    assert row[2] == k and 1 <= k < 10 and int(row[3]) == n, row
    assert k >= c["min_k"], "this case is here for a rejected first trial"
    Hb = hp.band_of_dense(Hdense)
    F = HS.check(Hb, b, n, k, batch.get_teb(0), after.get_teb(0))
    # accepted (rho > 0): lambda after the iteration is lambda_k times a factor in [1/3, 2/3]; a rejected one leaves >= 2 lambda_k
    assert F["lam"] / 3 * (1 - 4 * EPS) <= row[1] <= F["lam"] * 2 / 3 * (1 + 4 * EPS), (row[1], F["lam"])
    assert max(np.abs(batch.theta[0, :n]).max(), np.abs(after.theta[0, :n]).max()) <= SC.MAX_THETA
    print(HS.report(name, F))
    return F


def assert_bounds(F):
    assert F["omega"] <= F["bound_omega"], ("omega", F["omega"] / EPS, "row", F["omega_row"], "bound", F["bound_omega"] / EPS)
    assert F["fwd"] <= F["bound_fwd"], ("forward", F["fwd"] / EPS, "bound", F["bound_fwd"] / EPS)


# ---- the pipeline with the oracle as the device, and the conditions on the inputs --------------------------------------------------------
def test_the_case_table_is_the_one_the_issue_sets():
    for layout, sizes in SC.SIZES.items():
        for n in sizes:
            assert "%s_n%d" % (layout, n) in SC.CASES
    assert SC.SIZES["cr"] == (3, 4, 5, 16, 17, 32, 33, 64, 65, 129, 238) and SC.SIZES["band_ldlt"] == (5, 65, 257)
    assert SC.SIZES["band"] == (3, 5, 33, 65, 128, 129, 130, 255, 256, 257, 258, 337) and SC.SIZES["bandg"] == (5, 129, 257, 338, 512, 513, 944)
    for layout in ("cr", "band", "bandg"):
        assert sum(1 for v in SC.CASES.values() if v["layout"] == layout and v["kw"].get("footprint") == "polygon") == 1
        assert any(v["layout"] == layout and v["min_k"] >= 2 and not v["helpers"] for v in SC.CASES.values())
    for layout in ("cr", "band"):
        assert any(v["layout"] == layout and v["min_k"] >= 2 and v["helpers"] for v in SC.CASES.values())


@pytest.mark.parametrize("name", list(SC.CASES))
def test_pipeline_with_the_oracle_as_the_device(oracle, name):
    c = SC.build(name)
    cfg, obst, via, batch, n = c["cfg"], c["obst"], c["via"], c["batch"], c["n"]
    assert batch.count == 1 and int(batch.n[0]) == n and not cfg.trajectory.teb_autosize
    A = oracle.linearize(cfg, obst, via, batch, 0, 1.0)
    assert A["chi2"][hp.CAT_OBST] > 0, "no obstacle row is active"
    out, res, tr = oracle.optimize_batch(cfg, obst, via, batch, inner=1, outer=1, trace=True)
    assert len(tr[0]) == 1 and out.n[0] == n
    F = run_check(name, c, A["H"], A["b"], tr[0][0], out)
    assert F["noise_share"] <= NOISE_SHARE, F["noise_share"] / EPS
    assert_bounds(F)
