"""The product kernel's LM trial - chi^2 per category, gain ratio, lambda update, band cost - against the 80-digit reference
(tests/test_hp_lm_trial.py is the CPU side and describes the reference, the tolerances and the cases; tests/hp_lm_trial.py,
tests/hp_lm_trial_cases.py, fixtures tests/golden/hp_lm_trial_*.npz). Needs neither mpmath nor the oracle.

No kernel and no entry point of its own. Per run (one band, teb_autosize off, inner = outer = 1, iteration log on, the layout pinned
and confirmed with last_instantiation): the six launches of hp_lm_trial.LAUNCHES on the same upload; the downloaded band, chi2 and
the log row must be bit-equal across them, the log's chi2 bit-equal to results.chi2; then hp_lm_trial.check_launches forms
delta = downloaded state - the fixture's and holds chi2 = ((c0 + c1) + c2) + c3, every launch's cost, k and the lambda after the
iteration to the reference, as on the CPU. A state whose second-order term exceeds 1e-10 c_k FAILS.
Also per run: the same launch with divergence detection on (max_chi_squared huge) gives the same band, chi2 and cost bit for bit and
batch_statistics() reports that chi2; the runs with no_near_cache = 1 must equal the plain run of their scene bit for bit; the
point-like scene on the generic distance path is held to the same reference as on the LDS path, nothing bitwise. The solver-helper runs
(speculative_trials = 3 on a rejected first trial, one per LDS layout) print whether the helpers arrived.
Three ragged bands (n = 3, 17, 65) run in one launch, as one scene and as a fleet batch of two scenes (set_scenes / set_band_scenes),
every band against the reference of its own scene. Two outer iterations (n = 17, point and polygon footprint): only the second
iteration's row and the final cost are checked; the start state of that iteration is the device's own (taken from a launch with
outer = 1, within 1e-8 of the oracle's), so lambda_k comes from the device's H there (debug_linearize, as tests/test_gpu_hp_solve.py
does) and rho carries the slack the CPU test derives for it.

Largest observed on an MI355X, per family (chi2 error / worst cost error, each in eps of its value and as a share of its tolerance;
||delta||_inf; largest k):
  pose counts, every layout          1.5 eps (0.06) / 3.9 eps (0.08); 6.8e-13; k 3
  edge families (n = 17)             1.9 eps (0.02) / 5.9 eps (0.06); 9.3e-14; k 3
  rejected first trials, helpers     2.2 eps (0.00) / 3.0 eps (0.02); 7.2e-14; k 5
  ragged bands, fleet batch          1.0 eps (0.03) / 2.9 eps (0.06); 2.3e-13; k 1
  two outer iterations               1.3 eps (0.01) / 2.4 eps (0.02); 2.4e-13; k 3 (the state after the first iteration 7.5e-14 from the oracle's)
The second-order part of the tolerance stayed below 1e-17 c_k; k was the oracle's everywhere; all solver helpers arrived. The
categories recovered by differencing the first four launches' costs are printed too; they carry the cancellation of that difference
(up to 1.5e3 eps of the time-optimal category, 31 against a cost of 7.7e4, at n = 513) and are not asserted on. No defect found.
The whole file takes 1.8 s (57 tests).
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
import hp_lm_trial as LT  # noqa: E402
import hp_lm_trial_cases as TC  # noqa: E402
import make_hp_lm_trial as MK  # noqa: E402

from teb_local_planner_amd import planner  # noqa: E402

pytestmark = pytest.mark.gpu
EPS = LT.EPS


def launch_all(s, batch, layout, keys=LT.LAUNCHES, outer=1):
    """[{launch: dict(after, chi2, cost, row, statistics, info)} per band]: the batch uploaded afresh for every launch"""
    s.set_iteration_log(True)
    out = [dict() for _ in range(batch.count)]
    for key in keys:
        s.upload(batch)
        s.optimize(1, outer, True, key[0], key[1], key[2])
        ran, info = s.last_instantiation(), s.last_launch_info()
        res = s.results()
        after = s.download(batch.copy())
        av, back = s.batch_statistics()
        if layout != "auto":
            assert ran[0] == TC.LAYOUT_INDEX[layout], (layout, ran)
        for b in range(batch.count):
            log = s.iteration_log(b)
            assert len(log) == outer and int(after.n[b]) == int(batch.n[b]) and int(res.status[b]) == 0, (b, log, after.n, res.status)
            out[b][key] = dict(after=after.get_teb(b), chi2=float(res.chi2[b]), cost=float(res.cost[b]), row=log[-1].copy(),
                               statistics=(bool(av[b]), float(back[b])), info=info)
    return out


def same_bits(A, B):
    return all(np.array_equal(u, v) for u, v in zip(A["after"], B["after"])) and A["chi2"] == B["chi2"] and A["cost"] == B["cost"] \
        and np.array_equal(A["row"], B["row"])


def run_scene(c, options, layout, **kw):
    s = planner.make_solver(c["cfg"], c["obst"], c["via"], c["batch"], options=options)
    L = launch_all(s, c["batch"], layout, **kw)
    s.close()
    return L[0]


def load(scene, c, b=0):
    F = MK.load(scene)
    assert str(F["scene"]) == hp.input_hash(c["cfg"], c["obst"], c["via"], c["batch"], b), "the fixture is of another scene"
    return F


@pytest.mark.parametrize("run", list(TC.RUNS))
def test_lm_trial_against_the_reference(run):
    scene, layout, opt = TC.RUNS[run]
    stride = TC.HELPERS[run][1] if run in TC.HELPERS else None
    c = TC.build(scene, stride=stride)
    F = load(scene, c)
    assert np.array_equal(TC.state_of(c["batch"]), F["s0"])
    L = run_scene(c, TC.options(run), layout)
    first = L[LT.LAUNCHES[0]]
    if run in TC.HELPERS:
        assert first["info"][1] == 3, first["info"]
        print("%s: %d solver helpers per band; %s" % (run, first["info"][1], "the helpers did not arrive in time - the one-CU path ran"
                                                      if first["info"][2] else "the helpers arrived"))
    fig = LT.check_launches(run, F, c["batch"].get_teb(0), L)
    LT.assert_figures(run, fig)
    # divergence detection: evaluate runs once more on the accepted state, with the trig cache as the update step left it
    c["cfg"].recovery.divergence_detection_enable = True
    c["cfg"].recovery.divergence_detection_max_chi_squared = 1e300
    D = run_scene(c, TC.options(run), layout, keys=(LT.LAUNCHES[0], LT.LAUNCHES[5]))
    for key, v in D.items():
        assert same_bits(v, L[key]), (run, key, "divergence detection changed the result", v["chi2"], L[key]["chi2"], v["cost"], L[key]["cost"])
        assert v["statistics"] == (True, v["chi2"]), v["statistics"]
    if opt.get("no_near_cache"):
        plain = run_scene(TC.build(scene), TC.options_of(layout), layout)
        for key in LT.LAUNCHES:
            assert same_bits(plain[key], L[key]), (run, key, "no_near_cache changed the result")


@pytest.mark.parametrize("fleet", [False, True], ids=["one_scene", "fleet_of_two_scenes"])
def test_three_ragged_bands_in_one_launch(fleet):
    names = TC.FLEET if fleet else TC.RAGGED
    cfg, cases, batch = TC.ragged_batch(names)
    tables = [cases[0]["obst"], cases[1]["obst"]]
    if fleet:
        s = planner.TebBatchSolver(cfg, batch.count, batch.stride, len(tables[0]) + len(tables[1]), 1, 1, options=TC.options_of("auto"))
        s.set_scenes(tables, [[], []])
        s.set_band_scenes(list(TC.FLEET_SCENE_OF))
        s.upload(batch)
    else:
        s = planner.make_solver(cfg, tables[0], [], batch, options=TC.options_of("auto"))
    L = launch_all(s, batch, "auto")
    s.close()
    for b, (name, c) in enumerate(zip(names, cases)):
        fig = LT.check_launches("%s (band %d%s)" % (name, b, ", scene %d" % TC.FLEET_SCENE_OF[b] if fleet else ""), load(name, c), c["batch"].get_teb(0), L[b])
        LT.assert_figures(name, fig)


@pytest.mark.parametrize("scene", list(TC.OUTER2))
def test_second_outer_iteration(scene):
    c = TC.build(scene)
    F = load(scene, c)
    cfg, obst, via, batch, n = c["cfg"], c["obst"], c["via"], c["batch"], c["n"]
    opt = TC.options_of("auto")
    s = planner.make_solver(cfg, obst, via, batch, options=opt)
    s.optimize(1, 1)
    S1 = s.download(batch.copy())
    s.upload(S1)
    G = s.debug_linearize(0, n, float(cfg.optim.weight_adapt_factor))   # the device's own H at the state its second graph is built at
    s.close()
    d1 = float(np.abs(LT.flat(S1.get_teb(0), n) - LT.flat(tuple(F["s0"][q] for q in range(4)), n)).max())
    assert d1 <= TC.D1_MAX, d1
    L = run_scene(c, opt, "auto", outer=2)
    k = int(L[LT.LAUNCHES[0]]["row"][2])
    lam_k = HS.lambda_of(hp.band_of_dense(G["H"]), n, k)
    fig = LT.check_launches(scene, F, S1.get_teb(0), L, lam=(lam_k * (1 - 4 * EPS), lam_k * (1 + 4 * EPS)), rho_slack=TC.SENS_MAX * d1)
    print("%s: the state after the first iteration is %.2e from the oracle's" % (scene, d1))
    LT.assert_figures(scene, fig)
