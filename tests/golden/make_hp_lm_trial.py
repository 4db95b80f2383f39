"""Writes tests/golden/hp_lm_trial_*.npz: the 80-digit reference (tests/hp_lm_trial.py) of what one LM iteration does with its solved
step, for every scene of tests/hp_lm_trial_cases.py, rounded to float64. Run from the repository root:

    python tests/golden/make_hp_lm_trial.py [substring of the scene names to write; default all]

Per scene ("<scene>/<key>"), S0 the state the iteration starts from, S1 the CPU oracle's state after it, everything else from the
reference alone:
  n, k             pose count; the oracle's accepted damping trial
  s0, s1 [4][n]    x, y, theta, dt (padded with one 0)
  c [4], rows [4]  category sums {obstacle-type, via-point, time-optimal, other} of the graph built at S0, evaluated at S1, and the number
                   of residual rows behind each
  g [4][4n], S [4] their gradient at S1 and the second-order constant (sum of |Hessian entries|)
  c0, rows0 [4]    the category sums at S0 (chi^2_cur)
  hmax, b0 [4n]    max |H_ii| over the free variables and the right-hand side of the reference linearisation at S0
  trials [k]       chi^2 at the state of every damping trial 1 .. k, each state formed as S0 + the 60-digit step of tests/hp_solve.py on the
                   reference H and b with lambda_j, rounded once to fp64 (the last one is within the solve's forward error of S1)
  margins [2]      the smallest branch margin at S0 and over the trial states and S1 (the reference raises below 1e-7)
  scene, edges     sha256 of the inputs (hp_linearize.input_hash / edges_hash)
A scene of two outer iterations holds the SECOND one: s0 is the oracle's state after the first iteration, the graph is built there with
weight_multiplier = weight_adapt_factor, s1 is the state after both; `scene` is the hash of the uploaded scene all the same.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import hp_linearize as hp  # noqa: E402
import hp_solve as HS  # noqa: E402
import hp_lm_trial as LT  # noqa: E402
import hp_lm_trial_cases as TC  # noqa: E402

MAX_FILE_BYTES = 500 * 1000
LONG = 200   # scenes from this pose count on have a file of their own


def groups():
    """{file stem: [scene names]}"""
    out = {}
    for name, s in TC.SCENES.items():
        stem = "hp_lm_trial_" + name if s["n"] >= LONG else "hp_lm_trial_short"
        out.setdefault(stem, []).append(name)
    return out


def group_of(name):
    for stem, names in groups().items():
        if name in names:
            return stem
    raise KeyError(name)


def load(name):
    fx = np.load(os.path.join(HERE, group_of(name) + ".npz"))
    return {k[len(name) + 1:]: fx[k] for k in fx.files if k.startswith(name + "/")}


def f64(v):
    return np.array([float(q) for q in v])


def reference_record(name, oracle, derivatives=True):
    """(case, {key: array}) - the reference of one scene, recomputed (derivatives=False leaves g and S out: the CPU test recomputes
    them only for the short scenes)"""
    c = TC.build(name)
    cfg, obst, via, n = c["cfg"], c["obst"], c["via"], c["n"]
    batch, wm, outer = c["batch"], 1.0, c["outer"]
    if outer == 2:   # the fixture is of the second outer iteration: it starts at the oracle's state after the first one
        batch = oracle.optimize_batch(cfg, obst, via, batch, inner=1, outer=1)[0]
        wm = float(cfg.optim.weight_adapt_factor)
    ir, _ = oracle.edges(cfg, obst, via, batch, 0, wm)
    R0 = hp.linearize(cfg, obst, via, batch, 0, wm, ir)
    Hb, bv, c0 = hp.to_band(R0)
    rows0 = np.zeros(4, np.int64)
    for (t, r), st in R0["rows"].items():
        rows0[hp._CATEGORY.get(t, hp.CAT_OTHER)] += st[0]
    out, res, tr = oracle.optimize_batch(cfg, obst, via, c["batch"], inner=1, outer=outer, trace=True)
    assert len(tr[0]) == outer and int(out.n[0]) == n
    k = int(tr[0][-1][2])
    S0, S1 = TC.state_of(batch), TC.state_of(out)
    T = LT.chi2_at(cfg, obst, via, batch, tuple(S1), wm, ir, derivatives=derivatives)
    trials, margin1 = [], T["margin"]
    for j in range(1, k + 1):
        lam, dx = HS.reference_step(Hb, bv, n, j)
        Tj = LT.chi2_at(cfg, obst, via, batch, LT.state_plus(tuple(S0), dx, n), wm, ir)
        trials.append(float(sum(Tj["chi2"])))
        margin1 = min(margin1, Tj["margin"])
    rec = dict(n=np.int64(n), k=np.int64(k), s0=S0, s1=S1, c=f64(T["chi2"]), rows=np.array(T["rows"], np.int64), c0=c0, rows0=rows0,
               hmax=np.float64(LT.free_max_diagonal(R0)), b0=bv, trials=np.array(trials), margins=np.array([R0["margin"], margin1]),
               scene=np.array(hp.input_hash(cfg, obst, via, c["batch"], 0)), edges=np.array(hp.edges_hash(ir)))
    if derivatives:
        rec.update(g=np.array([f64(row) for row in T["grad"]]), S=f64(T["S"]))
    c.update(irec=ir, Hband=Hb, start=batch, wm=wm, oracle_out=out, row_kinds=R0["rows"])
    return c, {name + "/" + key: v for key, v in rec.items()}


def main():
    from oracle import oracle_py
    oracle_py.build()
    only = sys.argv[1] if len(sys.argv) > 1 else None
    for stem, names in groups().items():
        if only is not None and not any(only in name for name in names):
            continue
        data = {}
        for name in names:
            c, rec = reference_record(name, oracle_py)
            data.update(rec)
            print("  %-40s n %3d k %d chi2 %.6g -> %.6g margins %.2e %.2e" % (
                name, c["n"], int(rec[name + "/k"]), rec[name + "/c0"].sum(), rec[name + "/c"].sum(), *rec[name + "/margins"]), flush=True)
        path = os.path.join(HERE, stem + ".npz")
        np.savez_compressed(path, **data)
        size = os.path.getsize(path)
        assert size < MAX_FILE_BYTES, (path, size)
        print("%-50s %3d scenes %7d bytes" % (stem + ".npz", len(names), size), flush=True)


if __name__ == "__main__":
    main()
