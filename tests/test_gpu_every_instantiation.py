"""Every pre-built instantiation of the optimise kernel is launched and its bands are COMPARED (tools/launch_every_instantiation.py records
the launches, one process per layout: a GPU memory fault aborts only that process and its last line says which case; this module judges
the records). ADVICE r05 / r06: the miscompile of the out-of-line solve call (profiles/fault_bisect_r05.txt) moves between translation
units with their register allocation, and a wrong clobber mask may as well corrupt a live register and return finite, wrong poses as
fault. The safe calling conventions were measured and cost + 0.9 % time and 5 x the fabric traffic (IPRA off) or + 3.2 % (plain
convention) on the headline (teb_local_planner_amd/build.py above HIPCC_FLAGS): the default kinds keep the cheap call, this test is the net.
Per case, on the configuration's own schedule (5 x 4):
  a. a case on a specialised kind (4 .. 11) has a generic twin (generic_config_path, a -DTEB_AMD_SOLVE_CSR unit) that reports the generic
     kind of the same size class and the same helper counts, and returns the same bits (same_bits of test_gpu_config_profile.py);
  b. the run with helpers reports helpers, the run of the same scene without reports none, and the two return the same bits;
  c. oracle parity in the case's own Jacobian mode - closed form: the rule of test_randomized_scenes_full_parity (status, pose count, LM
     iteration / trial counts identical; state and relative cost <= 1e-7 on well-conditioned bands, <= 1e-6 on the others), g2o numeric:
     the rule of test_optimizeTEB_matches_reference_code (status and pose count identical, state and relative cost within the band's
     sensitivity.band_tolerances) - on EVERY band; no overflow flag;
  d. at least one rejected LM trial (the retry path, and with helpers the speculative solve, ran);
  e. every element of EXPECTED is compared: by the oracle, and by a twin where it is a specialised kind.
The instantiations of the cases, their twins and the build's units are tied together on the CPU by tests/test_instantiation_table.py."""
import collections
import importlib.util
import os
import subprocess
import sys
import types

import numpy as np
import pytest

import sensitivity
from test_gpu_config_profile import same_bits
from teb_local_planner_amd import _abi

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "launch_every_instantiation.py")
UNREACHABLE = {}   # (the band-in-HBM layout's point-like small-batch kinds cannot be launched and are no longer built: tools/launch_every_instantiation.py)
THREADS = min(os.cpu_count() or 1, 16)


def _tool():
    spec = importlib.util.spec_from_file_location("launch_every_instantiation", TOOL)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _load(path):
    with np.load(path) as z:
        return types.SimpleNamespace(**{k: z[k] for k in z.files})


def _teb(r, b):
    n = int(r.n[b])
    return r.x[b, :n], r.y[b, :n], r.theta[b, :n], r.dt[b, :n - 1]


def _differs(a, b):
    """None when same_bits holds for the two records, else the fields that differ"""
    try:
        same_bits(a, a, b, b)
    except AssertionError:
        return "fields " + ", ".join(f for f in ("n", "x", "y", "theta", "dt", "status", "lm_iterations", "lm_trials", "chi2", "cost")
                                     if not np.array_equal(getattr(a, f), getattr(b, f)))
    return None


def _oracle_parity(oracle, case, rec, bad):
    """c. of the module docstring for one case; returns (max state error, max relative cost error, rejected trials of the oracle)"""
    cfg, obst, via, batch = case.cfg, case.obst, case.via, case.batch
    tols = sensitivity.band_tolerances(oracle, cfg, obst, via, batch, threads=THREADS)
    ref, rres = oracle.optimize_batch(cfg, obst, via, batch, threads=THREADS)
    numeric = cfg.jacobian_mode == _abi.JACOBIAN_G2O_NUMERIC
    worst_state = worst_cost = 0.0
    for b in range(batch.count):
        if int(rec.status[b]) != int(rres.status[b]) or int(rec.n[b]) != int(ref.n[b]):
            bad("band %d: status %d n %d, oracle %d n %d" % (b, rec.status[b], rec.n[b], rres.status[b], ref.n[b]))
            continue
        counts = (int(rec.lm_iterations[b]), int(rec.lm_trials[b]), int(rres.lm_iterations[b]), int(rres.lm_trials[b]))
        if numeric:
            print("    band %d: LM iterations / trials %d / %d, oracle %d / %d" % ((b,) + counts))
            if tols[b] is None:
                bad("band %d: no tolerance (the oracle's two Jacobian modes end apart): the band would be skipped" % b)
                continue
            bound = tols[b]
        else:
            if counts[:2] != counts[2:]:
                bad("band %d: LM iterations / trials %d / %d, oracle %d / %d" % ((b,) + counts))
            well = tols[b] is not None and tols[b] <= sensitivity.WELL_CONDITIONED_TOL
            bound = 1e-7 if well else 1e-6
        d = max(float(np.abs(u - v).max()) for u, v in zip(_teb(rec, b), ref.get_teb(b)))
        worst_state = max(worst_state, d)
        if d > bound:
            bad("band %d: state error %.3g > %.3g" % (b, d, bound))
        if np.isfinite(rres.cost[b]):
            dc = abs(float(rec.cost[b]) - float(rres.cost[b]))
            if rres.cost[b] != 0:
                worst_cost = max(worst_cost, dc / abs(float(rres.cost[b])))
            if not dc <= bound * abs(float(rres.cost[b])):
                bad("band %d: cost %.17g, oracle %.17g (bound %.3g relative)" % (b, rec.cost[b], rres.cost[b], bound))
        elif numeric:
            bad("band %d: oracle cost %s" % (b, rres.cost[b]))
    return worst_state, worst_cost, int((rres.lm_trials - rres.lm_iterations).sum())


@pytest.mark.parametrize("layout", ["band", "blocks", "bandg"])
def test_every_prebuilt_instantiation_of_the_layout_launches(layout, oracle, tmp_path):
    """... and matches its generic twin, its helper pair and the oracle (the module docstring)"""
    LE = _tool()
    r = subprocess.run([sys.executable, TOOL, layout, "--out", str(tmp_path)], cwd=ROOT, capture_output=True, text=True, timeout=900)
    print(r.stdout[-12000:])
    assert r.returncode == 0, "layout %s: rc %d after: %s | %s" % (layout, r.returncode, (r.stdout.strip().splitlines() or ["-"])[-1], r.stderr[-400:])
    lay = LE.LAYOUTS[layout]
    cases = LE.cases(layout)
    index = {c.label: i for i, c in enumerate(cases)}
    recs = [_load(tmp_path / ("%s_%02d.npz" % (layout, i))) for i in range(len(cases))]
    errors = []
    # per instantiation: cases, twin / helper-pair verdicts, worst oracle errors, rejected trials (device, oracle)
    table = collections.defaultdict(lambda: dict(cases=0, compared=False, twin=[], pair=[], state=0.0, cost=0.0, rejected=0, oracle_rejected=0))
    for k in LE.EXPECTED:
        if k[0] == lay:
            table[k]

    for i, (case, rec) in enumerate(zip(cases, recs)):
        def bad(msg, case=case):
            errors.append("%s | %s: %s" % (layout, case.label, msg))
        assert str(rec.label) == case.label, (str(rec.label), case.label)
        inst = tuple(int(v) for v in rec.instantiation)
        info = tuple(int(v) for v in rec.launch_info)
        row = table[inst]
        row["cases"] += 1
        if inst != (lay,) + tuple(case.expected):
            bad("ran instantiation %s, expected %s" % (inst, (lay,) + tuple(case.expected)))
        if not ((rec.status == _abi.TEB_OK).all() and all(np.isfinite(getattr(rec, f)).all() for f in ("x", "y", "theta", "dt", "cost"))):
            bad("status %s or non-finite output" % rec.status.tolist())
        if rec.overflow.any():
            bad("overflow flags %s" % rec.overflow.tolist())
        rejected = int((rec.lm_trials - rec.lm_iterations).sum())
        row["rejected"] += rejected
        if rejected <= 0:
            bad("no rejected LM trial: the retry path did not run")
        # a. the generic twin
        kind = inst[2]
        if case.twin:
            tw = _load(tmp_path / ("%s_%02d_twin.npz" % (layout, i)))
            tinst = tuple(int(v) for v in tw.instantiation)
            want = (lay, inst[1], LE.TWIN_KIND.get(kind, -1))
            msg = None
            if tinst != want:
                msg = "twin ran instantiation %s, expected %s" % (tinst, want)
            elif tuple(int(v) for v in tw.launch_info[:2]) != info[:2]:
                msg = "twin helpers %s, case %s" % (tuple(tw.launch_info[:2].tolist()), info[:2])
            elif tw.overflow.any():
                msg = "twin overflow flags %s" % tw.overflow.tolist()
            else:
                msg = _differs(rec, tw)
                msg = msg and "bands differ from the generic twin: " + msg
            row["twin"].append(msg is None)
            if msg:
                bad(msg)
        elif kind >= 4:
            bad("specialised kind %d without a generic twin" % kind)
        # b. the helper pair
        if case.pair:
            j = index[case.pair]
            p, pinst = recs[j], tuple(int(v) for v in recs[j].instantiation)
            msg = None
            if sum(info[:2]) <= 0:
                msg = "the run with helpers reports helpers %s" % (info[:2],)
            elif tuple(int(v) for v in p.launch_info[:2]) != (0, 0):
                msg = "the run without helpers reports helpers %s" % (tuple(p.launch_info[:2].tolist()),)
            else:
                msg = _differs(rec, p)
                msg = msg and "bands differ from the run without helpers: " + msg
            row["pair"].append(msg is None)
            table[pinst]["pair"].append(msg is None)
            if msg:
                bad(msg)
        # c. the oracle
        print("%s | %s: instantiation %s helpers %s one-CU repeat %d rejected trials %d" % (layout, case.label, inst, info[:2], info[2], rejected))
        st, co, orej = _oracle_parity(oracle, case, rec, bad)
        row["state"] = max(row["state"], st)
        row["cost"] = max(row["cost"], co)
        row["oracle_rejected"] += orej
        row["compared"] = True

    # e. coverage
    for k in sorted(k for k in LE.EXPECTED if k[0] == lay):
        if k in UNREACHABLE.get(layout, set()):
            continue
        row = table[k]
        if not row["compared"]:
            errors.append("%s: instantiation %s: no case compared it with the oracle" % (layout, k))
        if k[2] >= 4 and not row["twin"]:
            errors.append("%s: instantiation %s: no case compared it with its generic twin" % (layout, k))

    def verdict(v):
        return "-" if not v else ("ok x%d" % len(v) if all(v) else "DIFFERENT %d of %d" % (v.count(False), len(v)))
    print("\n%s: instantiation   cases  generic twin    helper pair     max state err  max cost rel   rejected trials (device / oracle)" % layout)
    for k in sorted(table):
        row = table[k]
        print("%s: %-16s %5d  %-14s  %-14s  %13.3g  %12.3g   %d / %d%s" % (
            layout, k, row["cases"], verdict(row["twin"]) if k[2] >= 4 else "(generic)", verdict(row["pair"]), row["state"], row["cost"],
            row["rejected"], row["oracle_rejected"], "" if k in LE.EXPECTED else "   NOT IN EXPECTED"))
    assert not errors, "\n".join(errors)
