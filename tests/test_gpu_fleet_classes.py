"""Equivalence classes per scene of a fleet batch on the MI355X (include/teb_amd.h: teb_amd_compute_h_signatures_per_scene,
teb_amd_filter_equivalence_classes_per_scene, teb_amd_filter_detours_per_scene) - renewAndAnalyzeOldTebs of every robot of a fleet.

  * signatures: every band's values equal, bit for bit, those of a single-scene handle that holds only its scene (2-D, 3-D, 3-D with
    either kernel pinned; 255 / 256 / 257 rows in the widest scene), and the CPU oracle within the tolerances of
    tests/test_gpu_hsignature.py (3-D: 4 ulp x max(1, |want|); 2-D: 1e-10 of the scene's largest |value|);
  * class filter and detour filter: equal to the oracle's rule per scene AND to the single-scene handles, remembered best class included;
  * a renew step end to end beside three single-scene handles, bit for bit; state and errors.

The fixtures (tests/fleet_class_cases.py) and the margins that make every decision robust are checked on the CPU in
tests/test_fleet_classes.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import fleet_cases  # noqa: E402
import fleet_class_cases as FC  # noqa: E402

from teb_local_planner_amd import _abi, planner  # noqa: E402

pytestmark = pytest.mark.gpu

THRESHOLD = 0.1
EPS = np.finfo(float).eps
SINGLE = dict(generic_config_path=True, multi_cu=-1, speculative_trials=-1)


def _fleet_solver(f, **opts):
    mo, mv, mw = f.capacities()
    s = planner.TebBatchSolver(f.cfg, f.batch.count, f.batch.stride, mo, mv, mw, options=_abi.Options(**opts))
    s.set_scenes(f.tables, f.vias)
    s.set_band_scenes(f.scene_of)
    s.upload(f.batch)
    return s


def _single_solvers(f, **opts):
    """{scene: (band indices, single-scene handle holding tables[scene] and the scene's bands)} for the scenes with bands"""
    mo, mv, mw = f.capacities()
    out = {}
    for sc in range(f.n_scenes):
        sub, idx = f.scene_batch(sc)
        if not idx:
            continue
        s = planner.TebBatchSolver(f.cfg, f.batch.count, f.batch.stride, mo, mv, mw, options=_abi.Options(**opts))
        s.set_obstacles(f.tables[sc])
        s.set_via_points(f.vias[sc])
        s.upload(sub)
        out[sc] = (idx, s, sub)
    return out


def _close(singles):
    for _, s, _ in singles.values():
        s.close()


@pytest.fixture(scope="module")
def oracle_signatures(oracle):
    """(big_rows, mode) -> (fleet, {scene: [bands, W]}) - computed once, shared, never written to"""
    cache = {}

    def get(big, mode):
        if (big, mode) not in cache:
            f = FC.point_class_fleet(big, dynamic=(mode == 3))
            sig = {}
            for sc in range(f.n_scenes):
                sub, idx = f.scene_batch(sc)
                if idx:
                    sig[sc] = oracle.h_signatures(f.cfg, f.tables[sc], sub, mode, FC.PRESCALER[mode])
                    sig[sc].setflags(write=False)
            cache[big, mode] = (f, sig)
        return cache[big, mode]
    return get


KERNELS = [(2, "auto"), (3, "auto"), (3, "wide"), (3, "small")]


@pytest.mark.parametrize("big", [255, 256, 257])
@pytest.mark.parametrize("mode,kern", KERNELS)
def test_signatures_equal_single_scene_handles_bit_for_bit(mode, kern, big):
    f = FC.point_class_fleet(big, dynamic=(mode == 3))
    s = _fleet_solver(f, hsig3d_kernel=kern)
    sig = s.h_signatures_per_scene(FC.PRESCALER[mode])
    assert len(sig) == f.batch.count
    rows = [len(t) for t in f.tables]
    # offset is the prefix sum of the scenes' row counts (3-D) / of 2 (2-D)
    off = np.zeros(f.batch.count + 1, np.int32); n = C.c_int64(-1)
    planner._chk(planner.lib().teb_amd_compute_h_signatures_per_scene(s._h, FC.PRESCALER[mode], None, 0, _abi._ptr(off, C.c_int32), C.byref(n)), "compute")
    widths = [rows[sc] if mode == 3 else 2 for sc in f.scene_of]
    np.testing.assert_array_equal(off, np.concatenate([[0], np.cumsum(widths)]))
    assert n.value == sum(widths) and [len(v) for v in sig] == widths
    singles = _single_solvers(f, hsig3d_kernel=kern)
    seen = 0
    for sc, (idx, s1, _) in singles.items():
        one = s1.h_signatures(FC.PRESCALER[mode])
        assert one.shape == (len(idx), rows[sc] if mode == 3 else 2)
        for k, b in enumerate(idx):
            np.testing.assert_array_equal(sig[b], one[k], err_msg="scene %d (%d rows), band %d" % (sc, rows[sc], b))
            seen += 1
        if rows[sc] == 0:   # a scene without rows: no values in 3-D, (0, 0) in 2-D
            for b in idx:
                assert (len(sig[b]) == 0) if mode == 3 else (sig[b] == 0).all()
        elif mode == 3:
            assert all(np.abs(sig[b]).max() > 0 for b in idx)
    assert seen == f.batch.count
    _close(singles)
    s.close()


@pytest.mark.parametrize("big", [255, 256, 257])
@pytest.mark.parametrize("mode,kern", KERNELS)
def test_signatures_against_the_oracle(oracle_signatures, mode, kern, big):
    f, want = oracle_signatures(big, mode)
    s = _fleet_solver(f, hsig3d_kernel=kern)
    sig = s.h_signatures_per_scene(FC.PRESCALER[mode])
    s.close()
    for sc, w in want.items():
        idx = f.bands_of(sc)
        got = np.array([sig[b] for b in idx]).reshape(w.shape)
        if w.size == 0:
            continue
        err = np.abs(got - w).max()
        print("scene %d, %d rows, mode %d/%s: max |device - oracle| = %.3e, largest |value| = %.3e" % (sc, len(f.tables[sc]), mode, kern, err, np.abs(w).max()))
        if mode == 3:
            assert (np.abs(got - w) <= 4 * EPS * np.maximum(1.0, np.abs(w))).all(), (sc, err)
        else:
            assert err <= 1e-10 * np.abs(w).max(), (sc, err, np.abs(w).max())


def _best_per_scene(f):
    """A band of every scene that has one: the k of KEEPS_TWO_OF_BEST where the fixture names one, else the scene's last band."""
    best = np.full(f.n_scenes, -1, np.int32)
    for sc in range(f.n_scenes):
        idx = f.bands_of(sc)
        if idx:
            best[sc] = idx[FC.KEEPS_TWO_OF_BEST.get(sc, len(idx) - 1)]
    return best


@pytest.mark.parametrize("mode", [2, 3])
def test_class_filter_equals_the_oracle_and_the_single_scene_handles(oracle, oracle_signatures, mode):
    f, want = oracle_signatures(256, mode)
    s = _fleet_solver(f)
    s.h_signatures_per_scene(FC.PRESCALER[mode], values=False)
    singles = _single_solvers(f)
    for _, s1, _ in singles.values():
        s1.h_signatures(FC.PRESCALER[mode], values=False)
    best = _best_per_scene(f)
    dropped = kept_two = 0
    remembered = False   # after the first call with a best band every scene carries its class into the calls without one
    for use_best, maxp in ((False, 1), (False, 2), (True, 1), (True, 2), (False, 1), (False, 2)):
        got = s.filter_equivalence_classes_per_scene(THRESHOLD, best if use_best else None, maxp)
        remembered = remembered or use_best
        for sc, (idx, s1, _) in singles.items():
            k = idx.index(int(best[sc]))
            ora = oracle.filter_equivalence_classes(mode, want[sc], THRESHOLD, k if use_best else -1, maxp,
                                                    stale_best_sig=want[sc][k] if (remembered and not use_best) else None)
            one = s1.filter_equivalence_classes(THRESHOLD, k if use_best else -1, maxp)
            for name, g, o, h in zip(("keep", "valid", "reasonable"), got, ora, one):
                np.testing.assert_array_equal(g[idx], o, err_msg="%s, scene %d against the oracle (best %s, %d plans)" % (name, sc, use_best, maxp))
                np.testing.assert_array_equal(g[idx], h, err_msg="%s, scene %d against its handle (best %s, %d plans)" % (name, sc, use_best, maxp))
            if not remembered and maxp == 1 and sc in FC.DROPS_A_CLASS:
                dropped += int(len(idx) - got[0][idx].sum())
            if use_best and maxp == 2 and sc in FC.KEEPS_TWO_OF_BEST:
                kept_two += 1
                assert got[0][idx].sum() == s.filter_equivalence_classes_per_scene(THRESHOLD, best, 1)[0][idx].sum() + 1
    assert dropped >= len(FC.DROPS_A_CLASS) and kept_two == len(FC.KEEPS_TWO_OF_BEST)
    _close(singles)
    s.close()


def test_detour_filter_equals_the_oracle_and_the_single_scene_handles(oracle):
    f = FC.point_class_fleet(256)
    B = f.batch.count
    s = _fleet_solver(f)
    singles = _single_solvers(f)
    best = np.full(f.n_scenes, -1, np.int32)
    for sc in range(f.n_scenes):
        idx = f.bands_of(sc)
        if idx and sc != 2:   # scene 2: no best (the rule does not run there)
            best[sc] = idx[FC.LOSES_A_DETOUR[sc][0]] if sc in FC.LOSES_A_DETOUR else idx[0]
    assert len(f.bands_of(4)) == 1 and best[4] >= 0   # one kept band: the early-out
    opt = np.ones(B, np.int32)
    opt[f.bands_of(5)[1]] = 0   # a band that was never optimised (not the best of its scene)
    s.set_optimized_flags(opt)
    keep = s.filter_detours_per_scene(np.ones(B, np.int32), best)
    for sc, (idx, s1, sub) in singles.items():
        k = idx.index(int(best[sc])) if best[sc] >= 0 else -1
        s1.set_optimized_flags(opt[idx])
        ones = np.ones(len(idx), np.int32)
        np.testing.assert_array_equal(keep[idx], oracle.filter_detours(f.cfg, sub, ones, k, opt[idx]), err_msg="scene %d against the oracle" % sc)
        np.testing.assert_array_equal(keep[idx], s1.filter_detours(ones, k), err_msg="scene %d against its handle" % sc)
    for sc, (kb, kd) in FC.LOSES_A_DETOUR.items():
        assert keep[f.bands_of(sc)[kd]] == 0 and keep[f.bands_of(sc)[kb]] == 1
    assert keep[f.bands_of(5)[1]] == 0 and keep[f.bands_of(2)].all() and keep[f.bands_of(4)].all()
    # bands that the class filter dropped before stay dropped and do not count as kept
    pre = np.ones(B, np.int32); pre[f.bands_of(0)[1]] = 0
    again = s.filter_detours_per_scene(pre, best)
    assert again[f.bands_of(0)[1]] == 0 and again[f.bands_of(0)[0]] == 1
    _close(singles)
    s.close()


def _optimize(s, cfg):
    s.optimize(cfg.optim.no_inner_iterations, cfg.optim.no_outer_iterations, True, cfg.hcp.selection_obst_cost_scale,
               cfg.hcp.selection_viapoint_cost_scale, cfg.hcp.selection_alternative_time_cost)


def test_renew_step_end_to_end_equals_three_single_scene_handles():
    f = fleet_cases.point_fleet(106, n_scenes=3, stride=96, bands=(3, 5))
    cfg = f.cfg
    hp = cfg.hcp
    s = _fleet_solver(f, layout="cr")
    singles = _single_solvers(f, layout="cr", **SINGLE)
    assert len(singles) == 3
    # fleet: optimise -> signatures -> classes -> detours -> compact -> optimise -> select
    _optimize(s, cfg)
    last, _ = s.select_best_per_scene()
    s.h_signatures_per_scene(hp.h_signature_prescaler, values=False)
    keep, _, _ = s.filter_equivalence_classes_per_scene(hp.h_signature_threshold, last, hp.max_number_plans_in_current_class)
    after_classes = int(keep.sum())
    keep = s.filter_detours_per_scene(keep, last)
    print("renew step: %d bands, %d after the class filter, %d after the detour filter" % (f.batch.count, after_classes, int(keep.sum())))
    assert s.compact_bands(keep)[0] == int(keep.sum())
    _optimize(s, cfg)
    winners, wcost = s.select_best_per_scene()
    out, res = s.download(f.batch.copy()), s.results()
    assert (res.status == _abi.TEB_OK).all()
    kept = [b for b in range(f.batch.count) if keep[b]]   # fleet band k after the compaction was band kept[k]
    assert 3 <= len(kept)
    for sc, (idx, s1, sub) in singles.items():
        _optimize(s1, cfg)
        l1, _ = s1.select_best()
        assert idx[l1] == last[sc]
        s1.h_signatures(hp.h_signature_prescaler, values=False)
        k1, _, _ = s1.filter_equivalence_classes(hp.h_signature_threshold, l1, hp.max_number_plans_in_current_class)
        k1 = s1.filter_detours(k1, l1)
        np.testing.assert_array_equal(keep[idx], k1, err_msg="kept set of scene %d" % sc)
        s1.compact_bands(k1)
        _optimize(s1, cfg)
        w1, c1 = s1.select_best()
        out1, res1 = s1.download(sub.copy()), s1.results()
        mine = [k for k, b in enumerate(kept) if f.scene_of[b] == sc]   # the scene's bands in the compacted fleet, in order
        assert len(mine) == int(k1.sum())
        assert mine[w1] == winners[sc] and c1 == wcost[sc]
        for j, k in enumerate(mine):
            assert int(out.n[k]) == int(out1.n[j])
            for name, u, v in zip(("x", "y", "theta", "dt"), out.get_teb(k), out1.get_teb(j)):
                np.testing.assert_array_equal(u, v, err_msg="scene %d, band %d, %s" % (sc, k, name))
            for fld in ("status", "lm_iterations", "lm_trials", "chi2", "cost", "lambda_"):
                np.testing.assert_array_equal(getattr(res, fld)[k], getattr(res1, fld)[j], err_msg="scene %d, band %d, %s" % (sc, k, fld))
    _close(singles)
    s.close()


def _refused(call, *words):
    with pytest.raises(planner.TebAmdError) as e:
        call()
    assert e.value.code == _abi.ERR_INVALID_ARG and all(w in str(e.value) for w in words), str(e.value)


@pytest.mark.parametrize("mode", [2, 3])
def test_state_and_errors(mode):
    f = FC.point_class_fleet(256, dynamic=(mode == 3))
    B = f.batch.count
    mo, mv, mw = f.capacities()
    s = planner.TebBatchSolver(f.cfg, B, f.batch.stride, mo, mv, mw)
    # single-scene mode: scene 1 with ITS bands first; what it gives is recorded
    sub, idx = f.scene_batch(1)
    s.set_obstacles(f.tables[1]); s.upload(sub)
    for name, call in (("teb_amd_compute_h_signatures_per_scene", lambda: s.h_signatures_per_scene()),
                       ("teb_amd_filter_equivalence_classes_per_scene", lambda: s.filter_equivalence_classes_per_scene()),
                       ("teb_amd_filter_detours_per_scene", lambda: s.filter_detours_per_scene(np.ones(len(idx), np.int32), None))):
        _refused(call, "teb_amd_set_scenes", name)
    sig0 = s.h_signatures(FC.PRESCALER[mode])
    with_best = s.filter_equivalence_classes(THRESHOLD, 0, 2)
    stale0 = s.filter_equivalence_classes(THRESHOLD, -1, 2)   # relies on the class remembered from band 0
    assert stale0[0].sum() != s.filter_equivalence_classes(THRESHOLD, -1, 1)[0].sum(), "the remembered class changes nothing: the case checks nothing"
    # fleet mode on the same handle
    s.set_scenes(f.tables, f.vias); s.set_band_scenes(f.scene_of); s.upload(f.batch)
    _refused(lambda: s.filter_equivalence_classes_per_scene(), "teb_amd_compute_h_signatures_per_scene")   # filter before compute
    # a too-small capacity: the count comes back, the signatures are kept
    n = C.c_int64(-1); small = np.zeros(1)
    rc = planner.lib().teb_amd_compute_h_signatures_per_scene(s._h, FC.PRESCALER[mode], _abi._ptr(small, C.c_double), 1, None, C.byref(n))
    widths = [len(f.tables[sc]) if mode == 3 else 2 for sc in f.scene_of]
    assert rc == _abi.ERR_CAPACITY and n.value == sum(widths) and small[0] == 0
    first = s.filter_equivalence_classes_per_scene(THRESHOLD, _best_per_scene(f), 2)
    sig = s.h_signatures_per_scene(FC.PRESCALER[mode])
    for u, v in zip(first, s.filter_equivalence_classes_per_scene(THRESHOLD, _best_per_scene(f), 2)):
        np.testing.assert_array_equal(u, v)
    # best[s] names a band of another scene
    wrong = _best_per_scene(f); wrong[1] = f.bands_of(3)[0]
    _refused(lambda: s.filter_equivalence_classes_per_scene(THRESHOLD, wrong), "best[1]")
    _refused(lambda: s.filter_detours_per_scene(np.ones(B, np.int32), wrong), "best[1]")
    # what invalidates the signatures
    s.set_band_scenes(f.scene_of)
    _refused(lambda: s.filter_equivalence_classes_per_scene(), "teb_amd_compute_h_signatures_per_scene")
    s.h_signatures_per_scene(values=False)
    s.set_scenes(f.tables, f.vias)
    _refused(lambda: s.filter_equivalence_classes_per_scene(), "teb_amd_compute_h_signatures_per_scene")
    # the remembered classes survive set_scenes with the same scene count: no best now, two plans per class still keeps two
    s.h_signatures_per_scene(FC.PRESCALER[mode], values=False)
    for u, v in zip(first, s.filter_equivalence_classes_per_scene(THRESHOLD, None, 2)):
        np.testing.assert_array_equal(u, v)
    # a band mapped to a scene >= n_scenes
    bad = f.scene_of.copy(); bad[0] = f.n_scenes
    s.set_band_scenes(bad)
    _refused(lambda: s.h_signatures_per_scene(), "scene")
    s.set_band_scenes(f.scene_of)
    # compact_bands invalidates as well (and is undone by the upload)
    s.h_signatures_per_scene(values=False)
    keep = np.ones(B, np.int32); keep[0] = 0
    s.compact_bands(keep)
    _refused(lambda: s.filter_equivalence_classes_per_scene(), "teb_amd_compute_h_signatures_per_scene")
    # back to the single scene: its signatures, its 2-D products and its remembered class are as they were
    s.clear_scenes()
    s.upload(sub)
    np.testing.assert_array_equal(s.h_signatures(FC.PRESCALER[mode]), sig0)
    for u, v in zip(s.filter_equivalence_classes(THRESHOLD, -1, 2), stale0):
        np.testing.assert_array_equal(u, v)
    for u, v in zip(s.filter_equivalence_classes(THRESHOLD, 0, 2), with_best):
        np.testing.assert_array_equal(u, v)
    # a scene set of another size forgets the remembered classes of the set
    s.set_scenes(f.tables, f.vias); s.set_band_scenes(f.scene_of); s.upload(f.batch)
    s.h_signatures_per_scene(FC.PRESCALER[mode], values=False)
    fresh = s.filter_equivalence_classes_per_scene(THRESHOLD, None, 2)
    assert fresh[0].sum() < first[0].sum()
    for b in range(B):
        np.testing.assert_array_equal(s.h_signatures_per_scene(FC.PRESCALER[mode])[b], sig[b])
    s.close()


def test_single_scene_signatures_survive_fleet_calls_without_recomputation():
    """compute + filter on the single scene, then a whole per-scene round on a scene set over the SAME resident bands, then
    clear_scenes: the single-scene filter answers from the signatures it had (no compute call in between)."""
    f = FC.point_class_fleet(256)
    sub, idx = f.scene_batch(1)
    mo, mv, mw = f.capacities()
    s = planner.TebBatchSolver(f.cfg, f.batch.count, f.batch.stride, mo, mv, mw)
    s.set_obstacles(f.tables[1]); s.upload(sub)
    s.h_signatures(values=False)
    before = s.filter_equivalence_classes(THRESHOLD, 0, 2)
    stale = s.filter_equivalence_classes(THRESHOLD, -1, 2)
    s.set_scenes([f.tables[3], f.tables[1]]); s.set_band_scenes([1, 0, 1, 0])
    s.h_signatures_per_scene(values=False)
    s.filter_equivalence_classes_per_scene(THRESHOLD, [1, 2], 2)
    s.filter_detours_per_scene(np.ones(len(idx), np.int32), [1, 2])
    s.clear_scenes()
    for u, v in zip(s.filter_equivalence_classes(THRESHOLD, -1, 2), stale):
        np.testing.assert_array_equal(u, v)
    for u, v in zip(s.filter_equivalence_classes(THRESHOLD, 0, 2), before):
        np.testing.assert_array_equal(u, v)
    s.close()
