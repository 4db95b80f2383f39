"""The fixtures of the per-scene equivalence-class tests (tests/fleet_class_cases.py) on the CPU: the oracle plays the device. What the GPU
tests (tests/test_gpu_fleet_classes.py) rely on is asserted here, over oracle.h_signatures per scene:

  * every scene meant to drop a band under the class filter does, every scene meant to keep two bands of the best class does, every
    scene meant to lose a detour does;
  * every decision is separated from its threshold by far more than the device's error. 3-D (device <= 4 ulp): no |H| within 1e-9 of the
    threshold 0.1 or of 1.0 (isReasonable), and no entry that decides a sign (both values at or above the threshold) below 1e-9.
    2-D (device <= 1e-10 of the scene's largest |value|): no |d re| or |d im| between two bands of a scene within 1e-8 x that largest
    |value| of the threshold - 100 x the device tolerance.

Nothing is skipped: a seed that violates a condition is replaced in the fixture file."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import fleet_class_cases as FC  # noqa: E402

THRESHOLD = 0.1
BIG_ROWS = (255, 256, 257)


def scene_signatures(oracle, f, mode):
    """[n_scenes] (band indices, [bands, W] oracle signatures)"""
    out = []
    for s in range(f.n_scenes):
        sub, idx = f.scene_batch(s)
        sig = oracle.h_signatures(f.cfg, f.tables[s], sub, mode, FC.PRESCALER[mode]) if idx else np.zeros((0, len(f.tables[s]) if mode == 3 else 2))
        out.append((idx, sig))
    return out


@pytest.fixture(scope="module")
def cases(oracle):
    got = {}
    for big in BIG_ROWS:
        for mode in (2, 3):
            f = FC.point_class_fleet(big, dynamic=(mode == 3))
            got[big, mode] = (f, scene_signatures(oracle, f, mode))
    return got


def test_fixture_shapes():
    for big in BIG_ROWS:
        f = FC.point_class_fleet(big)
        rows = [len(t) for t in f.tables]
        assert rows == FC.rows_of(big) and {0, 1, 15, 16, 17, big} <= set(rows)
        assert rows.index(max(rows)) != 0                                    # the widest scene is not the first
        assert any(not f.bands_of(s) for s in range(f.n_scenes))             # a scene without bands
        assert any(rows[s] == 0 and f.bands_of(s) for s in range(f.n_scenes))   # bands against a scene without rows
        assert {2, 17, 18, 40} <= set(int(n) for n in f.batch.n) and f.batch.stride == 96
        runs = 1 + int((np.diff(f.scene_of) != 0).sum())
        assert runs > f.n_scenes, "the bands of the scenes are not interleaved"
        dup = [b for b in range(f.batch.count) if any(f.batch.x[b, i] == f.batch.x[b, i + 1] and f.batch.y[b, i] == f.batch.y[b, i + 1] and f.batch.dt[b, i] == 0
                                                      for i in range(int(f.batch.n[b]) - 1))]
        assert len(dup) == 1
        g = FC.point_class_fleet(big, dynamic=False)
        for t, u in zip(f.tables, g.tables):
            assert t.ax == u.ax and t.ay == u.ay and not any(u.dynamic)
        assert any(any(t.dynamic) for t in f.tables)
        np.testing.assert_array_equal(f.batch.x, g.batch.x)


@pytest.mark.parametrize("mode", [2, 3])
@pytest.mark.parametrize("big", BIG_ROWS)
def test_class_filter_drops_and_keeps_as_intended(oracle, cases, big, mode):
    f, sigs = cases[big, mode]
    for s in FC.DROPS_A_CLASS:
        idx, sig = sigs[s]
        keep, valid, reas = oracle.filter_equivalence_classes(mode, sig, THRESHOLD, -1, 1)
        assert valid.all() and reas.all()
        assert 2 <= keep.sum() < len(idx), (s, keep)
    for s, k in FC.KEEPS_TWO_OF_BEST.items():
        idx, sig = sigs[s]
        one, _, _ = oracle.filter_equivalence_classes(mode, sig, THRESHOLD, k, 1)
        two, _, _ = oracle.filter_equivalence_classes(mode, sig, THRESHOLD, k, 2)
        assert two.sum() == one.sum() + 1 and two[k] == 1 and (two >= one).all(), (s, one, two)
    for s in range(f.n_scenes):   # every signature of the fleet is usable
        idx, sig = sigs[s]
        assert np.isfinite(sig).all()


@pytest.mark.parametrize("big", BIG_ROWS[:1])
def test_detour_rule_drops_as_intended(oracle, big):
    f = FC.point_class_fleet(big)
    for s, (kb, kd) in FC.LOSES_A_DETOUR.items():
        sub, idx = f.scene_batch(s)
        ones = np.ones(len(idx), np.int32)
        keep = oracle.filter_detours(f.cfg, sub, ones, kb, ones)
        assert keep[kd] == 0 and keep[kb] == 1 and keep.sum() == len(idx) - 1, (s, keep)
        notopt = ones.copy(); notopt[(kb + 1) % len(idx)] = 0       # a band that was never optimised goes as well
        assert oracle.filter_detours(f.cfg, sub, ones, kb, notopt)[(kb + 1) % len(idx)] == 0
        np.testing.assert_array_equal(oracle.filter_detours(f.cfg, sub, ones, -1, ones), ones)   # no best: nothing happens


@pytest.mark.parametrize("big", BIG_ROWS)
def test_3d_decisions_are_separated(cases, big):
    f, sigs = cases[big, 3]
    for s, (idx, sig) in enumerate(sigs):
        a = np.abs(sig)
        assert (np.abs(a - THRESHOLD) > 1e-9).all() and (np.abs(a - 1.0) > 1e-9).all(), s
        for i in range(len(idx)):
            for j in range(i + 1, len(idx)):
                decides = (a[i] >= THRESHOLD) & (a[j] >= THRESHOLD)
                assert (a[i][decides] > 1e-9).all() and (a[j][decides] > 1e-9).all(), (s, i, j)


@pytest.mark.parametrize("big", BIG_ROWS)
def test_2d_decisions_are_separated(cases, big):
    f, sigs = cases[big, 2]
    for s, (idx, sig) in enumerate(sigs):
        if not idx:
            continue
        margin = 1e-8 * np.abs(sig).max()
        for i in range(len(idx)):
            for j in range(i + 1, len(idx)):
                d = np.abs(sig[i] - sig[j])
                assert (np.abs(d - THRESHOLD) > margin).all(), (s, i, j, d, margin)
