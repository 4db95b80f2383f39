"""The two signature sets of a handle on the MI355X (csrc/teb_hcp_host.hpp, SignatureSet): the single scene's, which a compaction
gathers with its bands, and the scene set's, which a compaction clears - and neither compute call touches the other's set.

Small on purpose: 3 scenes x 2 - 3 bands x 12 poses x 4 obstacles, HSignature (2-D) and HSignature3d (3-D). Where two bands must fall
into one class they are copies of each other: equal rows are equal classes whatever the geometry."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import fleet_cases  # noqa: E402

from teb_local_planner_amd import _abi, planner  # noqa: E402

pytestmark = pytest.mark.gpu

THRESHOLD, PRESCALER = 0.1, 1.0
BAND_FIELDS = ("n", "x", "y", "theta", "dt", "has_vel_start", "vel_start", "has_vel_goal", "vel_goal", "prefer_rotdir", "via_points_enabled")


def _fleet(mode):
    f = fleet_cases.point_fleet(314, n_scenes=3, stride=16, bands=(2, 3), poses=12, obstacles=4)
    f.cfg.obstacles.include_dynamic_obstacles = mode == 3
    return f


def _solver(f, count):
    mo, mv, mw = f.capacities()
    return planner.TebBatchSolver(f.cfg, count, f.batch.stride, mo, mv, mw)


def _refused(call, *words):
    with pytest.raises(planner.TebAmdError) as e:
        call()
    assert e.value.code == _abi.ERR_INVALID_ARG and all(w in str(e.value) for w in words), str(e.value)


@pytest.mark.parametrize("mode", [2, 3])
def test_single_scene_signatures_survive_a_compaction(mode):
    f = _fleet(mode)
    src = f.batch
    assert src.count >= 3
    batch = _abi.TebBatchHost(5, src.stride)   # bands A B A C B: bands 2 and 4 are copies of bands 0 and 1
    for k, b in enumerate((0, 1, 0, 2, 1)):
        for fld in BAND_FIELDS:
            getattr(batch, fld)[k] = getattr(src, fld)[b]
    s = _solver(f, 5)
    s.set_obstacles(f.tables[0]); s.upload(batch)
    s.h_signatures(PRESCALER, values=False)
    keep = np.array([1, 1, 0, 1, 1], np.int32)
    n, new_best = s.compact_bands(keep, 4)   # 4 <-> 0, then band 2 leaves: B B C A
    assert (n, new_best) == (4, 0)
    got = s.filter_equivalence_classes(THRESHOLD, new_best, 1)   # no recompute: the gathered rows
    moved = s.download(_abi.TebBatchHost(4, src.stride))
    for k, b in enumerate((4, 1, 3, 0)):
        assert int(moved.n[k]) == int(batch.n[b])
        np.testing.assert_array_equal(moved.get_teb(k)[0], batch.get_teb(b)[0])
    fresh = _solver(f, 5)
    fresh.set_obstacles(f.tables[0]); fresh.upload(moved)
    fresh.h_signatures(PRESCALER, values=False)
    want = fresh.filter_equivalence_classes(THRESHOLD, new_best, 1)
    for name, u, v in zip(("keep", "valid", "reasonable"), got, want):
        np.testing.assert_array_equal(u, v, err_msg=name)
    assert got[0][0] == 1 and got[0][1] == 0 and got[1].all()   # the copy of the best band falls into its class
    fresh.close()
    s.close()
    # the same sequence on a scene set: its signatures are computed again after a compaction
    t = _solver(f, f.batch.count)
    t.set_scenes(f.tables, f.vias); t.set_band_scenes(f.scene_of); t.upload(f.batch)
    t.h_signatures_per_scene(PRESCALER, values=False)
    keep = np.ones(f.batch.count, np.int32); keep[f.bands_of(0)[0]] = 0
    best = np.array([f.bands_of(sc)[-1] for sc in range(3)], np.int32)
    n, new_best = t.compact_bands_per_scene(keep, best)
    assert n == f.batch.count - 1 and (new_best >= 0).all()
    _refused(lambda: t.filter_equivalence_classes_per_scene(THRESHOLD, new_best, 1), "call teb_amd_compute_h_signatures_per_scene first")
    t.close()


@pytest.mark.parametrize("mode", [2, 3])
def test_the_two_signature_sets_do_not_see_each_other(mode):
    f = _fleet(mode)
    s = _solver(f, f.batch.count)
    s.set_obstacles(f.tables[0]); s.upload(f.batch)   # the single scene: every band against table 0
    s.set_scenes(f.tables, f.vias); s.set_band_scenes(f.scene_of)
    s.h_signatures_per_scene(PRESCALER, values=False)
    of_set = s.filter_equivalence_classes_per_scene(THRESHOLD, None, 1)
    s.clear_scenes()
    _refused(lambda: s.filter_equivalence_classes(THRESHOLD, -1, 1), "call teb_amd_compute_h_signatures first")   # nothing of the set's
    s.h_signatures(PRESCALER, values=False)
    of_single = s.filter_equivalence_classes(THRESHOLD, -1, 1)
    s.set_scenes(f.tables, f.vias)
    _refused(lambda: s.filter_equivalence_classes_per_scene(THRESHOLD, None, 1), "call teb_amd_compute_h_signatures_per_scene first")   # nothing of the single scene's
    s.h_signatures_per_scene(PRESCALER, values=False)
    for u, v in zip(s.filter_equivalence_classes_per_scene(THRESHOLD, None, 1), of_set):
        np.testing.assert_array_equal(u, v)
    s.clear_scenes()   # the per-scene compute call left the single scene's signatures alone: no recompute
    for u, v in zip(s.filter_equivalence_classes(THRESHOLD, -1, 1), of_single):
        np.testing.assert_array_equal(u, v)
    s.close()
