"""isTrajectoryFeasible of the device (feasibility_kernel / feasibility_fleet_kernel, csrc/teb_feasibility.hpp) against the fixtures of
tests/golden/make_hp_feasibility.py: the op-by-op fp64 restatement of the reference's function and of the navigation stack's footprint
test, checked at 80 digits, against the reference planner's own function and against the CPU oracle, on cases built ON the thresholds
of every decision (tests/feasibility_threshold_cases.py; what the cases cover is asserted on the CPU in tests/test_hp_feasibility.py).

This file reads only the fixtures. Every case runs through set_costmap + is_trajectory_feasible with b = k for every band and, where
it has several bands, with b = -1; the two fleets run through set_costmaps + is_trajectory_feasible_per_scene beside single-scene
handles. The assertion is (feasible, first_infeasible) equal to the fixture: integer work, no tolerance. The refusals (65 footprint
vertices, 2^22 + 1 footprint tests) are asserted with their documented error codes.

Observed on an MI355X: 365 tests in 4.9 s, of which the case of exactly 2^22 footprint tests takes 1.9 s (one workgroup replays the
sample recurrence from the segment's first pose for each of its four million tests).
"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import hp_feasibility as HF  # noqa: E402  (unpack: no mpmath needed)

from teb_local_planner_amd import _abi, planner  # noqa: E402
from teb_local_planner_amd.config import TebConfig  # noqa: E402

pytestmark = pytest.mark.gpu

FAMILIES = ["cell", "codes", "raster", "interp", "look", "lanes", "fleet", "limits"]
REFUSED = (-9, -9)
_FIX = {}


def _family(fam):
    if fam not in _FIX:
        _FIX[fam] = HF.unpack(np.load(os.path.join(HERE, "golden", "hp_feasibility_%s.npz" % fam)))
    return _FIX[fam]


def _names():
    return [(fam, n) for fam in FAMILIES for n in _family(fam)]


def _batch(bands):
    batch = _abi.TebBatchHost(len(bands), max(max(len(b[0]) for b in bands), 4))
    for k, (x, y, th) in enumerate(bands):
        batch.set_teb(k, x, y, th, np.ones(len(x) - 1))
    return batch


def _args(fx):
    r, ang, look, dist = fx["params"]
    return [tuple(p) for p in fx["fp"]], float(r), float(ang), int(look), float(dist)


def _single(fx):
    s = planner.make_solver(TebConfig(), _abi.ObstacleTable(), [], _batch(fx["bands"]))
    res, ox, oy = fx["geom"]
    s.set_costmap(fx["cells"], res, ox, oy)
    return s


@pytest.mark.parametrize("fam,name", _names())
def test_every_case_band_by_band_and_as_a_batch(fam, name):
    fx = _family(fam)[name]
    want = [(bool(ok), int(first)) for ok, first in fx["expected"]]
    s = _single(fx)
    try:
        if tuple(fx["expected"][0]) == REFUSED:
            with pytest.raises(planner.TebAmdError) as e:
                s.is_trajectory_feasible(0, *_args(fx))
            assert e.value.code == _abi.ERR_CAPACITY
            return
        got = [s.is_trajectory_feasible(k, *_args(fx)) for k in range(len(want))]
        assert got == want, (name, [(k, g, w) for k, (g, w) in enumerate(zip(got, want)) if g != w])
        if len(want) > 1:
            ok, first = s.is_trajectory_feasible(-1, *_args(fx))
            assert [(bool(a), int(b)) for a, b in zip(ok, first)] == want, name
    finally:
        s.close()


@pytest.mark.parametrize("fleet", ["fleeta", "fleetb"])
def test_four_scenes_in_one_launch_equal_the_fixture_and_their_single_scene_handles(fleet):
    raw = np.load(os.path.join(HERE, "golden", "hp_feasibility_fleet.npz"))
    members, bands = [str(m) for m in raw["fleet_" + fleet]], raw["fleetbands_" + fleet]
    fxs = [_family("fleet")[m] for m in members]
    for fx in fxs[1:]:   # one launch shares footprint and parameters (but not the band and the grid)
        np.testing.assert_array_equal(fx["params"], fxs[0]["params"])
        np.testing.assert_array_equal(fx["fp"], fxs[0]["fp"])
    ns = len(members)
    batch = _batch([fx["bands"][0] for fx in fxs])
    s = planner.TebBatchSolver(TebConfig(), batch.count, batch.stride, 4, 4, 4)
    s.set_scenes([_abi.ObstacleTable() for _ in range(ns)])
    s.set_band_scenes(np.arange(ns, dtype=np.int32))
    s.upload(batch)
    from types import SimpleNamespace
    s.set_costmaps([SimpleNamespace(cells=fx["cells"], resolution=fx["geom"][0], origin_x=fx["geom"][1], origin_y=fx["geom"][2]) for fx in fxs])
    ok, first = s.is_trajectory_feasible_per_scene(bands, *_args(fxs[0]))
    s.close()
    answers = set()
    for k, fx in enumerate(fxs):
        want = (bool(fx["expected"][0][0]), int(fx["expected"][0][1]))
        one = _single(fx)
        assert one.is_trajectory_feasible(0, *_args(fx)) == want, members[k]
        one.close()
        answers.add(want)
        if bands[k] < 0:
            assert (ok[k], first[k]) == (-1, -1), members[k]
        else:
            assert (bool(ok[k]), int(first[k])) == want, members[k]
    assert len(answers) == ns and (bands < 0).sum() == (1 if fleet == "fleetb" else 0)


def test_a_footprint_of_65_vertices_is_refused():
    fx = _family("codes")["codes_nf64_free"]
    s = _single(fx)
    fp, r, ang, look, dist = _args(fx)
    assert len(fp) == 64 and s.is_trajectory_feasible(0, fp, r, ang, look, dist) == (True, -1)
    with pytest.raises(planner.TebAmdError) as e:
        s.is_trajectory_feasible(0, fp + [fp[0]], r, ang, look, dist)
    assert e.value.code == _abi.ERR_INVALID_ARG
    s.close()
