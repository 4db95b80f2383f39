"""The fixtures of tests/fleet_tick_cases.py on the CPU: they exercise what they are meant to exercise, and what the GPU tests expect of
them comes from the oracle (pinned on the reference) and the restatement of tests/test_costmap_obstacles.py. The Python surface of the
per-scene calls is checked as far as no GPU is needed. No GPU."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import feasibility_cases  # noqa: E402
import fleet_tick_cases as FT  # noqa: E402
from test_costmap_obstacles import _loop_restatement, reference_costmap_obstacles  # noqa: E402
from teb_local_planner_amd import _abi, planner  # noqa: E402

NEW_SYMBOLS = ("teb_amd_set_costmaps", "teb_amd_set_scenes_from_costmaps", "teb_amd_is_trajectory_feasible_per_scene",
               "teb_amd_update_and_prune_per_scene", "teb_amd_get_velocity_commands")


def test_library_exports_the_calls_and_rejects_a_null_handle():
    L = planner.lib()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name), name
    assert L.teb_amd_set_costmaps(None, 0, None, None, None, None, None, None) == _abi.ERR_INVALID_ARG
    assert L.teb_amd_set_scenes_from_costmaps(None, 1, None, 1.5, None, None, None, None, None, None, None, 0) == _abi.ERR_INVALID_ARG
    assert L.teb_amd_is_trajectory_feasible_per_scene(None, None, 0, None, None, 0.1, 0.1, -1, -1.0, None, None) == _abi.ERR_INVALID_ARG
    assert L.teb_amd_update_and_prune_per_scene(None, None, None, 3, None, None) == _abi.ERR_INVALID_ARG
    assert L.teb_amd_get_velocity_commands(None, 0, None, 1, 0, None, None) == _abi.ERR_INVALID_ARG
    for name in ("set_costmaps", "set_scenes_from_costmaps", "is_trajectory_feasible_per_scene", "update_and_prune_per_scene", "velocity_commands"):
        assert callable(getattr(planner.TebBatchSolver, name))
    for name in ("isTrajectoryFeasible", "hasDiverged", "getVelocityCommands", "updateAllTEBs"):
        assert callable(getattr(planner.FleetHomotopyClassPlanner, name))


def test_table_sets_hold_the_shapes_they_are_meant_to():
    sets = FT.table_sets()
    assert sorted(t.n_scenes for t in sets) == [1, 3, 3, 6]
    assert sorted(t.dist for t in sets) == [-1.0, 0.0, 1.5, 100.0]
    rule = {(sx, sy): FT.lane_rule(sx, sy) for t in sets for sx, sy in FT.SET_SHAPES[t.name]}
    assert rule[(1, 37)][4] == 0 and rule[(41, 1)][4] == 0                     # no interior columns / rows
    assert rule[(2, 2)][4] == 1
    assert rule[(65, 17)][4] == 256 and rule[(66, 17)][4] == 260               # one workgroup exactly / two workgroups
    assert rule[(401, 700)][2] == 8 and rule[(120, 120)][2] == 4 and rule[(63, 65)][2] == 4
    assert rule[(401, 700)][4] <= 65536 < 400 * ((699 + 3) // 4)
    six = FT.table_set("six")
    assert {FT.lane_rule(g.size_x, g.size_y)[2] for g in six.grids} == {4, 8}  # chunk 8 beside chunk-4 scenes in ONE set
    for t in sets:
        assert len(t.scene_of) == t.batch.count and set(t.scene_of) == set(range(t.n_scenes))
        kinds = set()
        for s, g in enumerate(t.grids):
            assert (g.size_x, g.size_y) == FT.SET_SHAPES[t.name][s]
            xs, ys = reference_costmap_obstacles(g.cells, g.resolution, g.origin_x, g.origin_y, t.poses[s], t.dist)
            if g.size_x * g.size_y <= 63 * 65:
                lx, ly = _loop_restatement(g.cells, g.resolution, g.origin_x, g.origin_y, t.poses[s], t.dist)
                assert np.array_equal(xs, lx) and np.array_equal(ys, ly)
            if s in FT.SET_FREE[t.name]:
                assert not (g.cells == 254).any() and len(xs) == 0
            elif min(g.size_x, g.size_y) < 2:
                assert (g.cells == 254).any() and len(xs) == 0           # lethal cells, but none the reference visits
            else:
                assert 1 <= len(xs) <= 40
            if t.customs[s] is not None:
                kinds |= set(t.customs[s].type)
        if t.name == "six":
            assert kinds == {_abi.OBST_POINT, _abi.OBST_CIRCULAR, _abi.OBST_LINE, _abi.OBST_PILL, _abi.OBST_POLYGON}
            assert any(c is None for c in t.customs)
            assert FT.SET_FREE["six"] == [5] and t.n_scenes == 6              # an all-free grid as the last scene
    assert FT.SET_FREE["three"] == [1]                                        # ... and as the middle scene
    # the behind filter drops something at 0 and at 1.5, nothing at 100 and everything behind at -1
    three, far = FT.table_set("three"), FT.table_set("three_far")
    n0 = sum(len(reference_costmap_obstacles(g.cells, g.resolution, g.origin_x, g.origin_y, three.poses[s], 0.0)[0]) for s, g in enumerate(three.grids))
    n100 = sum(len(reference_costmap_obstacles(g.cells, g.resolution, g.origin_x, g.origin_y, far.poses[s], 100.0)[0]) for s, g in enumerate(far.grids))
    assert n0 < n100


def test_concat_table_is_the_points_then_the_custom_rows():
    c = FT.custom_mixed(1.0, 2.0)
    t = FT.concat_table([0.5, 0.25], [1.5, 1.75], c)
    assert len(t) == 2 + len(c) and t.type[:2] == [_abi.OBST_POINT] * 2 and t.type[2:] == c.type
    assert t.vert_offset == [0, 0] + c.vert_offset and t.vert_x == c.vert_x
    assert len(FT.concat_table([], [], None)) == 0


def test_feasibility_fleet_against_the_oracle(oracle):
    f = FT.feasibility_fleet()
    assert any(s % 3 == 0 for s in FT.FEAS_SEEDS) and any(s % 7 == 3 for s in FT.FEAS_SEEDS) and len(FT.FEAS_SEEDS) == 8
    ns = len(f.grids)
    assert f.batch.count == 2 * ns and all(f.scene_of[f.bands[s]] == s and f.scene_of[f.decoys[s]] == s for s in range(ns))
    assert all(f.bands[s] > f.decoys[s] for s in range(ns))                   # the SECOND band of every scene is the one checked
    verdicts = []
    for fp in feasibility_cases.FOOTPRINTS.values():
        for (inscribed, ang, look, dist) in FT.FEAS_PARAMS:
            for s in range(ns):
                a = oracle.is_trajectory_feasible(f.batch, int(f.bands[s]), f.grids[s], fp, inscribed, ang, look, dist)
                b = oracle.is_trajectory_feasible(f.singles[s], 0, f.grids[s], fp, inscribed, ang, look, dist)
                assert a == b                                                  # the band is the case's band, bit for bit
                verdicts.append(a)
    assert any(v[0] for v in verdicts) and any(not v[0] for v in verdicts)
    assert any(v[1] > 0 for v in verdicts if not v[0])                        # a collision that is not the very first test


def test_prune_fleet_against_the_oracle(oracle):
    f = FT.prune_fleet()
    ns = len(FT.PRUNE_COUNTS)
    assert f.batch.count == sum(FT.PRUNE_COUNTS) and [int((f.scene_of == s).sum()) for s in range(ns)] == list(FT.PRUNE_COUNTS)
    assert any(f.scene_of[b] != f.scene_of[b + 1] for b in range(f.batch.count - 1))       # interleaved
    assert 0 < f.mask.sum() < ns
    n = sorted(int(v) for v in f.batch.n)
    ms = FT.PRUNE_MIN_SAMPLES
    assert {ms, ms + 1, ms + 2} <= set(n) and {255, 256, 257} <= set(n) and max(n) <= FT.PRUNE_STRIDE
    deleted = {s: [] for s in range(ns)}
    for b in range(f.batch.count):
        s = int(f.scene_of[b])
        x, y, th, dt = f.batch.get_teb(b)
        for st, gl in ((f.starts[s], f.goals[s]), (f.starts[s], None), (None, f.goals[s])):
            wx, wy, wth, wdt = oracle.update_and_prune(x, y, th, dt, st, gl, ms)
            if st is not None:
                assert (wx[0], wy[0], wth[0]) == tuple(st)
                if gl is not None:
                    deleted[s].append(len(x) - len(wx))
            else:
                assert len(wx) == len(x)
            if gl is not None:
                assert (wx[-1], wy[-1], wth[-1]) == tuple(gl)
    assert all(d == 0 for d in deleted[0])                                     # a scene whose prune deletes none
    assert max(deleted[2]) == 3 and max(deleted[3]) == 10 and max(deleted[4]) == 10   # 3 poses, and the cap of 10 for a start further on
    assert any(d > 0 for s in range(ns) for d in deleted[s])


def test_commands_of_the_prune_fleet_come_from_the_oracle(oracle):
    f = FT.prune_fleet()
    oks = []
    for b in range(f.batch.count):
        for la, prevent in ((1, 0), (4, 2)):
            w = oracle.consumers(f.cfg, f.batch, b, la, prevent)
            assert np.all(np.isfinite(w["cmd"]))
            oks.append(bool(w["ok"]))
    assert any(oks)


def test_python_argument_checks_need_no_device():
    """Shape errors of the wrappers are ValueErrors before the library is entered."""
    s = planner.TebBatchSolver.__new__(planner.TebBatchSolver)
    s._h = C.c_void_p(None); s._n_scenes = 3; s.max_obstacles = 8; s.count = 0
    with pytest.raises(ValueError):
        s.update_and_prune_per_scene(np.zeros((2, 3)), None)
    with pytest.raises(ValueError):
        s.update_and_prune_per_scene(np.zeros((3, 2)), None)
    with pytest.raises(ValueError):
        s.is_trajectory_feasible_per_scene([0, 1], [(0.0, 0.0)], 0.2)
    with pytest.raises(ValueError):
        s.set_scenes_from_costmaps(np.zeros((3, 3)), 1.5, custom=[None, None])
    with pytest.raises(planner.TebAmdError) as e:                              # the null handle reaches the library and is refused there
        s.velocity_commands([0, -1])
    assert e.value.code == _abi.ERR_INVALID_ARG
