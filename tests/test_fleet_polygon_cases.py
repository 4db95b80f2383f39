"""The polygon route of the costmap per scene (teb_amd_set_scenes_from_costmap_polygons) on the CPU: the symbol and its ABI, and the
fixtures of tests/fleet_polygon_cases.py held to the restatement - conditions on the fixtures, checked here, so that the GPU tests
(tests/test_gpu_fleet_polygons.py) cannot pass vacuously."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import costmap_polygon_cases as CP  # noqa: E402
import fleet_polygon_cases as FP  # noqa: E402
from test_costmap_obstacles import reference_costmap_obstacles  # noqa: E402
from teb_local_planner_amd import _abi, planner  # noqa: E402


def test_the_library_exports_the_call_and_keeps_its_abi():
    L = planner.lib()
    assert hasattr(L, "teb_amd_set_scenes_from_costmap_polygons")
    assert L.teb_amd_abi_version() == 3
    tiles = _abi.i32([8])
    pose = _abi.f64([0.0, 0.0, 0.0])
    rc = L.teb_amd_set_scenes_from_costmap_polygons(None, 1, _abi._ptr(pose, C.c_double), 1.5, _abi._ptr(tiles, C.c_int32), None, None, None, None,
                                                    None, None, None, None, None, 0, 0)
    assert rc == _abi.ERR_INVALID_ARG


def test_the_shapes_are_the_ones_the_indexing_can_go_wrong_at():
    assert FP.block_rule(63, 65, 8)[3:] == (8, 1, 8)                          # one block per tile column
    edges = [FP.block_rule(*q) for q in FP.SET_SHAPES["edges"]]
    assert [e[5] for e in edges] == [0, 0, 6, 1, 40, 0]                        # no blocks twice at the front and at the end
    assert edges[2][2:5] == (1, 3, 3) and edges[2][0] % 64 == 1 and edges[2][1] % 64 == 1   # k = 1, nby = 3, clipped tiles
    assert edges[3][:2] == (1, 1)                                              # one visited cell under T = 64
    assert edges[4][2] == 455 and 4096 % 9 != 0
    assert [i for i, e in enumerate(edges) if e[5] == 0] == FP.SET_NO_BLOCKS["edges"]
    mixed = [FP.block_rule(*q) for q in FP.SET_SHAPES["mixed"]]
    assert all(m[5] > 0 for m in mixed) and len({m[5] for m in mixed}) > 1


@pytest.mark.parametrize("name", list(FP.SET_SHAPES))
def test_every_set_holds_what_the_gpu_tests_rely_on(name):
    t = FP.polygon_set(name)
    rows = FP.expected_rows(name)
    assert len(rows) == t.n_scenes == len(FP.SET_SHAPES[name]) == len(t.tiles)
    kinds = set()
    for s, (types, off, xs, ys) in enumerate(rows):
        g = t.grids[s]
        assert g.cells.shape == (FP.SET_SHAPES[name][s][1], FP.SET_SHAPES[name][s][0])
        assert (g.cells == 253).any() or g.cells.size < 4
        assert (g.cells == 255).any() or g.cells.size < 4
        assert g.origin_x < t.poses[s][0] < g.origin_x + g.cells.shape[1] * g.resolution     # the robot stands inside its grid
        assert g.origin_y < t.poses[s][1] < g.origin_y + g.cells.shape[0] * g.resolution
        assert len(off) == len(types) + 1 and off[-1] == len(xs) == len(ys)
        if s in FP.SET_NO_BLOCKS[name] or s in FP.SET_FREE[name]:
            assert len(types) == 0, s
        else:
            assert len(types) >= 1, s
        if s in FP.SET_FREE[name]:
            assert FP.block_rule(*FP.SET_SHAPES[name][s])[5] > 0 and not (g.cells == 254).any()
        kinds |= set(int(k) for k in types)
        # with T = 1 the rows are the point route's points
        _, off1, x1, y1 = CP.reference_costmap_polygons(g.cells, g.resolution, g.origin_x, g.origin_y, t.poses[s], t.dist, 1)
        px, py = reference_costmap_obstacles(g.cells, g.resolution, g.origin_x, g.origin_y, t.poses[s], t.dist)
        assert np.array_equal(off1, np.arange(len(px) + 1))
        assert np.array_equal(x1.view(np.uint64), px.view(np.uint64)) and np.array_equal(y1.view(np.uint64), py.view(np.uint64))
    if name != "one":
        assert kinds == {CP.POINT, CP.LINE, CP.POLYGON}
    # the behind-robot filter bites where the set has a finite distance, and a turned heading changes the rows
    if name == "edges":
        s = 4
        g = t.grids[s]
        every = CP.reference_costmap_polygons(g.cells, g.resolution, g.origin_x, g.origin_y, t.poses[s], float("inf"), int(t.tiles[s]))
        assert len(every[0]) > len(rows[s][0])
        assert len(FP.expected_rows(name, 2.5)[s][2]) != len(rows[s][2])
    # custom rows of both kinds and none; one or two bands per scene
    assert any(c is None for c in t.customs) or name == "one"
    for s in range(t.n_scenes):
        assert 1 <= int((t.scene_of == s).sum()) <= 2
    assert ((t.batch.n >= 12) & (t.batch.n <= 20)).all()


def test_concat_table_is_the_converted_rows_then_the_custom_rows():
    t = FP.polygon_set("mixed")
    rows = FP.expected_rows("mixed")
    tab = FP.concat_table(rows[0], t.customs[0])
    n, c = len(rows[0][0]), t.customs[0]
    assert len(tab) == n + len(c) and tab.type[:n] == rows[0][0].tolist() and tab.type[n:] == c.type
    assert len(tab.vert_offset) == len(tab) + 1 and tab.vert_offset[-1] == len(tab.vert_x) == len(tab.vert_y)
    assert tab.vert_x[tab.vert_offset[n]:] == c.vert_x
