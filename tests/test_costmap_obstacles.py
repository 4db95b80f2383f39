"""The costmap's point obstacles (TebLocalPlannerROS::updateObstacleContainerWithCostmap, reference
src/teb_local_planner_ros.cpp:478-504): the restatement the GPU tests compare against, its hand-worked answers, and the CPU-side parts
of teb_amd_set_obstacles_from_costmap (export, argument check, configuration defaults). No GPU needed."""
import ctypes as C
import math

import numpy as np

from teb_local_planner_amd import _abi, planner
from teb_local_planner_amd.config import TebConfig

LETHAL_OBSTACLE = 254   # costmap_2d/cost_values.h


def reference_costmap_obstacles(cells, res, ox, oy, pose, dist):
    """(xs, ys) of the point obstacles updateObstacleContainerWithCostmap appends, in its order.

    cells: uint8 [size_y, size_x] (costmap_2d's cells[my * size_x + mx]). The reference loops mx = 0 .. size_x - 2 outside and
    my = 0 .. size_y - 2 inside (the last column and row are never visited), keeps cells whose cost == LETHAL_OBSTACLE, places them at
    Costmap2D::mapToWorld (origin + (m + 0.5) * resolution) and skips those with obs_dir.dot(robot_orient) < 0 and
    obs_dir.norm() > dist, robot_orient = (cos theta, sin theta) (PoseSE2::orientationUnitVec, pose_se2.h:215). Element-wise float64:
    plain products and sums, correctly rounded sqrt - Eigen's dot / norm of a Vector2d."""
    cells = np.asarray(cells, dtype=np.uint8)
    sy, sx = cells.shape
    if sx < 2 or sy < 2:
        return np.zeros(0), np.zeros(0)
    mx, my = np.nonzero(cells[:sy - 1, :sx - 1].T == LETHAL_OBSTACLE)   # row-major over (mx, my): mx outer, my inner
    wx = ox + (mx.astype(np.float64) + 0.5) * res
    wy = oy + (my.astype(np.float64) + 0.5) * res
    c, s = math.cos(pose[2]), math.sin(pose[2])
    dx, dy = wx - pose[0], wy - pose[1]
    skip = (dx * c + dy * s < 0) & (np.sqrt(dx * dx + dy * dy) > dist)
    return wx[~skip], wy[~skip]


def _loop_restatement(cells, res, ox, oy, pose, dist):
    """The reference's loop, one cell at a time."""
    sy, sx = cells.shape
    c, s = math.cos(pose[2]), math.sin(pose[2])
    xs, ys = [], []
    for i in range(sx - 1):
        for j in range(sy - 1):
            if cells[j, i] == LETHAL_OBSTACLE:
                wx, wy = ox + (i + 0.5) * res, oy + (j + 0.5) * res
                dx, dy = wx - pose[0], wy - pose[1]
                if dx * c + dy * s < 0 and math.sqrt(dx * dx + dy * dy) > dist:
                    continue
                xs.append(wx); ys.append(wy)
    return np.array(xs), np.array(ys)


def test_3x3_last_row_and_column_skipped_mx_major():
    cells = np.zeros((3, 3), np.uint8)   # [my, mx]
    cells[0, 1] = 254                    # (mx 1, my 0)
    cells[1, 0] = 254                    # (mx 0, my 1): comes first, the table is mx-major
    cells[0, 2] = 254                    # last column: never visited
    cells[2, 0] = 254                    # last row: never visited
    cells[2, 2] = 254
    cells[1, 1] = 253                    # INSCRIBED_INFLATED_OBSTACLE: not a point obstacle
    cells[0, 0] = 255                    # NO_INFORMATION: not a point obstacle
    xs, ys = reference_costmap_obstacles(cells, 1.0, 0.0, 0.0, (0.0, 0.0, 0.0), 100.0)
    assert xs.tolist() == [0.5, 1.5] and ys.tolist() == [1.5, 0.5]


def test_4x5_behind_filter_drops_only_far_and_behind():
    # size_x 4, size_y 5, resolution 0.5, origin (-1, 2): centres x -0.75, -0.25, 0.25 (column 3 unvisited), y 2.25 .. 3.75 (row 4
    # unvisited). Robot at (0, 3) facing +x, dist 0.6.
    cells = np.zeros((5, 4), np.uint8)
    cells[1, 0] = 254   # (-0.75, 2.75): behind, norm 0.79 > 0.6 -> dropped
    cells[2, 1] = 254   # (-0.25, 3.25): behind, norm 0.35      -> kept
    cells[3, 2] = 254   # ( 0.25, 3.75): ahead,  norm 0.79      -> kept
    cells[0, 2] = 254   # ( 0.25, 2.25): ahead                  -> kept
    cells[1, 3] = 254   # last column
    cells[4, 1] = 254   # last row
    cells[3, 0] = 253
    cells[0, 1] = 255
    pose = (0.0, 3.0, 0.0)
    xs, ys = reference_costmap_obstacles(cells, 0.5, -1.0, 2.0, pose, 0.6)
    assert list(zip(xs.tolist(), ys.tolist())) == [(-0.25, 3.25), (0.25, 2.25), (0.25, 3.75)]
    xs, ys = reference_costmap_obstacles(cells, 0.5, -1.0, 2.0, pose, 1.0)    # the far-behind cell is now near enough
    assert list(zip(xs.tolist(), ys.tolist())) == [(-0.75, 2.75), (-0.25, 3.25), (0.25, 2.25), (0.25, 3.75)]
    xs, ys = reference_costmap_obstacles(cells, 0.5, -1.0, 2.0, pose, -1.0)   # negative distance: every cell behind goes
    assert list(zip(xs.tolist(), ys.tolist())) == [(0.25, 2.25), (0.25, 3.75)]
    assert reference_costmap_obstacles(cells[:1], 0.5, -1.0, 2.0, pose, 1.0)[0].size == 0      # size_y == 1
    assert reference_costmap_obstacles(cells[:, :1], 0.5, -1.0, 2.0, pose, 1.0)[0].size == 0   # size_x == 1


def test_vectorised_restatement_equals_the_loop():
    rng = np.random.default_rng(5)
    for _ in range(20):
        sy, sx = (int(v) for v in rng.integers(1, 40, 2))
        cells = rng.choice(np.array([0, 100, 253, 254, 255], np.uint8), size=(sy, sx), p=[0.5, 0.1, 0.1, 0.2, 0.1])
        res, ox, oy = rng.uniform(0.01, 0.2), rng.uniform(-3, 1), rng.uniform(-3, 1)
        pose = (rng.uniform(-2, 3), rng.uniform(-2, 3), rng.uniform(-math.pi, math.pi))
        dist = float(rng.choice([-1.0, 0.0, 0.5, 1.5, 100.0]))
        got = reference_costmap_obstacles(cells, res, ox, oy, pose, dist)
        want = _loop_restatement(cells, res, ox, oy, pose, dist)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def test_library_exports_the_entry_point_and_rejects_a_null_handle():
    L = planner.lib()
    assert hasattr(L, "teb_amd_set_obstacles_from_costmap")
    pose = _abi.f64([0.0, 0.0, 0.0])
    n = C.c_int32(-7)
    rc = L.teb_amd_set_obstacles_from_costmap(None, _abi._ptr(pose, C.c_double), 1.5, None, C.byref(n), None, None, 0)
    assert rc == _abi.ERR_INVALID_ARG
    assert n.value == -7   # nothing counted, nothing written


def test_config_carries_the_reference_defaults():
    o = TebConfig().obstacles
    assert o.include_costmap_obstacles is True and o.costmap_obstacles_behind_robot_dist == 1.5   # teb_config.h:306-307
    assert not hasattr(_abi.Config(), "include_costmap_obstacles")   # host-side fields: teb_amd_config_t is unchanged
    TebConfig().to_c()
