"""Fixtures for both ends of a fleet tick per scene (tests/test_fleet_tick_cases.py holds them to the oracle and the restatement on the
CPU, tests/test_gpu_fleet_tick.py runs them on the device):

  table_sets()        costmap sets of 1, 3 and 6 grids of different sizes with robot poses, a behind-robot distance, custom rows and
                      bands - what teb_amd_set_costmaps / teb_amd_set_scenes_from_costmaps get;
  feasibility_fleet() eight cases of tests/feasibility_cases.py, each as a scene with its own grid and two bands (a decoy first);
  prune_fleet()       5 scenes x 1 .. 4 bands, interleaved, with new starts / goals / start velocities per scene.

Everything is seeded and built once per process (functools.lru_cache); the tests do not change what they get."""
import functools

import numpy as np

from oracle.oracle_py import Costmap
from teb_local_planner_amd import _abi, scenes
from teb_local_planner_amd.config import TebConfig

import feasibility_cases

# ---- tables ----------------------------------------------------------------------------------------------------------------------
# (size_x, size_y) of every grid of a set; SET_FREE: the all-free grids; SET_CUSTOM: the scenes with custom rows
SET_SHAPES = {
    "one": [(63, 65)],
    "three": [(2, 2), (120, 120), (66, 17)],                                  # all-free grid in the middle
    "three_far": [(2, 2), (120, 120), (66, 17)],
    "six": [(1, 37), (65, 17), (41, 1), (401, 700), (120, 120), (63, 65)],    # all-free grid last; chunk 8 beside chunk-4 scenes
}
SET_DIST = {"one": -1.0, "three": 0.0, "three_far": 100.0, "six": 1.5}
SET_FREE = {"one": [], "three": [1], "three_far": [1], "six": [5]}
SET_CUSTOM = {"one": {0: "pointlike"}, "three": {}, "three_far": {2: "pointlike"}, "six": {0: "mixed", 3: "mixed", 4: "pointlike"}}
TABLE_STRIDE = 48


def lane_rule(size_x, size_y):
    """(ncols, nrows, chunk, nchunks, lanes) of teb_amd_set_obstacles_from_costmap on a grid: rows per lane = the smallest of 4, 8 .. 64
    that keeps the lanes within 64 K (include/teb_amd.h)."""
    ncols, nrows = size_x - 1, size_y - 1
    if ncols <= 0 or nrows <= 0:
        return 0, 0, 4, 0, 0
    chunk = 4
    while chunk < 64 and ncols * ((nrows + chunk - 1) // chunk) > 65536:
        chunk *= 2
    nchunks = (nrows + chunk - 1) // chunk
    return ncols, nrows, chunk, nchunks, ncols * nchunks


def custom_mixed(x0, y0):
    """a row of every obstacle class, two of them dynamic"""
    c = _abi.ObstacleTable()
    c.add_point(x0 + 1.5, y0 + 0.45)
    c.add_circle(x0 + 2.4, y0 + 0.9, 0.2)
    c.add_line(x0 + 2.0, y0 + 0.7, x0 + 2.8, y0 + 1.2)
    c.add_pill(x0 + 1.0, y0 - 0.9, x0 + 1.8, y0 - 1.1, 0.15)
    c.add_polygon([(x0 + 2.5, y0 - 0.5), (x0 + 3.1, y0 - 0.8), (x0 + 3.0, y0 - 0.2)])
    c.add_point(x0 + 2.0, y0 - 1.5, vel=(0.05, 0.12))
    c.add_circle(x0 + 3.0, y0 + 1.5, 0.15, vel=(-0.1, -0.1))
    return c


def custom_pointlike(x0, y0):
    c = _abi.ObstacleTable()
    c.add_point(x0 + 1.5, y0 + 0.45)
    c.add_circle(x0 + 2.4, y0 + 0.9, 0.2)
    c.add_point(x0 + 2.2, y0 - 0.6)
    return c


def concat_table(xs, ys, custom):
    """The table teb_amd_set_scenes gets for a scene: the cell points, then the custom rows (cells have no vertices)."""
    t = _abi.ObstacleTable()
    for x, y in zip(xs, ys):
        t.add_point(float(x), float(y))
    if custom is not None:
        for k in ("type", "ax", "ay", "bx", "by", "radius", "vx", "vy", "dynamic", "vert_x", "vert_y"):
            getattr(t, k).extend(getattr(custom, k))
        t.vert_offset.extend(custom.vert_offset[1:])
    return t


class TableSet:
    """cfg, grids [n] Costmap, poses [n, 3], dist, customs [n] ObstacleTable or None, batch + scene_of (1 .. 2 bands per scene)"""

    def __init__(self, name, cfg, grids, poses, dist, customs, batch, scene_of):
        self.name, self.cfg, self.grids, self.poses, self.dist, self.customs = name, cfg, grids, poses, dist, customs
        self.batch, self.scene_of = batch, np.asarray(scene_of, np.int32)

    @property
    def n_scenes(self):
        return len(self.grids)


@functools.lru_cache(maxsize=None)
def table_set(name):
    shapes = SET_SHAPES[name]
    rng = np.random.default_rng([4107, sorted(SET_SHAPES).index(name)])
    cfg = TebConfig()
    cfg.obstacles.include_dynamic_obstacles = True
    grids, poses, customs = [], [], []
    for s, (sx, sy) in enumerate(shapes):
        res = 0.05 if (sx, sy) == (120, 120) else float(rng.uniform(0.03, 0.12))
        ox, oy = float(rng.uniform(-20, 20)), float(rng.uniform(-20, 20))   # every robot somewhere else on the floor
        cells = rng.integers(0, 254, size=(sy, sx)).astype(np.uint8)      # every cost but lethal / unknown ...
        if cells.size >= 64:
            cells.reshape(-1)[rng.permutation(cells.size)[:3]] = 255      # ... a few unknown cells ...
        if s not in SET_FREE[name]:                                        # ... and about 40 lethal ones (fewer in the small grids)
            k = min(40, max(1, cells.size // 8))
            cells.reshape(-1)[rng.permutation(cells.size)[:k]] = 254
            if (sx, sy) == (2, 2):
                cells[0, 0] = 254                                          # the one cell the reference visits
        grids.append(Costmap(cells, res, ox, oy))
        # the robot inside its grid, looking along the bands (+x) with a little yaw
        poses.append((ox + 0.2 * sx * res, oy + 0.5 * sy * res, float(rng.uniform(-0.4, 0.4))))
        kind = SET_CUSTOM[name].get(s)
        customs.append(None if kind is None else (custom_mixed if kind == "mixed" else custom_pointlike)(poses[-1][0], poses[-1][1]))
    counts = [1 + (s % 2) for s in range(len(shapes))]
    scene_of = np.repeat(np.arange(len(shapes)), counts)
    rng.shuffle(scene_of)
    batch = _abi.TebBatchHost(len(scene_of), TABLE_STRIDE)
    for b, s in enumerate(scene_of):
        n = int(rng.integers(12, 21))
        px, py, th, dt = scenes.sine_band(n, 3.5, float(rng.uniform(-0.4, 0.4)), float(rng.integers(1, 3)), cfg.robot.max_vel_x)
        th = th + rng.normal(0.0, 2e-3, th.shape)
        batch.set_teb(b, px + poses[s][0], py + poses[s][1], th, dt)
    return TableSet(name, cfg, grids, np.array(poses), SET_DIST[name], customs, batch, scene_of)


def table_sets():
    return [table_set(k) for k in SET_SHAPES]


# ---- feasibility -----------------------------------------------------------------------------------------------------------------
FEAS_SEEDS = (0, 1, 3, 4, 6, 9, 10, 17)     # seed % 3 == 0: 0, 3, 6, 9 (interpolation); seed % 7 == 3: 3, 10, 17 (the map ends early)
FEAS_PARAMS = ((0.25, 0.3, -1, -1.0), (0.4, np.pi, 10, 4.0))   # (inscribed_radius, min_resolution_collision_check_angular, look_ahead_idx, lookahead distance)
FEAS_STRIDE = 128


class FeasFleet:
    """grids [8] Costmap, batch: band s (a straight decoy of scene s) and band 8 + (7 - s) (the band of case s), scene_of, bands [8]: the
    second band of every scene; singles [8]: the case's band as a batch of its own"""


@functools.lru_cache(maxsize=None)
def feasibility_fleet():
    f = FeasFleet()
    cases = [feasibility_cases.feasibility_case(seed) for seed in FEAS_SEEDS]
    ns = len(cases)
    f.grids = [c[1] for c in cases]
    f.singles = [c[0] for c in cases]
    f.batch = _abi.TebBatchHost(2 * ns, FEAS_STRIDE)
    f.scene_of = np.array(list(range(ns)) + list(range(ns - 1, -1, -1)), np.int32)
    f.bands = np.array([ns + (ns - 1 - s) for s in range(ns)], np.int32)
    for s, c in enumerate(cases):
        n = 5 + s
        f.batch.set_teb(s, np.linspace(0.0, 1.0 + s, n), np.full(n, 0.3), np.zeros(n), np.full(n - 1, 0.3))
        f.batch.set_teb(int(f.bands[s]), *c[0].get_teb(0))
    f.decoys = np.arange(ns, dtype=np.int32)
    return f


# ---- prune -----------------------------------------------------------------------------------------------------------------------
PRUNE_STRIDE = 320
PRUNE_MIN_SAMPLES = 3
PRUNE_COUNTS = (1, 2, 3, 4, 2)
# pose counts of the bands of every scene: either side of min_samples + 1 and of 256 poses (one 256-lane pass), and ordinary ones
PRUNE_POSES = ((40,), (3, 4), (255, 256, 257), (300, 5, 20, 64), (30, 6))
PRUNE_MOVE = (0, 1, 3, 14, 12)   # the new start of scene s lies at pose PRUNE_MOVE[s] of the scene's first band


class PruneFleet:
    """cfg, batch, scene_of (interleaved), starts / goals / vels [5, 3], mask [5]"""


@functools.lru_cache(maxsize=None)
def prune_fleet():
    f = PruneFleet()
    rng = np.random.default_rng(9103)
    f.cfg = TebConfig()
    ns = len(PRUNE_COUNTS)
    order = [(s, k) for s in range(ns) for k in range(PRUNE_COUNTS[s])]
    perm = rng.permutation(len(order))
    order = [order[i] for i in perm]
    f.scene_of = np.array([s for s, _ in order], np.int32)
    f.batch = _abi.TebBatchHost(len(order), PRUNE_STRIDE)
    origins = [(float(rng.uniform(-20, 20)), float(rng.uniform(-20, 20))) for _ in range(ns)]
    first = {}
    for b, (s, k) in enumerate(order):
        n = PRUNE_POSES[s][k]
        # the bands of a scene leave the same start along nearly the same line: the robot is ON all of them
        px, py, th, dt = scenes.sine_band(n, 0.1 * (n - 1) if n > 2 else 0.1, 0.05 * k, 1.0, f.cfg.robot.max_vel_x)
        f.batch.set_teb(b, px + origins[s][0], py + origins[s][1], th, dt)
        f.batch.has_vel_start[b] = int(rng.integers(0, 2))
        f.batch.vel_start[b] = rng.uniform(-0.2, 0.2, 3)
        if k == 0:
            first[s] = b
    f.starts = np.zeros((ns, 3)); f.goals = np.zeros((ns, 3))
    for s in range(ns):
        x, y, th, _ = f.batch.get_teb(first[s])
        i = min(PRUNE_MOVE[s], len(x) - 1)
        f.starts[s] = (x[i] + 1e-3, y[i] - 2e-3, th[i] + 0.01)
        f.goals[s] = (x[-1] + 0.05, y[-1] + 0.02, 0.1 * s)
    f.vels = rng.uniform(-0.3, 0.3, (ns, 3))
    f.mask = np.array([1, 0, 1, 1, 0], np.int32)
    return f
