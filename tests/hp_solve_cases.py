"""Cases of tests/test_hp_solve.py and tests/test_gpu_hp_solve.py. NOT a test file.

A case is ONE band, one launch, one LM iteration (teb_autosize off, start and goal fixed, default weights): build(name) returns a dict
  cfg, obst, via, batch     the scene
  layout, options           the pinned layout ("cr" blocks in LDS, "band" band in LDS / hybrid solve, "bandg" band in HBM) and the
                            keyword arguments of _abi.Options for it
  n                         pose count
  min_k                     the accepted damping trial must be at least this one (2: a first trial is rejected - in the blocks layout
                            the H restore from the backup runs, with solver helpers the accepted step comes from a helper)
  helpers                   solver helpers asked for (speculative_trials)
Pose counts: the smallest at which each part of the round structure can go wrong -
  cr     3 (minimal system), 4, 5 (even / odd block padding), 16, 17, 32, 33, 64, 65, 129 (a level with E % 16 != 0 on either side of a
         power of two), 238 (the capacity)
  band   3, 5, 33, 65 (one level-0 round of 32 eliminations and the first block row beyond it), 128, 129, 130 (two rounds; block rows that
         enter the compact system uneliminated), 255 .. 258 (the workgroup's 256 lanes), 337 (the capacity)
  band + band_ldlt   5, 65, 257: the sequential cross-check solver
  bandg  5, 129, 257 (either side of the 64-block-row compact LDS copy), 338 (first size only this layout holds), 512, 513, 944 (capacity)

The scenes. The step is recovered from the states either side of the iteration, so the rounding of the state update, ulp(state) / 2,
is the measurement's noise: it must stay a small share of the metric's scale (hp_solve.noise_share <= 64 eps on every row, asserted in
tests/test_hp_solve.py). That asks for steps that are not small against the coordinates - step >~ coordinate / 128 on some variable of
every row - so every band is COMPACT and centred on the origin: a sine band resampled to SPACING = 0.1 m of arc between poses, whose
half periods multiply with the pose count so that it stays a snake inside +- 2 m x +- 2 m (ulp <= 2.2e-16; headings inside +- pi / 2
+ the perturbation: no wrap), and every inner pose is perturbed by a FIXED size (0.08 m in a seeded direction, 0.2 .. 0.4 rad, time
differences x 0.7 / 1.4) with signs + + - -, so that no stretch of the band starts near its optimum: the first step takes centimetres
and tenths of a radian everywhere (observed share <= 37 eps; with independent uniform draws in a +- 4 m box 150 .. 280 eps at n >= 129).
A handful of static and dynamic point obstacles beside the band keep obstacle rows active. One polygon-footprint scene per layout runs
the generic scene kind (the solve on the plain calling convention). The rejected-first-trial cases ("rough") perturb by independent
uniform draws instead: the linear model of the first trials is poor there (k = 2 .. 5 with the oracle, asserted on the CPU; share
<= 43 eps at their sizes). Several of the plain cases take k = 2 or 3 as well.
"""
import math

import numpy as np

from teb_local_planner_amd import scenes, _abi
from teb_local_planner_amd.config import RobotFootprintModel

from hp_linearize_cases import LAYOUT_INDEX  # noqa: F401  (the tests confirm the layout that ran with it)

SPACING = 0.1      # metres between consecutive poses of the unperturbed band
HALF_X = 2.0       # the band runs from x = -HALF_X to +HALF_X (shorter bands: less)
KICK_XY, KICK_THETA = 0.08, 0.4   # size of the seeded perturbation of every inner pose (metres, radians)
MAX_THETA = 2.6    # |heading| of every case stays below this, before and after the step (pi - 0.54: normalize_theta is the identity)

SIZES = {
    "cr": (3, 4, 5, 16, 17, 32, 33, 64, 65, 129, 238),
    "band": (3, 5, 33, 65, 128, 129, 130, 255, 256, 257, 258, 337),
    "band_ldlt": (5, 65, 257),
    "bandg": (5, 129, 257, 338, 512, 513, 944),
}
POLYGON = {"cr": 65, "band": 129, "bandg": 129}
# rejected first trial: layout -> (n, seed), found with the oracle (tests/test_hp_solve.py asserts k >= 2 for them)
REJECTED = {"cr": (65, 3), "band": (129, 3), "band_ldlt": (65, 3), "bandg": (257, 3)}
HELPERS = {"cr": (120, 208, 3), "band": (120, 288, 3)}   # n, stride (as tests/test_gpu_multi_cu.py), seed


def _snake(n):
    """(x, y) of the unperturbed band: y = A sin(pi h s) over x in [-X, X], about SPACING between poses"""
    length = SPACING * (n - 1)
    X = min(HALF_X, 0.5 * length)
    if length <= 2.4 * HALF_X:
        amp, h = 0.15 * 0.5 * length, 2.0
    else:
        h = 2.0 * math.ceil(length / (8.0 * HALF_X))   # half periods: each carries at most ~ 4 HALF_X of path
        amp = min(HALF_X, 0.45 * math.sqrt((length / h) ** 2 - (2 * X / h) ** 2))
    s = np.linspace(0.0, 1.0, 40 * n)
    fx, fy = 2 * X * s - X, amp * np.sin(math.pi * h * s)
    arc = np.concatenate([[0.0], np.cumsum(np.hypot(np.diff(fx), np.diff(fy)))])
    u = np.linspace(0.0, arc[-1], n)               # equal steps of arc length
    return np.interp(u, arc, fx), np.interp(u, arc, fy)


def scene(n, seed, footprint="point", rough=False, stride=None):
    cfg = scenes.TebConfig()
    cfg.trajectory.teb_autosize = False
    cfg.obstacles.include_dynamic_obstacles = True
    if footprint == "polygon":
        cfg.robot_model = RobotFootprintModel.polygon([(-0.2, -0.15), (0.4, -0.15), (0.4, 0.15), (-0.2, 0.15)])
    rng = np.random.default_rng(1000 * n + seed)
    px, py = _snake(n)
    th, dt = scenes._band_from_path(px, py, cfg.robot.max_vel_x, theta_goal=None)
    if rough:   # independent draws: the linear model of the first trial is poor, the trial is rejected
        px[1:-1] += rng.uniform(-0.03, 0.03, n - 2); py[1:-1] += rng.uniform(-0.03, 0.03, n - 2)
        th[1:-1] += rng.uniform(-0.15, 0.15, n - 2)
        dt = dt * rng.uniform(0.7, 1.5, n - 1)
    else:       # fixed sizes, signs + + - - (the kinematics residual reads theta_i + theta_i+1: + - + - would cancel in it)
        sign = np.where((np.arange(n - 2) // 2) % 2, -1.0, 1.0)
        phi = rng.uniform(0, 2 * math.pi, n - 2)
        px[1:-1] += KICK_XY * sign * np.cos(phi); py[1:-1] += KICK_XY * sign * np.sin(phi)
        th[1:-1] += KICK_THETA * sign * rng.uniform(0.5, 1.0, n - 2)
        dt = dt * np.where(np.arange(n - 1) % 2, 0.7, 1.4) * rng.uniform(0.85, 1.15, n - 1)
    batch = _abi.TebBatchHost(1, stride or max(96, n))
    batch.set_teb(0, px, py, th, dt)
    batch.has_vel_start[0] = 1; batch.vel_start[0] = (0.1, 0.0, 0.05)
    batch.has_vel_goal[0] = 1
    obst = _abi.ObstacleTable()
    t = np.concatenate([[0.0], np.cumsum(dt)])
    m = max(3, min(12, n // 8))
    for q, i in enumerate(np.linspace(0, n - 1, m + 2)[1:-1].astype(int)):   # beside pose i, alternating sides; every third one moves
        side = 1.0 if q % 2 else -1.0
        off = rng.uniform(0.3, 0.55) if footprint == "point" else rng.uniform(0.55, 0.8)
        ox, oy = px[i] + rng.uniform(-0.1, 0.1), py[i] + side * off
        if q % 3 == 2:
            vx, vy = rng.uniform(-0.1, 0.1), rng.uniform(-0.1, 0.1)
            obst.add_point(ox - vx * t[i], oy - vy * t[i], vel=(vx, vy))   # at pose i's time stamp it is beside pose i
        else:
            obst.add_point(ox, oy)
    if footprint == "polygon":
        i = n // 2
        obst.add_polygon([(px[i] - 0.2, py[i] + 0.7), (px[i] + 0.2, py[i] + 0.7), (px[i], py[i] + 1.0)])
        obst.add_line(px[i // 2] - 0.2, py[i // 2] - 0.7, px[i // 2] + 0.2, py[i // 2] - 0.8)
    return cfg, obst, [], batch


def _cases():
    C = {}

    def add(name, layout, n, seed=1, min_k=1, helpers=0, **kw):
        lay = "band" if layout == "band_ldlt" else layout
        opt = dict(layout=lay, band_ldlt=(layout == "band_ldlt"), multi_cu=-1, speculative_trials=-1)
        if helpers:
            opt.update(multi_cu=0, speculative_trials=helpers)
        C[name] = dict(layout=lay, n=n, seed=seed, min_k=min_k, helpers=helpers, options=opt, kw=kw)

    for layout, sizes in SIZES.items():
        for n in sizes:
            add("%s_n%d" % (layout, n), layout, n)
    for layout, n in POLYGON.items():
        add("%s_polygon_n%d" % (layout, n), layout, n, footprint="polygon")
    for layout, (n, seed) in REJECTED.items():
        add("%s_rejected_n%d" % (layout, n), layout, n, seed=seed, min_k=2, rough=True)
    for layout, (n, stride, seed) in HELPERS.items():
        add("%s_helpers_n%d" % (layout, n), layout, n, seed=seed, min_k=2, helpers=3, rough=True, stride=stride)
    return C


CASES = _cases()


def build(name):
    c = dict(CASES[name])
    cfg, obst, via, batch = scene(c["n"], c["seed"], **c.pop("kw"))
    c.update(cfg=cfg, obst=obst, via=via, batch=batch, options=_abi.Options(**c["options"]))
    return c
