"""Fleets for the per-scene equivalence-class tests (tests/test_fleet_classes.py on the CPU, tests/test_gpu_fleet_classes.py on the
device), on the Fleet of tests/fleet_cases.py. Small, and at the sizes where the fleet H-signature kernels can go wrong:

  rows    scenes of 1, 15, 16, 17 and 0 rows and one of `big_rows` rows (255 / 256 / 257: the 256-lane block of the wide 3-D kernel; 15 /
          16 / 17: the 16-obstacle tile of the small one); the widest scene is not the first one;
  poses   bands of 2, 17, 18 and 40 poses (17 / 18 poses = 16 / 17 segments: either side of the small kernel's 16-segment chunk), one
          band with two coincident consecutive poses;
  layout  one scene without bands, the bands of the scenes interleaved (a fixed shuffle);
  classes the bands of a scene share start and goal, like the candidates of one robot. A band is the lateral sine +a sin or its mirror
          -a sin; `inner` obstacles lie inside the lens between the two (so mirrored bands differ in class), the others far outside it.
          Scenes 1 and 3 hold two bands on one side and one on the other: the class filter drops one, and with
          max_number_plans_in_current_class = 2 and the best band on the double side it keeps both;
  detours scene 3 has a fourth band that starts backwards (deletePlansDetouringBackwards drops it), scene 1 a band three and a half
          times as slow as the others; scene 4 has a single band (the rule's early-out).

point_class_fleet(dynamic=True): HSignature3d (include_dynamic_obstacles; some rows move), False: HSignature (2-D), same geometry.
Stride 96; capacities from Fleet.capacities().

A seed whose signatures sit too close to a decision (tests/test_fleet_classes.py states the margins) is replaced here, scene by scene,
as tests/fleet_cases.py does with `replaced=`: REPLACED maps a scene to the attempt used instead of attempt 0."""
import numpy as np

import fleet_cases
from teb_local_planner_amd import _abi, scenes
from teb_local_planner_amd.config import TebConfig

SEED = 20240
LENGTH = 4.0
STRIDE = 96
REPLACED = {}
# hcp.h_signature_prescaler of the tests. The 2-D signature scales with prod 1 / |o_l - o_j|: obstacles metres apart leave it far below the
# threshold 0.1 for every band, so nothing would be told apart; 100 brings the class scenes' differences to 0.2 .. 2.5.
PRESCALER = {2: 100.0, 3: 1.0}

# scene -> [(pose count, amplitude of the lateral sine, kind)]; kind: "sine", "dup" (two coincident consecutive poses), "back" (starts
# backwards), "slow" (3.5 x the transition times)
BANDS = {
    0: [(2, 0.0, "sine"), (17, 1.0, "sine")],
    1: [(40, 1.0, "sine"), (18, 0.8, "sine"), (40, -1.0, "sine"), (30, -0.9, "slow")],
    2: [(18, 1.0, "dup"), (40, -1.0, "sine")],
    3: [(17, -1.0, "sine"), (40, 1.0, "sine"), (18, -0.85, "sine"), (40, 1.0, "back")],
    4: [(17, 0.7, "sine")],
    5: [(18, 1.0, "sine"), (40, -1.0, "sine")],
    6: [],
}
INNER = {0: 0, 1: 5, 3: 6, 4: 4, 5: 0, 6: 1}   # obstacles inside the lens (scene 2: a third of its rows)
DROPS_A_CLASS = (1, 3)          # scenes where the class filter drops a band (best = None, one plan per class)
KEEPS_TWO_OF_BEST = {1: 0, 3: 0}   # scene -> k: with best = its k-th band and two plans per class, two bands of the best class are kept
LOSES_A_DETOUR = {1: (0, 3), 3: (1, 3)}   # scene -> (k of the best band, k of the band the detour rule drops), k: position among the scene's bands


def rows_of(big_rows):
    return [1, 15, big_rows, 16, 17, 0, 3]


def _band(kind, n, amp, max_vel_x):
    if kind == "back":   # first 0.9 m away from the goal, then round to it: the start orientation is more than pi / 2 off the others'
        way = np.array([(0.0, 0.0), (-0.8, 0.4), (0.5, 1.5), (3.0, 1.3), (LENGTH, 0.0)])
        seg = np.hypot(*np.diff(way, axis=0).T)
        at = np.concatenate([[0.0], np.cumsum(seg)])
        u = np.linspace(0.0, at[-1], n)
        px, py = np.interp(u, at, way[:, 0]), np.interp(u, at, way[:, 1])
        th, dt = scenes._band_from_path(px, py, max_vel_x, theta_goal=0.0)
        return px, py, th, dt
    px, py, th, dt = scenes.sine_band(n - 1 if kind == "dup" else n, LENGTH, amp, 1.0, max_vel_x)
    if kind == "dup":   # pose 7 twice, no time between the two
        k = 7
        px, py, th = np.insert(px, k, px[k]), np.insert(py, k, py[k]), np.insert(th, k, th[k])
        dt = np.insert(dt, k, 0.0)
    if kind == "slow":
        dt = dt * 3.5
    return px, py, th, dt


def point_class_fleet(big_rows=256, dynamic=True, seed=SEED, replaced=None):
    replaced = REPLACED if replaced is None else replaced
    rows = rows_of(big_rows)
    ns = len(rows)
    cfg = TebConfig()
    cfg.obstacles.include_dynamic_obstacles = bool(dynamic)
    scene_of = np.repeat(np.arange(ns), [len(BANDS[s]) for s in range(ns)])
    np.random.default_rng(seed).shuffle(scene_of)
    batch = _abi.TebBatchHost(len(scene_of), STRIDE)
    tables, vias, origins = [], [], []
    for s in range(ns):
        g = fleet_cases._scene_rng(seed, s, replaced)
        x0, y0 = float(g.uniform(-20, 20)), float(g.uniform(-20, 20))
        origins.append((x0, y0))
        for b, (n, amp, kind) in zip(np.nonzero(scene_of == s)[0], BANDS[s]):
            px, py, th, dt = _band(kind, n, amp, cfg.robot.max_vel_x)
            th = th + g.normal(0.0, 2e-3, th.shape)
            batch.set_teb(int(b), px + x0, py + y0, th, dt)
        M = rows[s]
        inner = INNER.get(s, M // 3)
        n_dyn = min(M - inner, max(1, M // 6)) if M > 1 else 0
        t = _abi.ObstacleTable()
        for k in range(M):
            if k < inner:   # inside the lens |y| < a sin(pi x / L), clear of the bands of amplitude >= 0.7
                x = g.uniform(1.0, 3.0)
                p = (x, g.uniform(-0.4, 0.4) * np.sin(np.pi * x / LENGTH))
            else:           # outside every band, the backwards one included
                p = (g.uniform(-0.5, LENGTH + 0.5), g.uniform(2.0, 3.5) * (1 if g.random() < 0.5 else -1))
            v = (g.uniform(-0.005, 0.005), g.uniform(-0.005, 0.005))   # (120 s of it: <= 0.6 m; drawn in 2-D as well: same geometry)
            vel = v if (dynamic and k >= M - n_dyn) else None
            t.add_point(x0 + p[0], y0 + p[1], vel=vel)
        tables.append(t)
        vias.append([])
    return fleet_cases.Fleet(cfg, tables, vias, batch, scene_of, origins)
