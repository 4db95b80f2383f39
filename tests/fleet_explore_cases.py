"""Scene sets for the per-scene candidate exploration (tests/test_fleet_explore.py on the CPU, tests/test_gpu_fleet_explore.py on the
device), on the Fleet of tests/fleet_cases.py. Eight scenes, each the planner of one robot with its own start, goal, best band and
initial plan; the bands of the scenes interleaved by a fixed shuffle. Every scene lies at its own origin; in its own frame the start is
(0, 0, 0) and the goal (4, 0, 0) unless stated. A band is a lateral sine between start and goal - `up` (+), `down` (-), `updown`,
`downup` (one full period) - and the `inner` obstacles lie on the axis between the two, so the shapes differ in class.

  scene 0  PLAIN    8 obstacles in front of the start (spread to both sides of the axis), 2 behind it, no band: gains several classes;
  scene 1  FULL     2 inner obstacles, four bands of four classes (max_number_classes = 4): stays untouched and draws nothing;
  scene 2  LINE     start within xy_goal_tolerance of the goal, no band: gets the line band;
  scene 3  AT_GOAL  the same with a band: gets nothing;
  scene 4  BEST     7 obstacles in front, 1 behind; bands up, up (smaller amplitude), down; the first is the best band: with
                    max_number_plans_in_current_class = 2 both `up` bands survive the class filter, with 1 only the best one;
  scene 5  PLAN_NEW 1 obstacle in front, 2 behind; a `down` band, an initial plan along `up` (a new class) and two via-points;
  scene 6  PLAN_OLD 2 obstacles in front; an `up` band, an initial plan along `up` (its class is present) and one via-point;
  scene 7  EMPTY    the empty table as the LAST scene of the set (the padded tail of the store), no band. Roadmap graph: every path
                    falls in one class, so the scene examines paths until max_paths = MAX_PATHS = 3 * 16 + 5 cuts it, inside its fourth
                    round of 16. Keypoint graph: start and goal only, one path.

Keypoint graph: 0 / 1 / 7 / 8 obstacles in front of the start give N = 2, 4, 16, 18 vertices, N^2 = 4, 16, 256, 324: either side of
one 256-lane workgroup, and one scene that needs two workgroups while the others need one. Roadmap graph: N = samples + 2 for every
scene, so the fixture takes roadmap_graph_no_samples 13 / 14 / 15 (N^2 = 225 / 256 / 289).

explore_fleet(kind="points")  point obstacles, some of them moving slowly when dynamic (HSignature3d), else HSignature;
explore_fleet(kind="mixed")   the same places as points, circles, lines, pills and polygons in turn: every branch of
                              Obstacle::checkLineIntersection is met by the edge kernel.
Bands of <= 40 poses, <= 10 obstacles per scene, stride 48."""
import numpy as np

import fleet_cases
import fleet_class_cases
from teb_local_planner_amd import _abi, scenes
from teb_local_planner_amd.config import TebConfig, RobotFootprintModel

SEED = 6021
LENGTH = 4.0
STRIDE = 48
QUOTA = 16                  # paths per scene and round of the library (kExploreQuota)
MAX_PATHS = 3 * QUOTA + 5
DIST_TO_OBST = 0.2          # of every exploration call of the tests: the roadmap's edges pass between obstacles half a metre apart
PLAIN, FULL, LINE, AT_GOAL, BEST, PLAN_NEW, PLAN_OLD, EMPTY = range(8)
N_SCENES = 8
IN_FRONT = {PLAIN: 8, FULL: 2, LINE: 3, AT_GOAL: 2, BEST: 7, PLAN_NEW: 1, PLAN_OLD: 2, EMPTY: 0}
BEHIND = {PLAIN: 2, BEST: 1, PLAN_NEW: 2}
KEYPOINT_VERTICES = {PLAIN: 18, BEST: 16, PLAN_NEW: 4, EMPTY: 2}   # 2 + 2 x obstacles in front (the scenes that reach their graph)
# scene -> [(pose count, shape)]
BANDS = {
    PLAIN: [],
    FULL: [(17, "up"), (18, "down"), (30, "updown"), (40, "downup")],
    LINE: [],
    AT_GOAL: [(5, "short")],
    BEST: [(40, "up"), (24, "up8"), (33, "down")],
    PLAN_NEW: [(25, "down")],
    PLAN_OLD: [(31, "up")],
    EMPTY: [],
}
BEST_BAND = {BEST: 0}          # scene -> position of the best band among the bands of the scene
PLAN = {PLAN_NEW: 12, PLAN_OLD: 9}   # scene -> poses of the initial plan (along `up`)
VIAS = {PLAN_NEW: [(1.3, 0.9), (2.7, 0.9)], PLAN_OLD: [(2.0, 1.0)]}
SHAPES = {"up": (1.0, 1.0), "down": (-1.0, 1.0), "updown": (1.0, 2.0), "downup": (-1.0, 2.0), "up8": (0.8, 1.0)}


def _band(shape, n, max_vel_x):
    if shape == "short":   # start and goal 0.1 m apart
        return scenes.sine_band(n, 0.1, 0.0, 1.0, max_vel_x)
    amp, half_periods = SHAPES[shape]
    return scenes.sine_band(n, LENGTH, amp, half_periods, max_vel_x)


def _add(t, kind, k, x, y, vel):
    """obstacle k of a scene at (x, y): a point, or for the mixed fleet one of the five obstacle classes in turn"""
    which = 0 if kind == "points" else k % 5
    if which == 0:
        t.add_point(x, y, vel=vel)
    elif which == 1:
        t.add_circle(x, y, 0.08, vel=vel)
    elif which == 2:
        t.add_line(x - 0.06, y - 0.1, x + 0.06, y + 0.1, vel=vel)
    elif which == 3:
        t.add_pill(x - 0.1, y + 0.05, x + 0.1, y - 0.05, 0.05, vel=vel)
    else:
        t.add_polygon([(x - 0.1, y - 0.08), (x + 0.1, y - 0.08), (x + 0.02, y + 0.12)], vel=vel)


class ExploreFleet(fleet_cases.Fleet):
    """A Fleet with what the exploration of every scene takes: starts / goals [n_scenes][3], best [n_scenes] (band index or -1),
    plans [n_scenes] ((x, y, yaw) or None), max_paths and dist_to_obst."""

    def scene_case(self, s):
        """scene s as a case of tests/test_gpu_candidates.py: what a planner that holds only this scene is given"""
        sub, idx = self.scene_batch(s)
        best = idx.index(int(self.best[s])) if self.best[s] >= 0 else -1
        return dict(cfg=self.cfg, obst=self.tables[s], via=self.vias[s], batch=sub if idx else None, best=best, start=list(self.starts[s]),
                    goal=list(self.goals[s]), initial_plan=self.plans[s], optimized=[1] * len(idx))


def explore_fleet(kind="points", dynamic=True, keypoint=False, no_samples=15, plans_in_class=1, viapoints_all_candidates=True, seed=SEED):
    cfg = TebConfig()
    if kind == "mixed":
        cfg.robot_model = RobotFootprintModel.polygon([(-0.2, -0.15), (0.4, -0.15), (0.4, 0.15), (-0.2, 0.15)])
    cfg.obstacles.include_dynamic_obstacles = bool(dynamic)
    h = cfg.hcp
    h.simple_exploration = bool(keypoint)
    h.roadmap_graph_no_samples = int(no_samples)
    h.max_number_classes = 4
    h.max_number_plans_in_current_class = int(plans_in_class)
    h.viapoints_all_candidates = bool(viapoints_all_candidates)
    h.h_signature_prescaler = fleet_class_cases.PRESCALER[3 if dynamic else 2]
    scene_of = np.repeat(np.arange(N_SCENES), [len(BANDS[s]) for s in range(N_SCENES)])
    np.random.default_rng(seed).shuffle(scene_of)
    batch = _abi.TebBatchHost(len(scene_of), STRIDE)
    tables, vias, origins, starts, goals, plans = [], [], [], [], [], []
    best = np.full(N_SCENES, -1, np.int32)
    for s in range(N_SCENES):
        g = np.random.default_rng([int(seed), s])
        x0, y0 = 12.0 * (s % 3) - 12.0 + float(g.uniform(-1, 1)), 12.0 * (s // 3) - 12.0 + float(g.uniform(-1, 1))
        origins.append((x0, y0))
        mine = np.nonzero(scene_of == s)[0]
        for b, (n, shape) in zip(mine, BANDS[s]):
            px, py, th, dt = _band(shape, n, cfg.robot.max_vel_x)
            th = th + g.normal(0.0, 2e-3, th.shape)
            th[0] = 0.0
            batch.set_teb(int(b), px + x0, py + y0, th, dt)
            batch.has_vel_goal[b] = 1
        if s in BEST_BAND:
            best[s] = mine[BEST_BAND[s]]
        t = _abi.ObstacleTable()
        nf, nb = IN_FRONT[s], BEHIND.get(s, 0)
        xs = np.linspace(0.7, LENGTH - 0.7, nf) if nf > 1 else np.array([LENGTH / 2])
        for k in range(nf):   # on the axis between the shapes, clear of every band of amplitude >= 0.8
            y = float(g.uniform(0.05, 0.25)) * (1 if k % 2 else -1)
            if s == PLAIN:   # spread out, so that the roadmap's edges (dist_to_obst from every obstacle) find gaps between them
                y = float(g.uniform(0.9, 1.9)) * (1 if k % 2 else -1)
            vel = (float(g.uniform(-0.004, 0.004)), float(g.uniform(-0.004, 0.004))) if (dynamic and k % 3 == 2) else None
            _add(t, kind, k, x0 + float(xs[k]) + float(g.uniform(-0.05, 0.05)), y0 + y, vel)
        for k in range(nb):   # behind the start: in the signature, not in the keypoint graph
            _add(t, kind, nf + k, x0 - 1.0 - 0.7 * k, y0 + float(g.uniform(-1.0, 1.0)), None)
        tables.append(t)
        vias.append([(x0 + vx, y0 + vy) for vx, vy in VIAS.get(s, [])])
        starts.append((x0, y0, 0.0))
        goals.append((x0 + (0.1 if s in (LINE, AT_GOAL) else LENGTH), y0, 0.0))
        if s in PLAN:
            px, py, th, _ = scenes.sine_band(PLAN[s], LENGTH, 1.0, 1.0, cfg.robot.max_vel_x)
            plans.append((px + x0, py + y0, th))
        else:
            plans.append(None)
    f = ExploreFleet(cfg, tables, vias, batch, scene_of, origins)
    f.starts, f.goals, f.plans, f.best = np.array(starts), np.array(goals), plans, best
    f.max_paths = MAX_PATHS
    f.dist_to_obst = DIST_TO_OBST
    return f


def unit_samples(f, seed=77, seed_empty=85):
    """[n_scenes][2 * roadmap_graph_no_samples] numbers in [0, 1): the samples of every scene's roadmap, given instead of drawn. The row
    of the scene without obstacles comes from a seed whose roadmaps hold more than MAX_PATHS start-goal paths (75 .. 80 with 13, 14 and
    15 samples), so that max_paths is what ends that scene."""
    shape = (f.n_scenes, 2 * f.cfg.hcp.roadmap_graph_no_samples)
    u = np.random.default_rng(seed).random(shape)
    u[EMPTY] = np.random.default_rng(seed_empty).random(shape)[EMPTY]
    return u
