"""Seeded fleets for the fleet-batch tests (tests/test_fleet_pack.py, tests/test_gpu_fleet.py): scenes that DIFFER, each with one to five
bands, the bands of a scene interleaved with the bands of the others.

  point_fleet : point scenes in the style of scenes._multi_band_scene - 20 .. 120 point obstacles per scene, some of them dynamic
                (include_dynamic_obstacles on), point footprint: every scene alone is point-like, and so is the fleet;
  mixed_fleet : the table of scenes.scene_small_mixed translated and thinned per scene, per-scene via-points, ONE scene without any
                obstacle, polygon footprint: every scene alone runs the generic distance path, and so does the fleet.

Bands come from scenes.sine_band with the heading noise of tests/random_cases.py (headings exactly along the segments sit on the sign(0)
convention of the non-holonomic Jacobian)."""
import numpy as np

from teb_local_planner_amd import _abi, scenes
from teb_local_planner_amd.config import TebConfig


class Fleet:
    """cfg, tables [n_scenes] ObstacleTable, vias [n_scenes] [(x, y)], batch (all bands), scene_of [B]"""

    def __init__(self, cfg, tables, vias, batch, scene_of, origins=None):
        self.cfg, self.tables, self.vias, self.batch = cfg, tables, vias, batch
        self.scene_of = np.asarray(scene_of, np.int32)
        self.origins = origins   # [n_scenes] (x, y): where each scene lies on the floor

    @property
    def n_scenes(self):
        return len(self.tables)

    def bands_of(self, s):
        return [int(b) for b in np.nonzero(self.scene_of == s)[0]]

    def scene_batch(self, s):
        """The bands of scene s as a batch of their own (same stride), in band order."""
        idx = self.bands_of(s)
        sub = _abi.TebBatchHost(len(idx), self.batch.stride)
        for k, b in enumerate(idx):
            for f in ("n", "x", "y", "theta", "dt", "has_vel_start", "vel_start", "has_vel_goal", "vel_goal", "prefer_rotdir", "via_points_enabled"):
                getattr(sub, f)[k] = getattr(self.batch, f)[b]
        return sub, idx

    def capacities(self):
        """(max_obstacles, max_obstacle_vertices, max_via_points) that hold the whole scene set"""
        return (max(sum(len(t) for t in self.tables), 1), max(sum(len(t.vert_x) for t in self.tables), 1), max(sum(len(v) for v in self.vias), 1))


def _interleave(rng, counts):
    """scene of every band: counts[s] bands of scene s, shuffled"""
    scene_of = np.repeat(np.arange(len(counts)), counts)
    rng.shuffle(scene_of)
    return scene_of.astype(np.int32)


def _scene_rng(seed, s, replaced):
    """Every scene has a generator of its own, so that ONE scene can be replaced (tests/sensitivity.py marks a band of it ill-conditioned)
    without moving the others: `replaced` maps a scene to the attempt that is used instead of attempt 0."""
    return np.random.default_rng([int(seed), int(s), int((replaced or {}).get(s, 0))])


def point_fleet(seed, n_scenes=6, stride=96, bands=(1, 5), poses=(20, 36), obstacles=(20, 120), length=None, empty_tail=False, spacing=None,
                amplitude=0.5, clearance=0.0, replaced=None):
    """bands / poses / obstacles: (lo, hi) inclusive ranges drawn per scene / band, or one number. spacing: pose spacing [m] of the bands
    (default: the band's length / its pose count, length 0.1 m per pose unless `length` is given). empty_tail: one more scene, without
    bands (the selection's empty case). amplitude: bound of the bands' lateral sine (with the defaults the CPU oracle ends the bands of
    the seeds the tests use at <= 79 poses: they fit the smallest capacity of the tests, 96). clearance: every obstacle starts at least that far
    from every band of its scene. replaced: {scene: attempt}, see _scene_rng."""
    rng = np.random.default_rng(seed)
    cfg = TebConfig()
    cfg.obstacles.include_dynamic_obstacles = True
    draw = lambda g, r: int(r) if np.isscalar(r) else int(g.integers(r[0], r[1] + 1))
    counts = [draw(rng, bands) for _ in range(n_scenes)]
    scene_of = _interleave(rng, counts)
    batch = _abi.TebBatchHost(len(scene_of), stride)
    tables, vias, origins = [], [], []
    for s in range(n_scenes):
        g = _scene_rng(seed, s, replaced)
        n_ref = draw(g, poses)
        L = float(length) if length is not None else (spacing if spacing is not None else 0.1) * (n_ref - 1)
        M = draw(g, obstacles)
        n_dyn = int(g.integers(1, max(2, M // 6)))
        x0, y0 = float(g.uniform(-20, 20)), float(g.uniform(-20, 20))   # every robot somewhere else on the floor
        origins.append((x0, y0))
        paths = []
        for b in np.nonzero(scene_of == s)[0]:
            n = n_ref if spacing is not None else draw(g, poses)
            px, py, th, dt = scenes.sine_band(n, L, g.uniform(-amplitude, amplitude), float(g.integers(1, 4)), cfg.robot.max_vel_x)
            th = th + g.normal(0.0, 2e-3, th.shape)
            batch.set_teb(int(b), px + x0, py + y0, th, dt)
            batch.has_vel_goal[b] = 1
            paths.append((px, py))
        t = _abi.ObstacleTable()
        pts = []
        while len(pts) < M:
            p = (g.uniform(0.5, max(L - 0.5, 1.0)), g.uniform(-3.0, 3.0))
            if clearance <= 0.0 or all(np.min(np.hypot(px - p[0], py - p[1])) >= clearance for px, py in paths):
                pts.append(p)
        for k, p in enumerate(pts):
            vel = None if k < M - n_dyn else (g.uniform(-0.5, 0.5), g.uniform(-0.5, 0.5))
            t.add_point(x0 + p[0], y0 + p[1], vel=vel)
        tables.append(t)
        vias.append([])
    if empty_tail:
        t = _abi.ObstacleTable()
        t.add_point(100.0, 100.0)
        tables.append(t); vias.append([]); origins.append((100.0, 100.0))
    return Fleet(cfg, tables, vias, batch, scene_of, origins)


def _translated_thinned(base, dx, dy, keep):
    """rows `keep` of an ObstacleTable, moved by (dx, dy)"""
    t = _abi.ObstacleTable()
    for i in keep:
        vel = (base.vx[i], base.vy[i]) if base.dynamic[i] else None
        ty = base.type[i]
        if ty == _abi.OBST_POLYGON:
            k0, k1 = base.vert_offset[i], base.vert_offset[i + 1]
            t.add_polygon([(base.vert_x[k] + dx, base.vert_y[k] + dy) for k in range(k0, k1)], vel=vel)
        else:
            t._add(ty, base.ax[i] + dx, base.ay[i] + dy, base.bx[i] + (dx if ty in (_abi.OBST_LINE, _abi.OBST_PILL) else 0.0),
                   base.by[i] + (dy if ty in (_abi.OBST_LINE, _abi.OBST_PILL) else 0.0), base.radius[i], vel=vel)
    return t


def _sample_points(t):
    """points on the outline of every row of an ObstacleTable, with the row's radius: (x, y, r)"""
    out = []
    for i in range(len(t)):
        ty = t.type[i]
        if ty == _abi.OBST_POLYGON:
            k0, k1 = t.vert_offset[i], t.vert_offset[i + 1]
            vs = [(t.vert_x[k], t.vert_y[k]) for k in range(k0, k1)]
            segs = list(zip(vs, vs[1:] + vs[:1]))
        elif ty in (_abi.OBST_LINE, _abi.OBST_PILL):
            segs = [((t.ax[i], t.ay[i]), (t.bx[i], t.by[i]))]
        else:
            segs = [((t.ax[i], t.ay[i]), (t.ax[i], t.ay[i]))]
        for (x0, y0), (x1, y1) in segs:
            out += [(x0 + (x1 - x0) * u, y0 + (y1 - y0) * u, t.radius[i]) for u in np.linspace(0.0, 1.0, 9)]
    return out


def mixed_fleet(seed, n_scenes=6, stride=96, bands=(1, 5), poses=(16, 40), clearance=0.3, replaced=None, empty=None):
    """empty: the scene without any obstacle (default: drawn from the seed). clearance: every band starts at least that far from the outline of every obstacle of its scene - the lateral sine is drawn again
    until it does. replaced: {scene: attempt}, see _scene_rng."""
    rng = np.random.default_rng(seed)
    cfg, base, base_via, _ = scenes.scene_small_mixed(seed=seed, footprint="polygon")
    counts = [int(rng.integers(bands[0], bands[1] + 1)) for _ in range(n_scenes)]
    scene_of = _interleave(rng, counts)
    batch = _abi.TebBatchHost(len(scene_of), stride)
    drawn = int(rng.integers(0, n_scenes))
    empty = drawn if empty is None else int(empty)   # the scene without any obstacle
    tables, vias = [], []
    for s in range(n_scenes):
        g = _scene_rng(seed, s, replaced)
        dx, dy = float(g.uniform(-10, 10)), float(g.uniform(-10, 10))
        keep = [] if s == empty else [i for i in range(len(base)) if g.random() < 0.7]
        tables.append(_translated_thinned(base, dx, dy, keep))
        vias.append([(vx + dx + float(g.uniform(-0.2, 0.2)), vy + dy) for (vx, vy) in base_via[:int(g.integers(0, len(base_via) + 1))]])
        pts = _sample_points(tables[-1])
        for b in np.nonzero(scene_of == s)[0]:
            n = int(g.integers(poses[0], poses[1] + 1))
            for _ in range(400):
                px, py, th, dt = scenes.sine_band(n, 6.0, g.uniform(-0.8, 0.8), float(g.integers(1, 3)), cfg.robot.max_vel_x)
                if all(np.min(np.hypot(px + dx - x, py + dy - y)) >= clearance + r for x, y, r in pts):
                    break
            else:
                raise RuntimeError("mixed_fleet: no band of scene %d keeps the clearance" % s)
            th = th + g.normal(0.0, 2e-3, th.shape)
            batch.set_teb(int(b), px + dx, py + dy, th, dt)
            batch.has_vel_goal[b] = 1
            batch.has_vel_start[b] = 1
            batch.vel_start[b] = (0.1, 0.0, 0.05)
    return Fleet(cfg, tables, vias, batch, scene_of)


# The two fleets that are compared with the CPU oracle (tests/test_gpu_fleet.py). sensitivity.band_tolerances, run on the CPU over every
# scene, marks none of their bands ill-conditioned (no None, none above WELL_CONDITIONED_TOL); the scenes it did mark at attempt 0 -
# mostly a dynamic obstacle that drifts into a band - are replaced by a later attempt of their own generator, listed here. The oracle
# ends the bands at <= 117 (points) and <= 57 (mixed) poses.
CLEARANCE = 0.6
POINTS_ORACLE_REPLACED = {0: 1, 3: 1, 12: 1, 16: 2, 21: 1, 31: 1, 38: 1, 42: 1, 43: 2, 46: 2, 48: 1, 56: 1, 61: 3}
MIXED_ORACLE_REPLACED = {0: 5, 1: 2, 2: 3, 3: 2}


def oracle_point_fleet(seed=4242, n_scenes=64, per_scene=4, poses=100, obstacles=60, stride=160):
    """The fleet of the oracle-parity test and of tools/fleet_bench.py: n_scenes point scenes x per_scene bands x poses x obstacles."""
    return point_fleet(seed, n_scenes=n_scenes, stride=stride, bands=per_scene, poses=poses, obstacles=obstacles, length=10.0, amplitude=1.5, clearance=CLEARANCE,
                       replaced=POINTS_ORACLE_REPLACED if seed == 4242 else None)


def oracle_mixed_fleet(stride=96):
    """The mixed fleet of the bit-identity and oracle-parity tests: 6 scenes, 17 bands."""
    return mixed_fleet(102, stride=stride, replaced=MIXED_ORACLE_REPLACED)
