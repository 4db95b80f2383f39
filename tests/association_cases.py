"""Cases of tests/test_hp_association.py and tests/test_gpu_hp_association.py: scenes ON the thresholds of the graph build. NOT a test file.

Everything is built so that fp64 is exact where a decision is close: the band lies on a dyadic grid (x_i = 0.25 i, y = 0, theta = 0: cos
and sin are exact; dt = 0.5), the thresholds are dyadic (min_obstacle_dist 0.5, force factor 1.5 -> 0.75, cutoff factor 5 -> 2.5; radii
and footprints 0.125 / 0.25 / 0.375), and a deciding obstacle sits on the axis through ITS pose ((x_p, +-D): sqrt(fl(D^2)) = D in fp64) or
at a scaled 3-4-5 offset ((+-0.75, 1.0): 1.25). tests/hp_association.py checks that every comparison of every pose is either exact or
separated by 1e-9 (neighbouring poses see the same obstacles at sqrt(D^2 + (0.25 j)^2)); a case that is not raises there.

A case is a dict: cfg, obst, via, batch; family; pointlike (which distance path must run); legacy; hcheck (H, b, chi^2 against the
80-digit linearisation); exempt [(edge type, pose, obstacle, argument name)] (hp_linearize.linearize(exempt=...)); numeric (the lists also
in the numeric Jacobian mode, and with hcheck H and b against the 80-digit central differences at delta = 1e-9 under numeric_bound); helpers (one optimize(1, 1) with and without helper workgroups must leave the same bits); claims (what the
CPU test asserts from the reference's records that the case contains - see each builder).
"""
import math

import numpy as np

from teb_local_planner_amd import _abi
from teb_local_planner_amd.config import RobotFootprintModel

import hp_linearize as hp
from hp_linearize_cases import _config

STEP = 0.25
MOD, FORCE, CUTOFF = 0.5, 0.75, 2.5
# the next five restate the kernel's geometry; tests/test_hp_association.py (test_the_kernel_has_the_geometry_the_cases_assume) reads them
# back from csrc/teb_kernel.hpp, teb_device.hpp and teb_opt_launch.hpp, tests/test_gpu_hp_association.py from the loaded build
K_SLICE_FORCED = 6   # csrc/teb_kernel.hpp: kSliceForced
K_THREADS = 256
POINTLIKE_KINDS = {0, 2, 4, 5, 8, 9, 10, 11}   # scene kinds of teb_amd_debug_last_instantiation on the point-like distance path

FOOTPRINTS = {
    "point": (RobotFootprintModel.point, 0.0), "circular": (lambda: RobotFootprintModel.circular(0.125), 0.125),
    "two_circles": (lambda: RobotFootprintModel.two_circles(0.25, 0.125, 0.25, 0.125), None),
    "line": (lambda: RobotFootprintModel.line((-0.25, 0.0), (0.25, 0.0)), None),
    "polygon": (lambda: RobotFootprintModel.polygon([(-0.25, -0.125), (0.25, -0.125), (0.25, 0.125), (-0.25, 0.125)]), None)}

# s of a rung: ("ulp", k) = k ulp of the centre distance, ("rel", +-e) = a factor 1 +- 2^-e
RUNGS = [("0", ("ulp", 0)), ("+1ulp", ("ulp", 1)), ("-1ulp", ("ulp", -1)), ("+4ulp", ("ulp", 4)), ("-4ulp", ("ulp", -4)),
         ("+2^-41", ("rel", 41)), ("-2^-41", ("rel", -41)), ("+2^-36", ("rel", 36)), ("-2^-36", ("rel", -36))]
RUNGS_GUARD9 = RUNGS + [("+2^-29", ("rel", 29)), ("-2^-29", ("rel", -29))]   # across the 1e-9 guard of the bounding circles
RUNGS_DYNAMIC = [r for r in RUNGS if r[0] not in ("0", "+1ulp", "-1ulp")]


NUMERIC_DELTA = 1e-9


def numeric_bound(batch):
    """Bound on the H / b error (metric of hp_linearize.errors) of an fp64 implementation of g2o's central differences, delta = 1e-9,
    against the same quotient at 80 digits. fl(v +- delta) is off by up to ulp(v) / 2, so the step actually taken differs from 2 delta
    by up to eps |v|: relative eps |v| / (2 delta) in a Jacobian entry; the rounding of the two residuals (a few eps of a distance of the
    order of 1) adds a few eps / (2 delta); H = w J^T J doubles the relative error and sums a few rows. 64 eps max(1, |v|max) / delta:
    1.1e-4 for a band within 8 m of the origin, 1.1e-3 at 75 m. An edge wrongly culled next to its threshold, where the quotient is
    half the slope, is an error of the order of 1 in this metric (measured with the closed forms in its place: 3.0)."""
    n = int(batch.n[0])
    vmax = max(1.0, float(np.abs(batch.x[0, :n]).max()), float(np.abs(batch.y[0, :n]).max()))
    return 64 * np.finfo(np.float64).eps * vmax / NUMERIC_DELTA


def rung(D, s):
    kind, k = s
    if kind == "ulp":
        for _ in range(abs(k)):
            D = float(np.nextafter(D, math.inf if k > 0 else -math.inf))
        return D
    out = D * (1.0 + math.copysign(2.0 ** -abs(k), k))
    assert out != D
    return out


def lanes_per_pose(poses_left):
    G = 1
    while G < 8 and 2 * G * poses_left <= K_THREADS:
        G *= 2
    return G


def leftover_lanes(n):
    """lanes per pose of the pass that holds the poses >= 256 (1: no such pass)"""
    return lanes_per_pose(n - K_THREADS) if n > K_THREADS else 1


def slice_width(M, G):
    return (((M + G - 1) // G) + 3) & ~3


def _band(n, bend=None):
    x, y = STEP * np.arange(n), np.zeros(n)
    if bend is not None:   # out along y = 0 up to pose `bend`, three poses up, back along y = 1: everything on the grid
        for i in range(bend + 1, n):
            up = min(i - bend, 4)
            x[i], y[i] = STEP * (bend - max(0, i - bend - 4)), STEP * up
    batch = _abi.TebBatchHost(1, max(96, n))
    batch.set_teb(0, x, y, np.zeros(n), np.full(n - 1, 0.5))
    batch.has_vel_start[0] = 0; batch.has_vel_goal[0] = 0
    return batch


def _cfg(footprint="point", force_factor=1.5, cutoff_factor=5.0, inflation=4.0, **weights):
    """inflation_dist 4 > cutoff: every associated obstacle has a live inflation row, so a wrong list shows in H at the size of the weight"""
    w = dict(weight_obstacle=50.0, weight_inflation=1.0)
    w.update(weights)
    cfg = _config(**w)
    cfg.robot_model = FOOTPRINTS[footprint][0]()
    o = cfg.obstacles
    o.min_obstacle_dist, o.inflation_dist = MOD, inflation
    o.obstacle_association_force_inclusion_factor, o.obstacle_association_cutoff_factor = force_factor, cutoff_factor
    o.include_dynamic_obstacles = False
    cfg.trajectory.teb_autosize = False   # (the helper-workgroup runs go through optimize(): the graph must be built on THIS band)
    return cfg


class _Table:
    """a static list of M entries: the named positions hold what the case puts there, every other one an obstacle far beyond the cutoff"""

    def __init__(self, M, kind="point", n=24):
        self.M, self.kind, self.n, self.at = M, kind, n, {}

    def put(self, pos, *spec):
        assert 0 <= pos < self.M and pos not in self.at, pos
        self.at[pos] = spec

    def free(self, lo=0):
        return next(p for p in range(lo, self.M) if p not in self.at)

    def build(self):
        t = _abi.ObstacleTable()
        for p in range(self.M):
            spec = self.at.get(p)
            if spec is None:
                spec = ("point", STEP * (p % self.n), 64.0 + p) if self.kind == "point" else ("circle", STEP * (p % self.n), 64.0 + p, 0.25)
            getattr(t, "add_" + spec[0])(*spec[1:])
        return t


def _case(family, cfg, obst, batch, via=(), pointlike=True, legacy=False, hcheck=False, exempt=(), numeric=False, helpers=False, claims=None,
          layouts=None):
    n = int(batch.n[0])
    return dict(family=family, cfg=cfg, obst=obst, via=list(via), batch=batch, pointlike=pointlike, legacy=legacy, hcheck=hcheck,
                exempt=list(exempt), numeric=numeric, helpers=helpers, claims=claims or {},
                layouts=tuple(layouts) if layouts else layouts_for(n))


LAYOUT_LIMITS = (("cr", 238), ("band", 337))   # the largest band each LDS layout holds (csrc/teb_amd.hip: teb_amd_create_ex; pinned by
#                                                  tests/test_gpu_parity.py: test_maximum_pose_capacities); the band in HBM holds every pose count


def layouts_for(n):
    """the host's own pick and every pinned layout the pose count admits"""
    return ("auto",) + tuple(name for name, most in LAYOUT_LIMITS if n <= most) + ("bandg",)


def auto_layout(n):
    """what the host picks for a handle of n poses whose obstacle cache fits beside the normal matrix (every case here: at most 130
    point-like obstacles, 5 doubles each): blocks in LDS while they fit, else the band in LDS, else the band in HBM"""
    return next((name for name, most in LAYOUT_LIMITS if n <= most), "bandg")


def _obstacle(kind, x, y):
    return ("point", x, y) if kind == "point" else ("circle", x, y, 0.25)


# ---- threshold ladder ---------------------------------------------------------------------------------------------------------------
def ladder(threshold, kind, footprint):
    """threshold 'force' / 'cutoff': the standard factors; 'cull': force factor 5 > cutoff factor 1.5, so the culling radius
    max(cutoff, force) + radii is the FORCE threshold (inside: forced, outside: beyond the cutoff as well). Pose 4 + 2 j carries rung
    j // 2 on side j % 2 (left / right); 'force': pose 4 + 12 j - two rungs of one side are 24 poses apart, beyond each other's cutoff, or
    the pose midway between them would see them at sqrt(D^2 + dx^2) and sqrt(D'^2 + dx^2), an inexact near-tie. A rung of 'force' has a companion on its side, farther (1.0) and EARLIER in the table: the list
    is [rung, companion] when the rung is forced and [rung] when it is a candidate. claims: rungs [(name, pose, obstacle, side, forced,
    associated)]."""
    radii = (0.25 if kind == "circle" else 0.0) + FOOTPRINTS[footprint][1]
    cfg = _cfg(footprint, 5.0, 1.5) if threshold == "cull" else _cfg(footprint)
    thr = {"force": FORCE, "cutoff": CUTOFF, "cull": 2.5}[threshold]
    step = 12 if threshold == "force" else 2
    n = 4 + step * (2 * len(RUNGS) - 1) + 10
    tab = _Table(2 * 2 * len(RUNGS) + 3, kind, n)
    rungs = []
    for j in range(2 * len(RUNGS)):
        name, s = RUNGS[j // 2]
        side = 1.0 if j % 2 == 0 else -1.0
        p = 4 + step * j
        D = rung(thr + radii, s)
        if threshold == "force":
            tab.put(2 * j, *_obstacle(kind, STEP * p, side * (1.0 + radii)))
        tab.put(2 * j + 1, *_obstacle(kind, STEP * p, side * D))
        inside = D < thr + radii
        rungs.append((name, p, 2 * j + 1, "left" if side > 0 else "right", bool(inside and threshold != "cutoff"),
                      bool(inside or (D == thr + radii and threshold != "cull") or threshold == "force")))
    return _case("ladder", cfg, tab.build(), _band(n), hcheck=True, numeric=(kind == "point" and footprint == "point"), claims=dict(rungs=rungs))


# ---- list positions and lengths -----------------------------------------------------------------------------------------------------
def positions(M, n=24, kind="point", where=None):
    """the deciding obstacle of pose p_j sits at list position where[j], exactly AT the cutoff (it must be associated), alone on its side;
    everything else lies far beyond the cutoff. n > 256: the deciding poses are >= 256 (several lanes per pose). claims: deciding
    [(pose, position)]"""
    radii = 0.25 if kind == "circle" else 0.0
    if where is None:
        where = sorted({0, 7, 8, 31, 32, 63, 64, M - 1} & set(range(M)))
    first, step = (2, 2) if n <= K_THREADS else (K_THREADS, 1 if n - K_THREADS < 2 * len(where) + 2 else 2)
    tab = _Table(M, kind, n)
    deciding = []
    for j, pos in enumerate(where):
        p = first + step * (j // 2 if n == 260 else j)   # n = 260 has three poses beyond 256: two deciding obstacles (left, right) per pose
        assert p < n - 1
        tab.put(pos, *_obstacle(kind, STEP * p, (1.0 if j % 2 == 0 else -1.0) * (CUTOFF + radii)))
        deciding.append((p, pos))
    return _case("positions", _cfg("point"), tab.build(), _band(n), claims=dict(deciding=deciding))


# ---- ties ---------------------------------------------------------------------------------------------------------------------------
def ties(n=120, M=40, pairs=None, triple=True):
    """pair (a, b) of list positions at bit-equal distance 1.25 on one side of its pose, at the mirrored 3-4-5 offsets (x_p -+ 0.75, 1.0):
    equidistant from pose p alone. Sides alternate and the poses are 13 apart (n = 260, three poses beyond 256: two pairs, poses 256 and
    257), so two pairs of one side are beyond each other's cutoff and each pair is the nearest of its side at its pose. With `triple`
    the first pose gets a third obstacle at the same distance, (x_p, 1.25). The lower list position must be kept.
    claims: ties [(pose, kept, rejected...)]"""
    if pairs is None:
        pairs = [(4 * q - 1, 4 * q) for q in range(1, 9)] + [(0, M - 1)]
    tab = _Table(M, "point", n)
    out = []
    for j, (a, b) in enumerate(pairs):
        side = 1.0 if j % 2 == 0 else -1.0
        p = (K_THREADS if n > K_THREADS else 4) + (1 if n == 260 else 13) * j
        assert p < n - 1 and (n != 260 or j < 2)
        tab.put(a, "point", STEP * p - 0.75, side); tab.put(b, "point", STEP * p + 0.75, side)
        rec = [p, a, b]
        if triple and j == 0:
            c = tab.free(b + 1)
            tab.put(c, "point", STEP * p, side * 1.25)
            rec.append(c)
        out.append(tuple(rec))
    return _case("ties", _cfg("point"), tab.build(), _band(n), helpers=True, claims=dict(ties=out))


def straight_ahead():
    """an obstacle on the band's own axis: the cross product is exactly 0 at every pose -> RIGHT. A left candidate farther away and later in
    the table tells the sides apart: [left, ahead] - were the obstacle ahead counted left it would win that side and the list be [ahead]."""
    n = 24
    tab = _Table(9, "point", n)
    tab.put(3, "point", STEP * 12 + 1.0, 0.0)
    tab.put(6, "point", STEP * 12, 1.5)
    return _case("ties", _cfg("point"), tab.build(), _band(n), helpers=True, claims=dict(ahead=(12, 3, 6)))


def line_centroid_side():
    """a line obstacle whose centroid lies left of pose 8 and whose nearest point (its end a) lies right of it: the side is the centroid's.
    A point on the left, nearer (1.0 < 1.0308) and later in the table, wins the left side: [point]; were the line counted right: [point, line]."""
    n = 24
    x = STEP * 8
    t = _abi.ObstacleTable()
    t.add_line(x + 1.0, -0.25, x + 3.0, 3.75)
    t.add_point(x, 1.0)
    return _case("ties", _cfg("point"), t, _band(n), pointlike=False, helpers=True, claims=dict(centroid_side=(8, 0, 1)))


# ---- forced clusters ------------------------------------------------------------------------------------------------------------------
FORCED_Y = [0.5, 0.375, 0.625, 0.25, 0.6875, 0.3125, 0.4375]   # < 0.75 on either side of the pose: 14 distinct places


def forced_clusters(n, counts, spread, M, bases):
    """per cluster j: a left candidate (1.0) at list position bases[j], `count` obstacles within the force radius of the cluster's pose
    at the positions after it (consecutive, or every third - every second for 13 - when `spread`), a right candidate (1.0) after the
    first of them when spread (between) else after the last; the first cluster also has a farther left candidate (1.5) at the end of
    the table. Clusters are 11 poses apart: an odd number, so that no pose lies midway between two. claims: clusters [(pose, [positions])]"""
    tab = _Table(M, "point", n)
    out = []
    for j, (count, base) in enumerate(zip(counts, bases)):
        p = (K_THREADS + (1 if n == 260 else 4) if n > K_THREADS else 10) + 11 * j
        assert p < n - 1
        x = STEP * p
        stride = (2 if count > 8 else 3) if spread else 1
        where = [base + 1 + stride * q for q in range(count)]
        tab.put(base, "point", x, 1.0)
        for q, w in enumerate(where):
            tab.put(w, "point", x, FORCED_Y[q // 2] * (1.0 if q % 2 == 0 else -1.0))
        tab.put(where[0] + 1 if spread else where[-1] + 1, "point", x, -1.0)
        if j == 0:
            tab.put(M - 1, "point", x, 1.5)
        out.append((p, where))
    return _case("forced", _cfg("point"), tab.build(), _band(n), helpers=True, claims=dict(clusters=out))


# ---- generic shapes -------------------------------------------------------------------------------------------------------------------
def generic_mixed(footprint):
    """line, pill and polygon obstacles beside the band, dyadic coordinates, nothing close to a threshold (the reference checks 1e-9)"""
    n = 24
    t = _abi.ObstacleTable()
    t.add_line(1.125, 1.0, 1.625, 1.375)
    t.add_pill(2.25, -1.125, 2.875, -0.875, 0.125)
    t.add_polygon([(3.5, 0.875), (4.0, 1.0), (3.875, 1.5), (3.375, 1.375)])
    t.add_line(4.5, -2.0, 4.625, -1.0)
    t.add_pill(0.5, 1.75, 0.75, 2.25, 0.25)
    t.add_polygon([(5.0625, -0.8125), (5.375, -1.5), (4.75, -1.625)])
    t.add_point(2.0, 0.625)
    t.add_circle(3.0, -0.5, 0.125)
    return _case("generic", _cfg(footprint), t, _band(n), pointlike=False, helpers=True)


def tight_bound(order):
    """T: a RADIAL segment (x_p, D) .. (x_p, D + 1), D = 1.0625: its bounding circle touches the pose's side of it, so the lower bound of
    the distance IS the distance (point footprint). E: a point at the 8-15-17 offset (0.5, 0.9375), the same distance 1.0625 from pose 8
    alone, on the same side. order 'after': E first, then T - T ties the running minimum and must not replace E; 'first': T first - it
    must be evaluated and kept. Pose 16 has a long TANGENTIAL segment (bound useless: negative) at 1.0 that must win against a point at
    1.25 earlier in the table. claims: kept (pose, kept, rejected), tangential (pose, kept, rejected)"""
    n = 24
    t = _abi.ObstacleTable()
    x = STEP * 8
    if order == "after":
        E = t.add_point(x + 0.5, 0.9375); T = t.add_line(x, 1.0625, x, 2.0625)
        kept = (8, E, T)
    else:
        T = t.add_line(x, 1.0625, x, 2.0625); E = t.add_point(x + 0.5, 0.9375)
        kept = (8, T, E)
    x = STEP * 16
    t.add_point(x, -1.25)
    t.add_line(x - 4.0, -1.0, x + 4.0, -1.0)
    return _case("generic", _cfg("point"), t, _band(n), pointlike=False, helpers=True, claims=dict(kept=kept, tangential=(16, 3, 2)))


def tight_ladder(threshold):
    """the ladder on the radial segment (x_p, D) .. (x_p, D + 1) with rungs out to +-2^-29, across the 1e-9 guard of the bounding circles"""
    thr = {"force": FORCE, "cutoff": CUTOFF}[threshold]
    step = 10 if threshold == "force" else 2   # (see ladder)
    n = 4 + step * (2 * len(RUNGS_GUARD9) - 1) + 10
    t = _abi.ObstacleTable()
    rungs = []
    for j in range(2 * len(RUNGS_GUARD9)):
        name, s = RUNGS_GUARD9[j // 2]
        side = 1.0 if j % 2 == 0 else -1.0
        p = 4 + step * j
        D = rung(thr, s)
        if threshold == "force":
            t.add_point(STEP * p, side * 1.0)
        k = t.add_line(STEP * p, side * D, STEP * p, side * (D + 1.0))
        rungs.append((name, p, k, "left" if side > 0 else "right", bool(D < thr and threshold == "force"), bool(D <= thr or threshold == "force")))
    return _case("generic", _cfg("point"), t, _band(n), pointlike=False, claims=dict(rungs=rungs))


# ---- dynamic far-field culling --------------------------------------------------------------------------------------------------------
DYN_NAME = "obstacle distance (dynamic_obstacle_inflation_dist)"
MOD_NAME = "obstacle distance (min_obstacle_dist)"


def dynamic_culling(n_dyn, footprint="point", kind="point", which="inflation", moving=False, n=32):
    """one dynamic obstacle per tested pose at thr (1 + s), thr = max(min_obstacle_dist + penalty_epsilon, dynamic_obstacle_inflation_dist)
    + radii, s from the ladder without 0 and +-1 ulp; the rest of the dynamic list (length n_dyn) far away. which: 'inflation'
    (dynamic_obstacle_inflation_dist 1.0 is the larger) or 'epsilon' (min_obstacle_dist + penalty_epsilon = 0.5 + 0.25 is). moving: the
    obstacle starts at y0 - t_p v with v = 0.25 and is at its place at the time stamp t_p = 0.5 p of ITS pose (all dyadic); at rest
    otherwise (the table accepts a dynamic obstacle with velocity zero). The deciding obstacles are spread over the list so that they fall
    on both sides of position 64 and of the multiples of 4 the slices of several lanes per pose are cut at. claims: rungs"""
    radii = (0.25 if kind == "circle" else 0.0) + FOOTPRINTS[footprint][1]
    cfg = _cfg(footprint, weight_dynamic_obstacle=50.0, weight_dynamic_obstacle_inflation=1.0, weight_inflation=0.0)
    o = cfg.obstacles
    o.include_dynamic_obstacles = True
    o.inflation_dist = 0.25
    if which == "inflation":
        o.dynamic_obstacle_inflation_dist, thr, name = 1.0, 1.0, DYN_NAME
    else:
        cfg.optim.penalty_epsilon, o.dynamic_obstacle_inflation_dist, thr, name = 0.25, 0.5, 0.75, MOD_NAME
    nr = 2 * len(RUNGS_DYNAMIC)
    assert n_dyn >= nr and n >= 4 + 2 * nr
    where = sorted({(j * (n_dyn - 1)) // (nr - 1) for j in range(nr)})
    assert len(where) == nr
    t = _abi.ObstacleTable()
    t.add_point(1.0, 80.0)   # the static list is not empty
    rungs, exempt, slot = [], [], {w: j for j, w in enumerate(where)}
    for q in range(n_dyn):
        if q not in slot:
            spec, v = _obstacle(kind, STEP * (q % n), 72.0 + q), (0.0, 0.0)
        else:
            j = slot[q]
            rname, s = RUNGS_DYNAMIC[j // 2]
            side = 1.0 if j % 2 == 0 else -1.0
            p = (K_THREADS if n > K_THREADS else 2) + 2 * j
            D = rung(thr + radii, s)
            y, v = side * D, (0.0, 0.0)
            if moving:   # y0 + t_p v = y exactly: t_p = 0.5 p, v = +-0.25, y0 = y - t_p v (exact: a dyadic shift of a number < 4)
                v = (0.0, 0.25 * side)
                y = y - 0.5 * p * v[1]
                assert y + 0.5 * p * v[1] == side * D
            spec = _obstacle(kind, STEP * p, y)
            rungs.append((rname, p, q + 1, "left" if side > 0 else "right", False, bool(D < thr + radii)))
            exempt.append((hp.E_DYN, p, q + 1, name))
        getattr(t, "add_" + spec[0])(*spec[1:], vel=v)
    return _case("dynamic", cfg, t, _band(n), hcheck=True, exempt=exempt, numeric=True, claims=dict(rungs=rungs, dynamic=True))


# ---- via-points and the legacy association ----------------------------------------------------------------------------------------------
def _via_cfg(ordered):
    cfg = _config(weight_viapoint=1.0)
    cfg.trajectory.via_points_ordered = ordered
    return cfg


def via_points(ordered, which):
    """'midway': via-points midway between poses 5 / 6 and 63 / 64 (exact ties: the earlier pose; lanes 63 and 64 are in different waves),
    one nearest to pose 0 (unordered: no edge, ordered: pose 1) and one nearest to pose n - 1 (pose n - 2);
    'bent': n = 300, the band bent on the grid so that pose 10 and pose 266 = 10 + 256 are equidistant from (2.5, 0.5) and pose 40 and 236
    from (10, 0.5): ties across the 256-lane stride and across waves;
    'start_at_n' / 'start_beyond_n' (ordered): a via-point attached to pose n - 2 / n - 1 leaves start_pose_idx = n / n + 1, the via-points
    after it finds no pose and goes to pose 1."""
    cfg = _via_cfg(ordered)
    n = 300 if which == "bent" else 100
    batch = _band(n, bend=136 if which == "bent" else None)
    batch.via_points_enabled[0] = 1
    if which == "midway":
        via = [(-0.5, 0.25), (STEP * 5 + 0.125, 0.5), (STEP * 63 + 0.125, -0.5), (STEP * (n - 1) + 0.5, 0.25)]
        want = [1 if ordered else -1, 5, 63, n - 2]
    elif which == "bent":
        via = [(2.5, 0.5), (10.0, 0.5), (STEP * 136 + 0.5, 0.5)]
        want = [10, 40, 138]
    else:
        last = n - 2 if which == "start_at_n" else n - 1
        via = [(STEP * 20, 0.5), (STEP * last, 0.25), (STEP * 50, 0.5), (STEP * 7 + 0.125, 0.5)]
        want = [20, n - 2, 1, 7]   # the third starts at -1 + 2 = 1 ... and leaves start_pose_idx = 1 again: the fourth finds its tie 7 / 8
    # (an empty obstacle table: there is no obstacle cache to keep in LDS, the host launches the generic scene kind)
    return _case("via", cfg, _abi.ObstacleTable(), batch, via=via, pointlike=False, hcheck=True, claims=dict(via=want))


def legacy(which):
    """'tie': a point, a circle, a pill, a line and a polygon each equidistant from two poses (the earlier one) with
    obstacle_poses_affected = 6; 'all': obstacle_poses_affected >= n, every obstacle goes to pose n / 2"""
    n = 24
    cfg = _cfg("point")
    cfg.obstacles.legacy_obstacle_association = True
    cfg.obstacles.obstacle_poses_affected = 6 if which == "tie" else n
    t = _abi.ObstacleTable()
    t.add_point(STEP * 5 + 0.125, 0.5)
    t.add_circle(STEP * 9 + 0.125, -0.75, 0.25)
    t.add_pill(STEP * 12 + 0.125, 0.5, STEP * 12 + 0.125, 1.5, 0.125)
    t.add_line(STEP * 15, -0.5, STEP * 16, -0.5)   # its two ends are the feet of poses 15 and 16: 0.5 each, exactly
    t.add_polygon([(STEP * 18, 0.5), (STEP * 19, 0.5), (STEP * 18 + 0.125, 1.0)])
    t.add_point(-1.0, 0.5)         # nearest to pose 0: no edge
    t.add_point(STEP * 1, 0.75)    # nearest to pose 1: no edge either (index <= 1)
    t.add_point(STEP * (n - 1) + 0.5, 0.5)   # nearest to pose n - 1: no edge (index > n - 2)
    return _case("legacy", cfg, t, _band(n), pointlike=False, legacy=True, claims=dict(closest=[5, 9, 12, 15, 18, 0, 1, n - 1] if which == "tie" else None))


def _cases():
    C = {}
    for thr in ("force", "cutoff", "cull"):
        for kind in ("point", "circle"):
            for fp in ("point", "circular"):
                C["ladder_%s_%s_%s" % (thr, kind, fp)] = (ladder, dict(threshold=thr, kind=kind, footprint=fp))
    for M in (1, 7, 8, 9, 31, 32, 33, 63, 64, 65, 130):
        C["positions_M%d" % M] = (positions, dict(M=M))
    for M in (33, 65, 130):
        C["positions_M%d_circles" % M] = (positions, dict(M=M, kind="circle"))
    # several lanes per pose: the positions either side of the slice boundaries ((M + G - 1) / G + 3) & ~3 = 20 / 36 / 68 at M = 130
    C["positions_n260_a"] = (positions, dict(M=130, n=260, where=[19, 20, 63, 64, 0, 129]))
    C["positions_n260_b"] = (positions, dict(M=130, n=260, where=[31, 32, 39, 40, 99, 100]))
    C["positions_n300"] = (positions, dict(M=130, n=300, where=[0, 7, 8, 31, 32, 35, 36, 63, 64, 71, 72, 107, 108, 129]))
    C["positions_n380"] = (positions, dict(M=130, n=380, where=[0, 7, 8, 31, 32, 63, 64, 67, 68, 129]))
    C["ties_n120"] = (ties, {})
    for tag, pairs in (("a", [(7, 8), (15, 16)]), ("b", [(23, 24), (31, 32)]), ("c", [(3, 4), (0, 39)])):   # slices of 8 at M = 40
        C["ties_n260_" + tag] = (ties, dict(n=260, pairs=pairs))
    C["ties_n300_a"] = (ties, dict(n=300, pairs=[(11, 12), (23, 24), (35, 36), (0, 39)]))   # slices of 12
    C["ties_n300_b"] = (ties, dict(n=300, pairs=[(3, 4), (31, 32), (12, 13), (27, 28)]))
    C["ties_n380"] = (ties, dict(n=380, pairs=[(19, 20), (0, 39), (3, 4), (31, 32), (15, 16), (23, 24)]))   # slices of 20
    C["ties_straight_ahead"] = (straight_ahead, {})
    C["ties_line_centroid_side"] = (line_centroid_side, {})
    # slices of ((M + G - 1) / G + 3) & ~3 list positions: M = 64: 16 (4 lanes) / 32 (2 lanes), M = 128: 32 / 64; every cluster starts a slice
    for n in (100, 300, 380):
        C["forced_consecutive_n%d" % n] = (forced_clusters, dict(n=n, counts=(5, 6, 7, 13), spread=False, M=64, bases=(0, 16, 32, 48)))
        C["forced_spread_n%d" % n] = (forced_clusters, dict(n=n, counts=(5, 6, 7, 13), spread=True, M=128, bases=(0, 32, 64, 96)))
    for count in (5, 6, 7, 13):   # n = 260: 8 lanes per pose, slices of 8 at M = 40 and M = 64; the cluster starts at position 8
        C["forced_consecutive_n260_%d" % count] = (forced_clusters, dict(n=260, counts=(count,), spread=False, M=40, bases=(7,)))
        C["forced_spread_n260_%d" % count] = (forced_clusters, dict(n=260, counts=(count,), spread=True, M=64, bases=(7,)))
    for fp in ("line", "polygon", "two_circles"):
        C["generic_mixed_%s" % fp] = (generic_mixed, dict(footprint=fp))
    C["generic_tight_bound_after"] = (tight_bound, dict(order="after"))
    C["generic_tight_bound_first"] = (tight_bound, dict(order="first"))
    C["generic_tight_ladder_force"] = (tight_ladder, dict(threshold="force"))
    C["generic_tight_ladder_cutoff"] = (tight_ladder, dict(threshold="cutoff"))
    for n_dyn in (12, 63, 64, 65, 70):
        C["dynamic_inflation_%d" % n_dyn] = (dynamic_culling, dict(n_dyn=n_dyn))
    C["dynamic_inflation_circles_circular_65"] = (dynamic_culling, dict(n_dyn=65, footprint="circular", kind="circle"))
    C["dynamic_epsilon_33"] = (dynamic_culling, dict(n_dyn=33, which="epsilon"))
    C["dynamic_moving_66"] = (dynamic_culling, dict(n_dyn=66, moving=True))
    C["dynamic_n300_24"] = (dynamic_culling, dict(n_dyn=24, n=300))   # 4 lanes per pose beyond 256: slices of 8 of the dynamic list
    for which in ("midway", "bent"):
        for ordered in (False, True):
            C["via_%s_%s" % (which, "ordered" if ordered else "unordered")] = (via_points, dict(ordered=ordered, which=which))
    C["via_start_at_n"] = (via_points, dict(ordered=True, which="start_at_n"))
    C["via_start_beyond_n"] = (via_points, dict(ordered=True, which="start_beyond_n"))
    C["legacy_tie"] = (legacy, dict(which="tie"))
    C["legacy_all_poses"] = (legacy, dict(which="all"))
    return C


CASES = _cases()
FAMILIES = ("ladder", "positions", "ties", "forced", "generic", "dynamic", "via", "legacy")


def build(name):
    builder, kw = CASES[name]
    return builder(**kw)
