"""Seeded cases of tests/test_hp_linearize.py and tests/test_gpu_hp_linearize.py. NOT a test file.

Each case is ONE cost-term family at a weight != 0 with every other weight 0, on one band, with limits tightened until the family's
penalties bite. A case is a dict:
  cfg, obst, via, batch          the scene (band 0 is linearised)
  wms                            weight multipliers that have a fixture of their own (the multiplier only enters the obstacle weights;
                                 the other families are compared with the one fixture at both multipliers)
  active    [(edge type, row)]   row kinds that must be non-zero on >= 25 % of their rows
  two_sided [(edge type, row)]   row kinds that must be active on each side on >= 2 rows
  ring      bool                 inflated obstacle rows: >= 2 edges inside min_obstacle_dist and >= 2 in the inflation ring only
  layouts                        the short cases run in the host's own pick and in each pinned layout, a long case in its named one
  kink_delta                     only the documented car-like kink: the reference is the central-difference quotient at this delta
  near                           cases next to a kink: ((edge type, argument, which switch point), side, the edge's integer record)
  silent    [(edge type, row)]   row kinds that are in the graph but must be exactly 0 everywhere (see velocity_obstacle_ratio)
The conditions are asserted from the high-precision reference alone (tests/test_hp_linearize.py).
"""
import math

import numpy as np

from teb_local_planner_amd import scenes, _abi
from teb_local_planner_amd.config import TebConfig, RobotFootprintModel

import hp_linearize as hp

SHORT_LAYOUTS = ("auto", "cr", "band", "bandg")
LAYOUT_INDEX = {"band": 0, "cr": 1, "bandg": 2}   # teb_amd_debug_last_instantiation's numbering


def _config(**weights):
    cfg = TebConfig()
    for k in vars(cfg.optim):
        if k.startswith("weight_") and k != "weight_adapt_factor":
            setattr(cfg.optim, k, 0.0)
    for k, v in weights.items():
        assert hasattr(cfg.optim, k)
        setattr(cfg.optim, k, v)
    return cfg


def _band(n, seed, length=None, amp=0.5, half_periods=2.0, xy=0.02, th=0.12, dt=(0.6, 1.6), backward=(), stride=None, vmax=0.4):
    """sine band of scenes.sine_band with seeded perturbations of the inner poses and of every time difference; the poses of
    `backward` (a range) head against their motion"""
    rng = np.random.default_rng(seed)
    length = 0.25 * (n - 1) if length is None else length
    px, py, pth, pdt = scenes.sine_band(n, length, amp, half_periods, vmax)
    px[1:-1] += rng.uniform(-xy, xy, n - 2); py[1:-1] += rng.uniform(-xy, xy, n - 2)
    pth[1:-1] += rng.uniform(-th, th, n - 2)
    for i in backward:
        pth[i] = scenes.normalize_theta(pth[i] + math.pi)
    pdt = pdt * rng.uniform(dt[0], dt[1], n - 1)
    batch = _abi.TebBatchHost(1, stride or max(96, n))
    batch.set_teb(0, px, py, pth, pdt)
    batch.has_vel_start[0] = 0; batch.has_vel_goal[0] = 0
    return batch


def _case(cfg, batch, obst=None, via=(), wms=(1.0,), active=(), two_sided=(), ring=False, layouts=SHORT_LAYOUTS, kink_delta=None,
          silent=()):
    return dict(near=None, cfg=cfg, obst=obst if obst is not None else _abi.ObstacleTable(), via=list(via), batch=batch, wms=tuple(wms),
                active=list(active), two_sided=list(two_sided), ring=ring, layouts=tuple(layouts), kink_delta=kink_delta,
                silent=list(silent))


# ---- velocity / acceleration ----------------------------------------------------------------------------------------------------------
def velocity(exact=False, n=24, seed=11, **kw):
    cfg = _config(weight_max_vel_x=2.0, weight_max_vel_theta=1.0)
    cfg.trajectory.exact_arc_length = exact
    cfg.robot.max_vel_x, cfg.robot.max_vel_x_backwards, cfg.robot.max_vel_theta = 0.35, 0.15, 0.12
    back = range(n // 3, n // 3 + max(4, n // 5))
    return _case(cfg, _band(n, seed, backward=back), active=[(hp.E_VEL, 0), (hp.E_VEL, 1)], two_sided=[(hp.E_VEL, 0), (hp.E_VEL, 1)], **kw)


def velocity_holonomic(n=24, seed=12):
    cfg = _config(weight_max_vel_x=2.0, weight_max_vel_y=2.0, weight_max_vel_theta=1.0)
    cfg.robot.max_vel_x, cfg.robot.max_vel_x_backwards, cfg.robot.max_vel_y = 0.3, 0.15, 0.03
    cfg.robot.max_vel_trans, cfg.robot.max_vel_theta = 0.42, 0.12
    back = range(n // 3, n // 3 + 5)
    return _case(cfg, _band(n, seed, th=0.3, backward=back), active=[(hp.E_VELH, 0), (hp.E_VELH, 1), (hp.E_VELH, 2)],
                 two_sided=[(hp.E_VELH, 0), (hp.E_VELH, 1), (hp.E_VELH, 2)])


def acceleration(holonomic=False, exact=False, n=24, seed=13, **kw):
    cfg = _config(weight_acc_lim_x=1.0, weight_acc_lim_theta=1.0)
    cfg.trajectory.exact_arc_length = exact
    cfg.robot.acc_lim_x, cfg.robot.acc_lim_theta = 0.08, 0.08
    batch = _band(n, seed, th=0.3 if holonomic else 0.12, backward=range(n // 2, n // 2 + 4))
    batch.has_vel_start[0] = 1; batch.has_vel_goal[0] = 1
    batch.vel_start[0] = (0.1, 0.05, 0.05); batch.vel_goal[0] = (0.05, -0.25, -0.1)
    if holonomic:
        cfg.optim.weight_acc_lim_y = 1.0
        cfg.robot.max_vel_y, cfg.robot.acc_lim_y = 0.2, 0.08
        mid, se, rows = hp.E_ACCH, (hp.E_ACCHS, hp.E_ACCHG), 3
    else:
        mid, se, rows = hp.E_ACC, (hp.E_ACCS, hp.E_ACCG), 2
    active = [(t, k) for t in (mid,) + se for k in range(rows)]
    return _case(cfg, batch, active=active, two_sided=[(mid, k) for k in range(rows)], **kw)


# ---- kinematics -------------------------------------------------------------------------------------------------------------------------
def diff_drive(row, n=24, seed=14, **kw):
    """row 0: the non-holonomic row alone, row 1: the forward-drive row alone (active on backward-moving segments)"""
    cfg = _config(**({"weight_kinematics_nh": 1000.0} if row == 0 else {"weight_kinematics_forward_drive": 1.0}))
    back = range(n // 4, n // 4 + max(7, n // 3))
    return _case(cfg, _band(n, seed, backward=back), active=[(hp.E_KDD, row)], two_sided=[(hp.E_KDD, 0)] if row == 0 else [], **kw)


def carlike(exact=False, n=24, seed=15, nh=True, **kw):
    cfg = _config(weight_kinematics_turning_radius=1.0, **({"weight_kinematics_nh": 1000.0} if nh else {}))
    cfg.trajectory.exact_arc_length = exact
    cfg.robot.min_turning_radius = 3.0
    return _case(cfg, _band(n, seed), active=[(hp.E_KCL, 1)] + ([(hp.E_KCL, 0)] if nh else []), two_sided=[(hp.E_KCL, 0)] if nh else [], **kw)


def carlike_straight_stretch(n=30, seed=16):
    """The documented kink: the first third of the band is an exact straight line along the x axis with heading 0 (the non-holonomic
    residual and the angle difference are exactly 0 there), the rest is curved. The reference of this case is the central-difference
    quotient at delta = 1e-9, which kin_nh<JAC, CDK> (csrc/teb_edges.hpp) is designed to reproduce: next to nothing on the straight
    stretch, where sign(x) g would be the full row."""
    c = carlike(n=n, seed=seed)
    b = c["batch"]
    k = n // 3
    b.x[0, :k + 1] = 0.25 * np.arange(k + 1); b.y[0, :k + 1] = 0.0; b.theta[0, :k + 1] = 0.0
    b.x[0, k + 1:n] += b.x[0, k] + 0.25 - b.x[0, k + 1]
    c["kink_delta"] = "1e-9"
    c["active"] = [(hp.E_KCL, 0), (hp.E_KCL, 1)]
    return c


# ---- time-optimal, shortest path, prefer-rotdir, via-points -------------------------------------------------------------------------------
def time_optimal(n=24, seed=17, **kw):
    return _case(_config(weight_optimaltime=1.0), _band(n, seed), active=[(hp.E_TIME, 0)], **kw)


def shortest_path(n=24, seed=18):
    return _case(_config(weight_shortest_path=0.7), _band(n, seed), active=[(hp.E_SP, 0)])


def prefer_rotdir(direction, n=24, seed=19):
    batch = _band(n, seed)
    batch.theta[0, 1:4] = batch.theta[0, 0] + np.array([0.1, -0.05, 0.1])   # turns left, right, left
    batch.prefer_rotdir[0] = direction
    return _case(_config(weight_prefer_rotdir=50.0), batch, active=[(hp.E_ROT, 0)])


def via_points(ordered, n=24, seed=20):
    cfg = _config(weight_viapoint=1.0)
    cfg.trajectory.via_points_ordered = ordered
    batch = _band(n, seed)
    batch.via_points_enabled[0] = 1
    L = 0.25 * (n - 1)
    return _case(cfg, batch, via=[(0.3 * L, 0.35), (0.55 * L, -0.3), (0.8 * L, 0.15)], active=[(hp.E_VIA, 0)])


# ---- obstacles ------------------------------------------------------------------------------------------------------------------------------
FOOTPRINTS = {
    "point": RobotFootprintModel.point, "circular": lambda: RobotFootprintModel.circular(0.2),
    "two_circles": lambda: RobotFootprintModel.two_circles(0.3, 0.2, 0.15, 0.25),
    "line": lambda: RobotFootprintModel.line((-0.2, 0.0), (0.4, 0.0)),
    "polygon": lambda: RobotFootprintModel.polygon([(-0.2, -0.15), (0.4, -0.15), (0.4, 0.15), (-0.2, 0.15)])}


def _table(seed, L, dynamic=False, near=0.55, far=1.0, per_type=2):
    """`per_type` obstacles of each of the five types beside the sine band of length L, at seeded lateral offsets"""
    rng = np.random.default_rng(seed)
    t = _abi.ObstacleTable()
    xs = np.linspace(0.12 * L, 0.88 * L, 5 * per_type)
    order = rng.permutation(5 * per_type)
    for j, k in enumerate(order):
        ty = int(k) % 5
        x = float(xs[j]) + rng.uniform(-0.1, 0.1)
        y0 = 0.5 * math.sin(math.pi * 2.0 * x / L)
        y = y0 + (1 if j % 2 else -1) * rng.uniform(near, far)
        vel = (rng.uniform(-0.08, 0.08), rng.uniform(-0.08, 0.08)) if dynamic else None
        a = rng.uniform(0, math.pi)
        ex, ey = 0.3 * math.cos(a), 0.3 * math.sin(a)
        if ty == 0: t.add_point(x, y, vel=vel)
        elif ty == 1: t.add_circle(x, y, 0.15, vel=vel)
        elif ty == 2: t.add_line(x - ex, y - ey, x + ex, y + ey, vel=vel)
        elif ty == 3: t.add_pill(x - ex, y - ey, x + ex, y + ey, 0.1, vel=vel)
        else:
            m = 3 + int(rng.integers(0, 3))
            t.add_polygon([(x + 0.25 * math.cos(a + 2 * math.pi * q / m), y + 0.25 * math.sin(a + 2 * math.pi * q / m)) for q in range(m)], vel=vel)
    return t


def static_obstacles(footprint, inflated, exponent, n=24, seed=21, legacy=False, overlap=False):
    cfg = _config(weight_obstacle=50.0, weight_inflation=0.1 if inflated else 0.0)
    cfg.robot_model = FOOTPRINTS[footprint]()
    cfg.obstacles.min_obstacle_dist = 0.45
    cfg.obstacles.inflation_dist = 0.8 if inflated else 0.3
    cfg.optim.obstacle_cost_exponent = exponent
    cfg.obstacles.include_dynamic_obstacles = False
    if legacy:
        cfg.obstacles.legacy_obstacle_association = True
        cfg.obstacles.obstacle_poses_affected = 6
    batch = _band(n, seed)
    obst = _table(seed + 100, 0.25 * (n - 1), near=0.3 if footprint == "point" else 0.55, far=0.75 if footprint == "point" else 1.0)
    if overlap:   # a polygon obstacle across the band's middle pose: the polygon footprint overlaps it (distance exactly 0)
        i = n // 2
        x, y = float(batch.x[0, i]), float(batch.y[0, i])
        obst.add_polygon([(x + 0.05, y - 0.3), (x + 0.33, y + 0.02), (x + 0.07, y + 0.31), (x - 0.28, y + 0.06)])
    ty = hp.E_INFL if inflated else hp.E_OBST
    return _case(cfg, batch, obst=obst, wms=(1.0, 2.0), active=[(ty, k) for k in range(2 if inflated else 1)], ring=inflated)


def dynamic_obstacles(footprint, n=24, seed=22):
    cfg = _config(weight_obstacle=50.0, weight_dynamic_obstacle=50.0, weight_dynamic_obstacle_inflation=0.1)
    cfg.robot_model = FOOTPRINTS[footprint]()
    cfg.obstacles.min_obstacle_dist, cfg.obstacles.dynamic_obstacle_inflation_dist = 0.7, 1.2
    cfg.obstacles.inflation_dist = 0.3
    cfg.obstacles.include_dynamic_obstacles = True
    # a short band (3 m): most poses are within reach of the five moving obstacles. The multiplier does not enter these weights.
    return _case(cfg, _band(n, seed, length=3.0), obst=_table(seed + 100, 3.0, dynamic=True, near=0.3, far=0.9, per_type=1),
                 active=[(hp.E_DYN, 0), (hp.E_DYN, 1)])


def velocity_obstacle_ratio(footprint="circular", n=24, seed=23):
    """The ratio edges hang on the obstacle association, which exists only with weight_obstacle != 0: min_obstacle_dist is set so small
    (and the association factors so large) that every obstacle edge is there and silent - residual and Jacobian exactly 0."""
    cfg = _config(weight_obstacle=50.0, weight_velocity_obstacle_ratio=3.0)
    cfg.robot_model = FOOTPRINTS[footprint]()
    cfg.obstacles.min_obstacle_dist, cfg.obstacles.inflation_dist = 0.01, 0.0
    cfg.obstacles.obstacle_association_force_inclusion_factor, cfg.obstacles.obstacle_association_cutoff_factor = 90.0, 500.0
    cfg.obstacles.obstacle_proximity_lower_bound, cfg.obstacles.obstacle_proximity_upper_bound = 0.3, 0.8
    cfg.obstacles.obstacle_proximity_ratio_max_vel = 0.8
    cfg.obstacles.include_dynamic_obstacles = False
    cfg.robot.max_vel_theta = 0.25
    back = range(n // 3, n // 3 + 5)
    return _case(cfg, _band(n, seed, backward=back), obst=_table(seed + 100, 0.25 * (n - 1), near=0.45, far=1.0), active=[(hp.E_VOR, 0), (hp.E_VOR, 1)],
                 two_sided=[(hp.E_VOR, 0), (hp.E_VOR, 1)], silent=[(hp.E_OBST, 0)])


# ---- long bands: one per layout ---------------------------------------------------------------------------------------------------------------
LONG = {"band": 300, "cr": 238, "bandg": 600}   # LDS band (leftover pass: several lanes per pose beyond 256), blocks, HBM band


def point_obstacles_long(n, seed=24):
    cfg = _config(weight_obstacle=50.0, weight_inflation=0.1)
    cfg.obstacles.min_obstacle_dist, cfg.obstacles.inflation_dist = 0.55, 0.8
    cfg.obstacles.include_dynamic_obstacles = False
    batch = _band(n, seed, stride=n)
    L = 0.25 * (n - 1)
    rng = np.random.default_rng(seed + 100)
    obst = _abi.ObstacleTable()
    for j in range(n // 4):
        x = rng.uniform(0.5, L - 0.5)
        obst.add_point(x, 0.5 * math.sin(math.pi * 2.0 * x / L) + rng.choice([-1, 1]) * rng.uniform(0.15, 0.6))
    return _case(cfg, batch, obst=obst, wms=(1.0, 2.0), active=[(hp.E_INFL, 0), (hp.E_INFL, 1)], ring=True)


def _long(builder, layout, **kw):
    n = LONG[layout]
    c = builder(n=n, **kw)
    b = c["batch"]
    if b.stride != n:   # the handle is sized for exactly this band
        nb = _abi.TebBatchHost(1, n)
        nb.set_teb(0, *b.get_teb(0))
        for k in ("has_vel_start", "vel_start", "has_vel_goal", "vel_goal", "prefer_rotdir", "via_points_enabled"):
            setattr(nb, k, getattr(b, k).copy())
        c["batch"] = nb
    c["layouts"] = (layout,)
    return c


# ---- next to a kink: one penalty (or |.|) argument 1e-6 below / above its switch point ------------------------------------------------------
NEAR_OFFSET = 1e-6
NEAR = [   # (base case, edge type, name of the argument in hp_linearize, which switch point)
    ("velocity", hp.E_VEL, "velocity", "lo"), ("velocity", hp.E_VEL, "velocity", "hi"),
    ("velocity", hp.E_VEL, "angular velocity", "lo"), ("velocity", hp.E_VEL, "angular velocity", "hi"),
    ("velocity_holonomic", hp.E_VELH, "vx", "lo"), ("velocity_holonomic", hp.E_VELH, "vx", "hi"),
    ("velocity_holonomic", hp.E_VELH, "vy", "lo"), ("velocity_holonomic", hp.E_VELH, "vy", "hi"),
    ("velocity_holonomic", hp.E_VELH, "angular velocity", "lo"), ("velocity_holonomic", hp.E_VELH, "angular velocity", "hi"),
    ("acceleration", hp.E_ACC, "acceleration", "lo"), ("acceleration", hp.E_ACC, "acceleration", "hi"),
    ("acceleration", hp.E_ACC, "angular acceleration", "lo"), ("acceleration", hp.E_ACC, "angular acceleration", "hi"),
    ("acceleration", hp.E_ACCS, "acceleration", "hi"), ("acceleration", hp.E_ACCG, "acceleration", "lo"),
    ("acceleration_holonomic", hp.E_ACCH, "acceleration x", "lo"), ("acceleration_holonomic", hp.E_ACCH, "acceleration x", "hi"),
    ("acceleration_holonomic", hp.E_ACCH, "acceleration y", "lo"), ("acceleration_holonomic", hp.E_ACCH, "acceleration y", "hi"),
    ("acceleration_holonomic", hp.E_ACCH, "angular acceleration", "lo"), ("acceleration_holonomic", hp.E_ACCH, "angular acceleration", "hi"),
    ("diff_drive_nh", hp.E_KDD, "non-holonomic constraint", "lo"), ("diff_drive_forward", hp.E_KDD, "forward projection", "lo"),
    ("carlike", hp.E_KCL, "non-holonomic constraint", "lo"), ("carlike", hp.E_KCL, "turning radius", "lo"),
    ("carlike_exact_arc", hp.E_KCL, "turning radius", "lo"),
    ("prefer_rotdir_left", hp.E_ROT, "preferred rotation", "lo"),
    ("obstacles_circular_inflated_exp1", hp.E_INFL, "obstacle distance (min_obstacle_dist)", "lo"),
    ("obstacles_circular_inflated_exp1", hp.E_INFL, "obstacle distance (inflation_dist)", "lo"),
    ("obstacles_polygon_plain_exp1p7", hp.E_OBST, "obstacle distance (min_obstacle_dist)", "lo"),
    ("dynamic_obstacles_two_circles", hp.E_DYN, "obstacle distance (min_obstacle_dist)", "lo"),
    ("dynamic_obstacles_two_circles", hp.E_DYN, "obstacle distance (dynamic_obstacle_inflation_dist)", "lo"),
    ("velocity_obstacle_ratio", hp.E_VOR, "velocity (ratio bound)", "lo"), ("velocity_obstacle_ratio", hp.E_VOR, "velocity (ratio bound)", "hi"),
    ("velocity_obstacle_ratio", hp.E_VOR, "angular velocity (ratio bound)", "lo"), ("velocity_obstacle_ratio", hp.E_VOR, "angular velocity (ratio bound)", "hi"),
]


def near_gap(c, edges_of, spec, key=None):
    """(gap, key): argument minus switch point of the edge named by `key` (its integer record), or of the edge of the wanted kind whose
    argument is nearest to its switch point"""
    edge, what, which = spec
    ir = edges_of(c)
    if key is None:
        pick = [e for e in range(len(ir)) if int(ir[e][0]) == edge]
    else:
        pick = [e for e in range(len(ir)) if tuple(int(v) for v in ir[e][:11]) == key]
    assert pick, "the edge left the graph"
    A = hp.switch_arguments(c["cfg"], c["obst"], c["via"], c["batch"], 0, 1.0, ir, only=set(pick))
    best = None
    for e in pick:
        for w, v, lo, hi in A[e]:
            thr = lo if which == "lo" else hi
            if w == what and thr is not None and (best is None or abs(v - thr) < abs(best[0])):
                best = (v - thr, tuple(int(q) for q in ir[e][:11]))
    assert best is not None
    return best


def near(base, edge, what, which, side, edges_of):
    """The case `base` with ONE state variable moved until the argument `what` of one edge of kind `edge` lies NEAR_OFFSET on `side`
    (+1 above, -1 below) of its switch point: the edge whose argument is nearest to start with, the variable it is most sensitive to,
    a secant iteration on the high-precision argument. edges_of(case) returns the edge records (oracle.edges)."""
    c = build(base)
    spec = (edge, what, which)
    gap0, key = near_gap(c, edges_of, spec)
    b, n = c["batch"], int(c["batch"].n[0])
    poses = [int(key[2 + k]) for k in range(key[1])]
    slots = [(arr, i) for i in poses if 0 < i < n - 1 for arr in (b.x, b.y, b.theta)] + [(b.dt, int(key[6 + k])) for k in range(key[5]) if key[6 + k] < n - 1]
    g = lambda: near_gap(c, edges_of, spec, key)[0] - side * NEAR_OFFSET
    sens = []
    for arr, i in slots:
        v0 = arr[0, i]
        arr[0, i] = v0 + 1e-5
        sens.append(abs(g() - (gap0 - side * NEAR_OFFSET)))
        arr[0, i] = v0
    arr, i = slots[int(np.argmax(sens))]
    x0, f0 = float(arr[0, i]), gap0 - side * NEAR_OFFSET
    x1 = x0 + 1e-5
    for _ in range(20):
        arr[0, i] = x1
        f1 = g()
        if abs(f1) < 1e-11 or f1 == f0:
            break
        x0, f0, x1 = x1, f1, x1 - f1 * (x1 - x0) / (f1 - f0)
    c["near"] = (spec, side, key)
    c["base"] = base
    c["active"], c["two_sided"], c["ring"] = [], [], False
    return c


def _cases():
    C = {}
    C["velocity"] = (velocity, {})
    C["velocity_exact_arc"] = (velocity, dict(exact=True))
    C["velocity_holonomic"] = (velocity_holonomic, {})
    C["acceleration"] = (acceleration, {})
    C["acceleration_exact_arc"] = (acceleration, dict(exact=True))
    C["acceleration_holonomic"] = (acceleration, dict(holonomic=True))
    C["diff_drive_nh"] = (diff_drive, dict(row=0))
    C["diff_drive_forward"] = (diff_drive, dict(row=1))
    C["carlike"] = (carlike, {})
    C["carlike_exact_arc"] = (carlike, dict(exact=True))
    C["carlike_turning_radius_only"] = (carlike, dict(nh=False))
    C["carlike_straight_stretch"] = (carlike_straight_stretch, {})
    C["time_optimal"] = (time_optimal, {})
    C["shortest_path"] = (shortest_path, {})
    C["prefer_rotdir_left"] = (prefer_rotdir, dict(direction=_abi.ROT_LEFT))
    C["prefer_rotdir_right"] = (prefer_rotdir, dict(direction=_abi.ROT_RIGHT))
    C["via_points_ordered"] = (via_points, dict(ordered=True))
    C["via_points_unordered"] = (via_points, dict(ordered=False))
    for fp in FOOTPRINTS:
        for inflated in (True, False):
            for ex in (1.0, 1.7):
                C["obstacles_%s_%s_exp%s" % (fp, "inflated" if inflated else "plain", "1" if ex == 1.0 else "1p7")] = \
                    (static_obstacles, dict(footprint=fp, inflated=inflated, exponent=ex))
    C["obstacles_polygon_overlap"] = (static_obstacles, dict(footprint="polygon", inflated=True, exponent=1.0, overlap=True))
    C["dynamic_obstacles_line"] = (dynamic_obstacles, dict(footprint="line"))
    C["dynamic_obstacles_two_circles"] = (dynamic_obstacles, dict(footprint="two_circles"))
    C["dynamic_obstacles_polygon"] = (dynamic_obstacles, dict(footprint="polygon"))
    C["velocity_obstacle_ratio"] = (velocity_obstacle_ratio, {})
    C["legacy_association"] = (static_obstacles, dict(footprint="circular", inflated=True, exponent=1.0, legacy=True))
    for layout in LONG:
        C["long_%s_velocity" % layout] = (_long, dict(builder=velocity, layout=layout))
        C["long_%s_acceleration" % layout] = (_long, dict(builder=acceleration, layout=layout))
        C["long_%s_kinematics" % layout] = (_long, dict(builder=diff_drive, layout=layout, row=0))
        C["long_%s_time_optimal" % layout] = (_long, dict(builder=time_optimal, layout=layout))
        C["long_%s_point_obstacles" % layout] = (_long, dict(builder=point_obstacles_long, layout=layout))
    for base, edge, what, which in NEAR:
        for side in (-1, 1):
            name = "near_%s_%s_%s_%s_%s" % (base, hp.EDGE_NAMES[edge], what.replace(" ", "_").replace("(", "").replace(")", ""), which, "below" if side < 0 else "above")
            C[name] = (near, dict(base=base, edge=edge, what=what, which=which, side=side))
    return C


CASES = _cases()

# Seeds off a builder's default. A seeded state can put two nearly equal coordinates into one difference (an obstacle straight ahead of
# a footprint vertex: J_x = (x_v - x_o) / d with x_v - x_o ~ 1e-3 of the coordinates) or a distance within 1e-3 of its threshold under
# obstacle_cost_exponent 1.7 (pow of a difference of two nearly equal numbers): fp64 INPUT rounding then shows at 1e-13 .. 1e-12 in the
# metric whatever the closed form. Such states are replaced by the next seed that is free of them; nothing else is selected for.
SEEDS = {"long_band_acceleration": 31, "long_bandg_acceleration": 31, "obstacles_line_inflated_exp1": 36, "obstacles_line_inflated_exp1p7": 36, "obstacles_line_plain_exp1": 36,
         "obstacles_line_plain_exp1p7": 38, "obstacles_polygon_inflated_exp1": 31, "obstacles_polygon_inflated_exp1p7": 31,
         "obstacles_polygon_plain_exp1": 31, "obstacles_polygon_plain_exp1p7": 31}


def is_near(name):
    return CASES[name][0] is near


def build(name, seed=None, edges_of=None, state=None):
    """edges_of(case) -> the edge records of band 0 (oracle.edges at multiplier 1): the cases next to a kink need it to find their
    state; or state = (x, y, theta, dt) as recorded in the fixture, which replaces the search (the GPU test: no mpmath, no oracle)"""
    builder, kw = CASES[name]
    kw = dict(kw)
    if builder is near:
        if state is not None:
            c = build(kw["base"])
            c["batch"].set_teb(0, *state)
            c["active"], c["two_sided"], c["ring"] = [], [], False
            return c
        kw["edges_of"] = edges_of
    seed = SEEDS.get(name) if seed is None else seed
    if seed is not None:
        kw["seed"] = seed
    return builder(**kw)
