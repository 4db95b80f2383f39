"""High-precision reference of one linearisation: H = sum w J^T J, b = -sum w J^T e, chi^2 per category. NOT a test file.

The residual of every edge class is restated here in plain Python over mpmath.mpf at 80 digits; no Jacobian formula exists in this
module. Every derivative is the central-difference quotient of the residual at delta = 1e-30 (truncation ~ delta^2 = 1e-60, rounding
~ 1e-80 / 1e-30 = 1e-50), so what comes out is the true derivative to ~ 1e-50 wherever the residual is smooth. The one documented
exception (cases with kink_delta set) uses delta = 1e-9, the quotient the reference planner's numeric differentiation forms.

The list of edges (which poses with which obstacle / via-point) is integer work and is passed in as `irec` (the records of
oracle.edges()); every residual, weight, time stamp and derivative is recomputed here. The decisions behind that list - thresholds,
ties, arg-mins - have an exact reference of their own, tests/hp_association.py, which holds the oracle and the device to it on scenes
built ON the thresholds (tests/test_hp_association.py, tests/test_gpu_hp_association.py).

Branch margins. A closed form and this reference agree only while both evaluate the same branch of every piecewise definition, so the
reference records how far each of the following is from its switch point, in the quantity's own unit: penalty arguments from their
thresholds, |.| arguments from 0, segment parameters u from 0 and 1, the runner-up gap of every closest-feature arg-min (candidates
that name the same pair of closest points are one feature, not rivals), the two-circle front / rear choice, the holonomic min()
choices and vt^2 - v^2 from 0, angle differences from 0 (exact arc length, car-like) and from +-pi, ||dS|| from 0. A margin below
MARGIN = 1e-7 raises BranchMarginError: 1e-7 is 1e8 x fp64 rounding at these magnitudes, so an fp64 implementation takes the same
branch. No row is ever dropped. linearize(exempt=...) leaves NAMED (edge, penalty argument) pairs out of that check for the cases
that sit on a threshold by construction: accepted only when the argument is exact in fp64 and at least 4 ulp from its switch point
(_check_exempt) - delta = 1e-30 then stays on one side, and so does any fp64 implementation. The default is unchanged.
"""
import hashlib

import numpy as np

try:
    import mpmath
    from mpmath import mpf
except ImportError:   # the fp64 part at the end (band views, metric, hashes) is all the GPU test uses, and it works without mpmath
    mpmath, mpf = None, (lambda v: v)

DPS = 80
MARGIN = 1e-7
BAND = 10  # |a - b| <= BAND for every non-zero H[a, b]: an edge spans at most three consecutive poses
EDGE_NAMES = ["obstacle", "inflated_obstacle", "dynamic_obstacle", "via_point", "velocity", "velocity_holonomic", "acceleration",
              "acceleration_start", "acceleration_goal", "acceleration_holonomic", "acceleration_holonomic_start",
              "acceleration_holonomic_goal", "time_optimal", "shortest_path", "kinematics_diff_drive", "kinematics_carlike",
              "prefer_rotdir", "velocity_obstacle_ratio"]
(E_OBST, E_INFL, E_DYN, E_VIA, E_VEL, E_VELH, E_ACC, E_ACCS, E_ACCG, E_ACCH, E_ACCHS, E_ACCHG, E_TIME, E_SP, E_KDD, E_KCL, E_ROT,
 E_VOR) = range(18)
CAT_OBST, CAT_VIA, CAT_TIME, CAT_OTHER = range(4)
FP_POINT, FP_CIRCULAR, FP_TWO_CIRCLES, FP_LINE, FP_POLYGON = range(5)
OB_POINT, OB_CIRCULAR, OB_LINE, OB_PILL, OB_POLYGON = range(5)
INF = mpf(float("inf"))


class BranchMarginError(ValueError):
    pass


class _Ctx:
    """What one evaluation of a residual records besides its value."""

    def __init__(self, allow_exact_zero):
        self.margin, self.what, self.on = INF, "", True
        self.allow_exact_zero = allow_exact_zero   # the documented kink: |x| and angle_diff may be EXACTLY 0 (a straight stretch)
        self.args = None   # a list: every kinked function then logs (name, argument, lower switch point, upper switch point)
        self.exempt = ()   # names of penalty arguments of the CURRENT edge whose distance from their switch points is not noted (linearize: exempt)

    def arg(self, what, var, lo, hi):
        if self.args is not None:
            self.args.append((what, var, lo, hi))

    def threshold(self, what, suffix, m):
        if what not in self.exempt:
            self.note(what + suffix, m)

    def note(self, what, m):
        if self.on and m < self.margin:
            self.margin, self.what = m, what


# ---- scalar pieces -------------------------------------------------------------------------------------------------------------
def _norm_theta(cx, t):
    pi = mpmath.pi
    if not (-pi <= t < pi):
        t = t - mpmath.floor(t / (2 * pi)) * 2 * pi
        if t >= pi:
            t -= 2 * pi
        if t < -pi:
            t += 2 * pi
    cx.note("angle difference from +-pi", pi - abs(t))
    return t


def _interval(cx, what, var, a, eps):
    """var kept inside (-a, a): returns (penalty, side)."""
    lo, hi = -a + eps, a - eps
    cx.arg(what, var, lo, hi)
    cx.threshold(what, " from its lower threshold", abs(var - lo)); cx.threshold(what, " from its upper threshold", abs(var - hi))
    if var < lo:
        return -var - (a - eps), -1
    if var <= hi:
        return mpf(0), 0
    return var - (a - eps), 1


def _interval2(cx, what, var, a, b, eps):
    lo, hi = a + eps, b - eps
    cx.arg(what, var, lo, hi)
    cx.threshold(what, " from its lower threshold", abs(var - lo)); cx.threshold(what, " from its upper threshold", abs(var - hi))
    if var < lo:
        return -var + (a + eps), -1
    if var <= hi:
        return mpf(0), 0
    return var - (b - eps), 1


def _below(cx, what, var, a, eps):
    cx.arg(what, var, a + eps, None)
    cx.threshold(what, " from its threshold", abs(var - (a + eps)))
    if var >= a + eps:
        return mpf(0), 0
    return -var + (a + eps), -1


def _abs(cx, what, v):
    cx.arg(what, v, mpf(0), None)
    if not (cx.allow_exact_zero and v == 0):
        cx.note("|.| argument (" + what + ") from 0", abs(v))
    return abs(v)


def _sigmoid(cx, x, scale):
    cx.note("fast_sigmoid argument from 0", abs(x) / scale)
    return x / (1 + abs(x))


def _signed_velocity(cx, P, x0, y0, t0, x1, y1, t1, dt):
    dx, dy = x1 - x0, y1 - y0
    dist = mpmath.sqrt(dx * dx + dy * dy)
    cx.note("||dS|| from 0", dist)
    ad = _norm_theta(cx, t1 - t0)
    if P.exact_arc:
        cx.note("angle difference from 0 (exact arc length)", abs(ad))
        if ad != 0:
            dist = abs(ad * (dist / (2 * mpmath.sin(ad / 2))))
    vel = dist / dt * _sigmoid(cx, 100 * (dx * mpmath.cos(t0) + dy * mpmath.sin(t0)), 100)
    return vel, ad / dt


# ---- closest features ------------------------------------------------------------------------------------------------------------
# a candidate: (value, margin inside its own evaluation, key naming the pair of closest points, flat = exactly 0 by intersection)
def _key(p, c):
    a, b = (p[0], p[1]), (c[0], c[1])
    return (a, b) if a <= b else (b, a)


def _pt_pt(p, q):
    return (mpmath.sqrt((p[0] - q[0]) ** 2 + (p[1] - q[1]) ** 2), INF, _key(p, q), False)


def _pt_seg(p, a, b):
    dx, dy = b[0] - a[0], b[1] - a[1]
    sq = dx * dx + dy * dy
    if sq == 0:
        return _pt_pt(p, a)
    u = ((p[0] - a[0]) * dx + (p[1] - a[1]) * dy) / sq
    if u <= 0:
        c, m = a, -u
    elif u >= 1:
        c, m = b, u - 1
    else:
        c, m = (a[0] + u * dx, a[1] + u * dy), min(u, 1 - u)
    return (mpmath.sqrt((p[0] - c[0]) ** 2 + (p[1] - c[1]) ** 2), m, _key(p, c), False)


def _argmin(cands):
    """first strictly smaller candidate wins (the reference's `if (new_dist < dist)` and std::min); the margin of the result is the
    winner's own margin and its gap to the best candidate that names ANOTHER feature"""
    win = cands[0]
    for c in cands[1:]:
        if c[0] < win[0]:
            win = c
    m = win[1]
    for c in cands:
        if c[2] != win[2] and not (win[3] and c[3]):
            m = min(m, c[0] - win[0])
    return (win[0], m, win[2], win[3])


def _seg_seg(a1, a2, b1, b2):
    l1 = (a2[0] - a1[0], a2[1] - a1[1]); l2 = (b2[0] - b1[0], b2[1] - b1[1])
    den = l1[0] * l2[1] - l2[0] * l1[1]
    if den != 0:
        ax = (a1[0] - b1[0], a1[1] - b1[1])
        s = (l1[0] * ax[1] - l1[1] * ax[0]) / den
        t = (l2[0] * ax[1] - l2[1] * ax[0]) / den
        if 0 <= s <= 1 and 0 <= t <= 1:   # the segments cross: distance exactly 0 until one parameter leaves [0, 1]
            return (mpf(0), min(s, 1 - s, t, 1 - t), ("cross", a1, a2, b1, b2), True)
    r = _argmin([_pt_seg(a1, b1, b2), _pt_seg(a2, b1, b2), _pt_seg(b1, a1, a2), _pt_seg(b2, a1, a2)])
    return (r[0], min(r[1], r[0]), r[2], False)   # r[0]: how far the segments are from touching


def _edges_of(V):
    e = [(V[i], V[i + 1]) for i in range(len(V) - 1)]
    if len(V) > 2:
        e.append((V[-1], V[0]))
    return e


def _pt_poly(p, V):
    if len(V) == 1:
        return _pt_pt(p, V[0])
    return _argmin([_pt_seg(p, a, b) for a, b in _edges_of(V)])


def _seg_poly(s, e, V):
    if len(V) == 1:
        return _pt_seg(V[0], s, e)
    return _argmin([_seg_seg(s, e, a, b) for a, b in _edges_of(V)])


def _poly_poly(V1, V2):
    if len(V1) == 1:
        return _pt_poly(V1[0], V2)
    return _argmin([_seg_poly(a, b, V2) for a, b in _edges_of(V1)])


def _minus(c, r):
    return (c[0] - r, c[1], c[2], c[3])


class _Obstacle:
    def __init__(self, table, i):
        f = lambda a: mpf(float(a[i]))
        self.type = int(table.type[i])
        self.a, self.b, self.r = (f(table.ax), f(table.ay)), (f(table.bx), f(table.by)), f(table.radius)
        self.v = (f(table.vx), f(table.vy))
        lo, hi = table.vert_offset[i], table.vert_offset[i + 1]
        self.verts = [(mpf(float(table.vert_x[k])), mpf(float(table.vert_y[k]))) for k in range(lo, hi)]

    def at(self, t):
        """(a, b, vertices) predicted with constant velocity; t = None: the obstacle as it stands"""
        if t is None:
            return self.a, self.b, self.verts
        ox, oy = t * self.v[0], t * self.v[1]
        sh = lambda p: (p[0] + ox, p[1] + oy)
        return sh(self.a), sh(self.b), [sh(p) for p in self.verts]


def _dist_point(p, ob, t):
    a, b, V = ob.at(t)
    if ob.type == OB_POINT: return _pt_pt(p, a)
    if ob.type == OB_CIRCULAR: return _minus(_pt_pt(p, a), ob.r)
    if ob.type == OB_LINE: return _pt_seg(p, a, b)
    if ob.type == OB_PILL: return _minus(_pt_seg(p, a, b), ob.r)
    return _pt_poly(p, V)


def _dist_segment(s, e, ob, t):
    a, b, V = ob.at(t)
    if ob.type == OB_POINT: return _pt_seg(a, s, e)
    if ob.type == OB_CIRCULAR: return _minus(_pt_seg(a, s, e), ob.r)
    if ob.type == OB_LINE: return _seg_seg(a, b, s, e)
    if ob.type == OB_PILL: return _minus(_seg_seg(a, b, s, e), ob.r)
    return _seg_poly(s, e, V)


def _dist_polygon(W, ob, t):
    a, b, V = ob.at(t)
    if ob.type == OB_POINT: return _pt_poly(a, W)
    if ob.type == OB_CIRCULAR: return _minus(_pt_poly(a, W), ob.r)
    if ob.type == OB_LINE: return _seg_poly(a, b, W)
    if ob.type == OB_PILL: return _minus(_seg_poly(a, b, W), ob.r)
    return _poly_poly(W, V)


def _footprint_distance(cx, P, x, y, th, ob, t):
    fp = P.fp
    if fp.type == FP_POINT:
        r = _dist_point((x, y), ob, t)
    elif fp.type == FP_CIRCULAR:
        r = _minus(_dist_point((x, y), ob, t), P.fp_radius)
    elif fp.type == FP_TWO_CIRCLES:
        c, s = mpmath.cos(th), mpmath.sin(th)
        front = _minus(_dist_point((x + P.fp_front_offset * c, y + P.fp_front_offset * s), ob, t), P.fp_front_radius)
        rear = _minus(_dist_point((x - P.fp_rear_offset * c, y - P.fp_rear_offset * s), ob, t), P.fp_rear_radius)
        r = _argmin([(front[0], front[1], ("front",) + front[2], False), (rear[0], rear[1], ("rear",) + rear[2], False)])
    else:
        c, s = mpmath.cos(th), mpmath.sin(th)
        W = [(x + c * vx - s * vy, y + s * vx + c * vy) for vx, vy in P.fp_verts]
        r = _dist_segment(W[0], W[1], ob, t) if fp.type == FP_LINE else _dist_polygon(W, ob, t)
    cx.note("closest feature (u from 0 / 1, runner-up gap, touching)", r[1])
    return r[0]


# ---- the edges: residual rows as functions of the edge's own variables -----------------------------------------------------------
# every function returns a list of (residual, side) with side = -1 / 0 / +1: which side of its penalty the row is on
class _Params:
    def __init__(self, cfg, wm):
        f = lambda v: mpf(float(v))
        r, o, w = cfg.robot, cfg.obstacles, cfg.optim
        self.exact_arc = bool(cfg.trajectory.exact_arc_length)
        for k in ("max_vel_x", "max_vel_x_backwards", "max_vel_y", "max_vel_trans", "max_vel_theta", "acc_lim_x", "acc_lim_y",
                  "acc_lim_theta", "min_turning_radius"):
            setattr(self, k, f(getattr(r, k)))
        for k in ("min_obstacle_dist", "inflation_dist", "dynamic_obstacle_inflation_dist", "obstacle_proximity_ratio_max_vel",
                  "obstacle_proximity_lower_bound", "obstacle_proximity_upper_bound"):
            setattr(self, k, f(getattr(o, k)))
        self.eps = f(w.penalty_epsilon)
        self.exponent = f(w.obstacle_cost_exponent)
        self.use_exponent = float(w.obstacle_cost_exponent) != 1.0 and float(o.min_obstacle_dist) > 0.0
        wm = f(wm)   # enters the static obstacle weight only: buildGraph calls AddEdgesDynamicObstacles with its default multiplier 1
        W = lambda k: f(getattr(w, k))
        self.weights = {
            E_OBST: [W("weight_obstacle") * wm], E_INFL: [W("weight_obstacle") * wm, W("weight_inflation")],
            E_DYN: [W("weight_dynamic_obstacle"), W("weight_dynamic_obstacle_inflation")], E_VIA: [W("weight_viapoint")],
            E_VEL: [W("weight_max_vel_x"), W("weight_max_vel_theta")],
            E_VELH: [W("weight_max_vel_x"), W("weight_max_vel_y"), W("weight_max_vel_theta")],
            E_TIME: [W("weight_optimaltime")], E_SP: [W("weight_shortest_path")],
            E_KDD: [W("weight_kinematics_nh"), W("weight_kinematics_forward_drive")],
            E_KCL: [W("weight_kinematics_nh"), W("weight_kinematics_turning_radius")], E_ROT: [W("weight_prefer_rotdir")],
            E_VOR: [W("weight_velocity_obstacle_ratio")] * 2}
        for t in (E_ACC, E_ACCS, E_ACCG):
            self.weights[t] = [W("weight_acc_lim_x"), W("weight_acc_lim_theta")]
        for t in (E_ACCH, E_ACCHS, E_ACCHG):
            self.weights[t] = [W("weight_acc_lim_x"), W("weight_acc_lim_y"), W("weight_acc_lim_theta")]
        m = cfg.robot_model
        self.fp = m
        self.fp_radius = f(m.radius)
        self.fp_front_offset, self.fp_front_radius = f(m.front_offset), f(m.front_radius)
        self.fp_rear_offset, self.fp_rear_radius = f(m.rear_offset), f(m.rear_radius)
        self.fp_verts = [(f(a), f(b)) for a, b in m.vertices]


def _obstacle_rows(cx, P, dist, inflated):
    e0, s0 = _below(cx, "obstacle distance (min_obstacle_dist)", dist, P.min_obstacle_dist, P.eps)
    if P.use_exponent:
        e0 = P.min_obstacle_dist * (e0 / P.min_obstacle_dist) ** P.exponent if e0 != 0 else mpf(0)
    rows = [(e0, s0)]
    if inflated:
        rows.append(_below(cx, "obstacle distance (inflation_dist)", dist, P.inflation_dist, mpf(0)))
    return rows


def _r_velocity(cx, P, v, aux):
    vel, om = _signed_velocity(cx, P, *v)
    return [_interval2(cx, "velocity", vel, -P.max_vel_x_backwards, P.max_vel_x, P.eps),
            _interval(cx, "angular velocity", om, P.max_vel_theta, P.eps)]


def _body_velocity(cx, x0, y0, t0, x1, y1, t1, dt):
    dx, dy = x1 - x0, y1 - y0
    c, s = mpmath.cos(t0), mpmath.sin(t0)
    return (c * dx + s * dy) / dt, (-s * dx + c * dy) / dt, _norm_theta(cx, t1 - t0) / dt


def _min_cfg(cx, what, remaining, limit):
    """std::min(remaining, limit)"""
    cx.note("holonomic min() choice (" + what + ")", abs(remaining - limit))
    return limit if limit < remaining else remaining


def _r_velocity_holonomic(cx, P, v, aux):
    vx, vy, om = _body_velocity(cx, *v)
    vt2 = P.max_vel_trans * P.max_vel_trans
    cx.note("vt^2 - vx^2 from 0", abs(vt2 - vx * vx)); cx.note("vt^2 - vy^2 from 0", abs(vt2 - vy * vy))
    rem_y = mpmath.sqrt(max(mpf(0), vt2 - vx * vx)); rem_x = mpmath.sqrt(max(mpf(0), vt2 - vy * vy))
    lim_y = _min_cfg(cx, "max_vel_y", rem_y, P.max_vel_y)
    lim_x = _min_cfg(cx, "max_vel_x", rem_x, P.max_vel_x)
    lim_xb = _min_cfg(cx, "max_vel_x_backwards", rem_x, P.max_vel_x_backwards)
    return [_interval2(cx, "vx", vx, -lim_xb, lim_x, mpf(0)), _interval(cx, "vy", vy, lim_y, mpf(0)),
            _interval(cx, "angular velocity", om, P.max_vel_theta, P.eps)]


def _r_acceleration(cx, P, v, aux):
    x0, y0, t0, x1, y1, t1, x2, y2, t2, d0, d1 = v
    v1, o1 = _signed_velocity(cx, P, x0, y0, t0, x1, y1, t1, d0)
    v2, o2 = _signed_velocity(cx, P, x1, y1, t1, x2, y2, t2, d1)
    T = d0 + d1
    return [_interval(cx, "acceleration", (v2 - v1) * 2 / T, P.acc_lim_x, P.eps),
            _interval(cx, "angular acceleration", (o2 - o1) * 2 / T, P.acc_lim_theta, P.eps)]


def _r_acceleration_start(cx, P, v, aux):
    vel, om = _signed_velocity(cx, P, *v)
    dt = v[6]
    return [_interval(cx, "acceleration", (vel - aux[0]) / dt, P.acc_lim_x, P.eps),
            _interval(cx, "angular acceleration", (om - aux[2]) / dt, P.acc_lim_theta, P.eps)]


def _r_acceleration_goal(cx, P, v, aux):
    vel, om = _signed_velocity(cx, P, *v)
    dt = v[6]
    return [_interval(cx, "acceleration", (aux[0] - vel) / dt, P.acc_lim_x, P.eps),
            _interval(cx, "angular acceleration", (aux[2] - om) / dt, P.acc_lim_theta, P.eps)]


def _acc_rows3(cx, P, ax, ay, ar):
    return [_interval(cx, "acceleration x", ax, P.acc_lim_x, P.eps), _interval(cx, "acceleration y", ay, P.acc_lim_y, P.eps),
            _interval(cx, "angular acceleration", ar, P.acc_lim_theta, P.eps)]


def _r_acceleration_holonomic(cx, P, v, aux):
    x0, y0, t0, x1, y1, t1, x2, y2, t2, d0, d1 = v
    a = _body_velocity(cx, x0, y0, t0, x1, y1, t1, d0)
    b = _body_velocity(cx, x1, y1, t1, x2, y2, t2, d1)
    T = d0 + d1
    return _acc_rows3(cx, P, (b[0] - a[0]) * 2 / T, (b[1] - a[1]) * 2 / T, (b[2] - a[2]) * 2 / T)


def _r_acceleration_holonomic_start(cx, P, v, aux):
    b = _body_velocity(cx, *v)
    dt = v[6]
    return _acc_rows3(cx, P, (b[0] - aux[0]) / dt, (b[1] - aux[1]) / dt, (b[2] - aux[2]) / dt)


def _r_acceleration_holonomic_goal(cx, P, v, aux):
    a = _body_velocity(cx, *v)
    dt = v[6]
    return _acc_rows3(cx, P, (aux[0] - a[0]) / dt, (aux[1] - a[1]) / dt, (aux[2] - a[2]) / dt)


def _nh(cx, x0, y0, t0, x1, y1, t1):
    val = (mpmath.cos(t0) + mpmath.cos(t1)) * (y1 - y0) - (mpmath.sin(t0) + mpmath.sin(t1)) * (x1 - x0)
    return (_abs(cx, "non-holonomic constraint", val), 1 if val > 0 else (-1 if val < 0 else 0))


def _r_kinematics_diff_drive(cx, P, v, aux):
    x0, y0, t0, x1, y1, t1 = v
    return [_nh(cx, *v), _below(cx, "forward projection", (x1 - x0) * mpmath.cos(t0) + (y1 - y0) * mpmath.sin(t0), mpf(0), mpf(0))]


def _r_kinematics_carlike(cx, P, v, aux):
    x0, y0, t0, x1, y1, t1 = v
    ad = _norm_theta(cx, t1 - t0)
    if not (cx.allow_exact_zero and ad == 0):
        cx.note("angle difference from 0 (car-like)", abs(ad))
    n = mpmath.sqrt((x1 - x0) ** 2 + (y1 - y0) ** 2)
    cx.note("||dS|| from 0", n)
    if ad == 0:
        row = (mpf(0), 0)
    elif P.exact_arc:
        row = _below(cx, "turning radius", abs(n / (2 * mpmath.sin(ad / 2))), P.min_turning_radius, mpf(0))
    else:
        row = _below(cx, "turning radius", n / abs(ad), P.min_turning_radius, mpf(0))
    return [_nh(cx, *v), row]


def _r_time_optimal(cx, P, v, aux):
    return [(v[0], 1)]


def _r_shortest_path(cx, P, v, aux):
    n = mpmath.sqrt((v[3] - v[0]) ** 2 + (v[4] - v[1]) ** 2)
    cx.note("||dS|| from 0", n)
    return [(n, 1)]


def _r_prefer_rotdir(cx, P, v, aux):
    return [_below(cx, "preferred rotation", aux * _norm_theta(cx, v[5] - v[2]), mpf(0), mpf(0))]


def _r_via_point(cx, P, v, aux):
    n = mpmath.sqrt((v[0] - aux[0]) ** 2 + (v[1] - aux[1]) ** 2)
    cx.note("distance to the via-point from 0", n)
    return [(n, 1)]


def _r_obstacle(cx, P, v, aux):
    return _obstacle_rows(cx, P, _footprint_distance(cx, P, v[0], v[1], v[2], aux, None), False)


def _r_inflated_obstacle(cx, P, v, aux):
    return _obstacle_rows(cx, P, _footprint_distance(cx, P, v[0], v[1], v[2], aux, None), True)


def _r_dynamic_obstacle(cx, P, v, aux):
    ob, t = aux
    dist = _footprint_distance(cx, P, v[0], v[1], v[2], ob, t)
    return [_below(cx, "obstacle distance (min_obstacle_dist)", dist, P.min_obstacle_dist, P.eps),
            _below(cx, "obstacle distance (dynamic_obstacle_inflation_dist)", dist, P.dynamic_obstacle_inflation_dist, mpf(0))]


def _r_velocity_obstacle_ratio(cx, P, v, aux):
    vel, om = _signed_velocity(cx, P, *v)
    d = _footprint_distance(cx, P, v[0], v[1], v[2], aux, None)
    lo, hi = P.obstacle_proximity_lower_bound, P.obstacle_proximity_upper_bound
    cx.note("obstacle distance from obstacle_proximity_lower_bound", abs(d - lo))
    cx.note("obstacle distance from obstacle_proximity_upper_bound", abs(d - hi))
    ratio = mpf(0) if d < lo else (mpf(1) if d > hi else (d - lo) / (hi - lo))
    ratio *= P.obstacle_proximity_ratio_max_vel
    return [_interval(cx, "velocity (ratio bound)", vel, ratio * P.max_vel_x, mpf(0)),
            _interval(cx, "angular velocity (ratio bound)", om, ratio * P.max_vel_theta, mpf(0))]


_RESIDUAL = {E_OBST: _r_obstacle, E_INFL: _r_inflated_obstacle, E_DYN: _r_dynamic_obstacle, E_VIA: _r_via_point, E_VEL: _r_velocity,
             E_VELH: _r_velocity_holonomic, E_ACC: _r_acceleration, E_ACCS: _r_acceleration_start, E_ACCG: _r_acceleration_goal,
             E_ACCH: _r_acceleration_holonomic, E_ACCHS: _r_acceleration_holonomic_start, E_ACCHG: _r_acceleration_holonomic_goal,
             E_TIME: _r_time_optimal, E_SP: _r_shortest_path, E_KDD: _r_kinematics_diff_drive, E_KCL: _r_kinematics_carlike,
             E_ROT: _r_prefer_rotdir, E_VOR: _r_velocity_obstacle_ratio}
_CATEGORY = {E_OBST: CAT_OBST, E_INFL: CAT_OBST, E_DYN: CAT_OBST, E_VIA: CAT_VIA, E_TIME: CAT_TIME}


class _Graph:
    """the state of band b and what an edge record needs to be evaluated"""

    def __init__(self, cfg, obst, via, batch, b, wm):
        self.n = n = int(batch.n[b])
        f = self.f = lambda v: mpf(float(v))
        self.X = X = [[f(batch.x[b, i]), f(batch.y[b, i]), f(batch.theta[b, i]), f(batch.dt[b, i])] for i in range(n)]
        self.P = _Params(cfg, wm)
        self.obst, self.via, self.batch, self.b, self.obs = obst, via, batch, b, {}
        self.stamp = [mpf(0)] * n   # time of pose i as AddEdgesDynamicObstacles accumulates it (constant within one linearisation)
        for i in range(1, n):
            self.stamp[i] = self.stamp[i - 1] + X[i - 1][3]

    def edge(self, rec):
        """(type, global variable indices, fixed flags, values, the edge's constant data)"""
        n, X, f, batch, b = self.n, self.X, self.f, self.batch, self.b
        ty, npose, nd = int(rec[0]), int(rec[1]), int(rec[5])
        poses = [int(rec[2 + k]) for k in range(npose)]
        dts = [int(rec[6 + k]) for k in range(nd)]
        var = [4 * i + c for i in poses for c in range(3)] + [4 * i + 3 for i in dts]
        fixed = [i == 0 or i == n - 1 for i in poses for c in range(3)] + [i >= n - 1 for i in dts]
        val = [X[i][c] for i in poses for c in range(3)] + [X[i][3] for i in dts]
        oi, vi = int(rec[9]), int(rec[10])
        if ty in (E_OBST, E_INFL, E_DYN, E_VOR) and oi not in self.obs:
            self.obs[oi] = _Obstacle(self.obst, oi)
        aux = None
        if ty in (E_OBST, E_INFL, E_VOR): aux = self.obs[oi]
        elif ty == E_DYN: aux = (self.obs[oi], self.stamp[poses[0]])
        elif ty == E_VIA: aux = (f(self.via[vi][0]), f(self.via[vi][1]))
        elif ty in (E_ACCS, E_ACCHS): aux = [f(q) for q in batch.vel_start[b]]
        elif ty in (E_ACCG, E_ACCHG): aux = [f(q) for q in batch.vel_goal[b]]
        elif ty == E_ROT: aux = {0: mpf(1), 2: mpf(-1)}[int(batch.prefer_rotdir[b])]   # preferLeft(): +1, preferRight(): -1
        return ty, var, fixed, val, aux


def switch_arguments(cfg, obst, via, batch, b, wm, irec, only=None):
    """per edge record: [(name, argument, lower switch point or None, upper switch point or None)] of every penalty and |.| it
    evaluates, as floats - what the cases next to a kink are built from and checked with"""
    with mpmath.workdps(DPS):
        g = _Graph(cfg, obst, via, batch, b, wm)
        out = []
        for e, rec in enumerate(irec):
            if only is not None and e not in only:
                out.append([])
                continue
            ty, var, fixed, val, aux = g.edge(rec)
            cx = _Ctx(True)
            cx.args = []
            _RESIDUAL[ty](cx, g.P, val, aux)
            out.append([(w, float(v), None if lo is None else float(lo), None if hi is None else float(hi)) for w, v, lo, hi in cx.args])
        return out


EXEMPT_ULPS = 4


def _check_exempt(g, rec, names):
    """An exempted penalty argument must be EXACT in fp64 (every operation rounded to 53 bits gives the 80-digit value, switch points
    included) and lie at least EXEMPT_ULPS ulp (of the smaller of the two numbers) from each switch point: an fp64 implementation then
    holds the same argument on the same side, and delta = 1e-30 stays on that side too."""
    ty, var, fixed, val, aux = g.edge(rec)
    logs = []
    for prec in (None, 53):
        cx = _Ctx(False)
        cx.on, cx.args = False, []
        with (mpmath.workprec(prec) if prec else mpmath.workdps(DPS)):
            _RESIDUAL[ty](cx, g.P, list(val), aux)
        logs.append(cx.args)
    seen = set()
    for (w, v, lo, hi), (w64, v64, lo64, hi64) in zip(*logs):
        if w not in names:
            continue
        seen.add(w)
        if not (w == w64 and v == v64 and lo == lo64 and hi == hi64):
            raise BranchMarginError("exempted argument '%s' is not exact in fp64: %s" % (w, mpmath.nstr(v, 25)))
        for thr in (lo, hi):
            if thr is not None:
                ulp = float(np.spacing(min(abs(float(v)), abs(float(thr)))))
                if abs(v - thr) < EXEMPT_ULPS * ulp:
                    raise BranchMarginError("exempted argument '%s' is %s from its switch point: less than %d ulp" % (w, mpmath.nstr(abs(v - thr), 5), EXEMPT_ULPS))
    if seen != set(names):
        raise BranchMarginError("exempted arguments %s are not evaluated by this edge" % sorted(set(names) - seen))


def linearize(cfg, obst, via, batch, b, wm, irec, kink_delta=None, exempt=None):
    """The reference linearisation of band b. irec: the edge records of oracle.edges() (only their integer part is read).
    exempt: {(index into irec, name of a penalty argument)} - pairs left out of the MARGIN check on the distance from their switch points
    (cases that sit ON a threshold by construction, tests/hp_association.py); each is accepted only under _check_exempt.
    Returns dict(H {(a, c): mpf, a >= c}, b [4n] mpf, chi2 [4] mpf, rows {(type, row): [rows, non-zero, side +, side -]},
    ring_only / inside (inflated static obstacle rows), margin, margin_what, n)."""
    with mpmath.workdps(DPS):
        g = _Graph(cfg, obst, via, batch, b, wm)
        n, P = g.n, g.P
        delta = mpf(10) ** -30 if kink_delta is None else mpf(kink_delta)
        cx = _Ctx(kink_delta is not None)
        H, bv, chi2 = {}, [mpf(0)] * (4 * n), [mpf(0)] * 4
        rows, ring_only, inside = {}, 0, 0
        by_edge = {}
        for e, name in (exempt or ()):
            by_edge.setdefault(int(e), set()).add(name)
        for e, rec in enumerate(irec):
            ty, var, fixed, val, aux = g.edge(rec)
            fun, w = _RESIDUAL[ty], P.weights[ty]
            cx.exempt = by_edge.get(e, ())
            if cx.exempt:
                _check_exempt(g, rec, cx.exempt)
            cx.on = True
            base = fun(cx, P, val, aux)
            cx.on = False
            assert len(base) == len(w) == int(rec[8])
            for k, (e, side) in enumerate(base):
                st = rows.setdefault((ty, k), [0, 0, 0, 0])
                st[0] += 1; st[1] += e != 0; st[2] += side > 0; st[3] += side < 0
                chi2[_CATEGORY.get(ty, CAT_OTHER)] += w[k] * e * e
            if ty == E_INFL:
                inside += base[0][0] != 0
                ring_only += base[0][0] == 0 and base[1][0] != 0
            J = [[None] * len(var) for _ in base]
            for q in range(len(var)):
                if fixed[q]:
                    continue
                v0 = val[q]
                val[q] = v0 + delta; ep = fun(cx, P, val, aux)
                val[q] = v0 - delta; em = fun(cx, P, val, aux)
                val[q] = v0
                for k in range(len(base)):
                    J[k][q] = (ep[k][0] - em[k][0]) / (2 * delta)
            for k, (e, side) in enumerate(base):
                if w[k] == 0:
                    continue
                nz = [q for q in range(len(var)) if J[k][q] is not None and J[k][q] != 0]
                for q in nz:
                    bv[var[q]] -= w[k] * J[k][q] * e
                    for p in nz:
                        if var[p] <= var[q]:
                            H[(var[q], var[p])] = H.get((var[q], var[p]), mpf(0)) + w[k] * J[k][q] * J[k][p]
        if cx.margin < MARGIN:
            raise BranchMarginError("%s: %s < %g" % (cx.what, mpmath.nstr(cx.margin, 5), MARGIN))
        return dict(H=H, b=bv, chi2=chi2, rows=rows, ring_only=int(ring_only), inside=int(inside), margin=float(cx.margin),
                    margin_what=cx.what, n=n)


# ---- fp64 views and the metric -----------------------------------------------------------------------------------------------------
def to_band(R):
    """H as its lower band [4n][BAND + 1] (column d holds H[a, a - d]), b [4n], chi2 [4], all float64 rounded from 80 digits. An entry
    outside the band is an error: no edge couples variables that far apart."""
    n = R["n"]
    Hb = np.zeros((4 * n, BAND + 1))
    for (a, c), v in R["H"].items():
        assert 0 <= a - c <= BAND, ("entry outside the band", a, c)
        Hb[a, a - c] = float(v)
    return Hb, np.array([float(v) for v in R["b"]]), np.array([float(v) for v in R["chi2"]])


def band_of_dense(H):
    """the lower band of a dense symmetric H [4n, 4n]; everything outside it must be exactly 0"""
    N = H.shape[0]
    Hb = np.zeros((N, BAND + 1))
    for d in range(BAND + 1):
        Hb[d:, d] = np.diagonal(H, -d)
    mask = np.abs(np.subtract.outer(np.arange(N), np.arange(N))) > BAND
    assert not H[mask].any(), "non-zero entry of H outside the band"
    assert np.array_equal(H, H.T), "H is not symmetric"
    return Hb


def errors(Hb, bv, Hb_ref, b_ref, chi2_ref):
    """(H error, b error) in the floored local metric: d_a = H_ref[a, a], D_k = max d_a over the variables of kind k (x, y, theta, dt),
    f_a = max(d_a, 1e-6 D_kind(a)); H error = max |H - H_ref|[a, c] / sqrt(f_a f_c), b error = max |b - b_ref|[a] / sqrt(f_a chi2_ref).
    An entry whose scale is exactly 0 must be exactly 0 (asserted here)."""
    N = Hb_ref.shape[0]
    d = Hb_ref[:, 0]
    f = np.zeros(N)
    for k in range(4):
        f[k::4] = np.maximum(d[k::4], 1e-6 * d[k::4].max())
    eH, eb = 0.0, 0.0
    for dd in range(BAND + 1):
        s = np.sqrt(f[dd:] * f[:N - dd])
        diff = np.abs(Hb[dd:, dd] - Hb_ref[dd:, dd])
        zero = s == 0
        assert not diff[zero].any() and not Hb[dd:, dd][zero].any(), "entry of H with scale 0 is not 0"
        if (~zero).any():
            eH = max(eH, float((diff[~zero] / s[~zero]).max()))
    s = np.sqrt(f * chi2_ref.sum())
    diff = np.abs(bv - b_ref)
    zero = s == 0
    assert not diff[zero].any() and not bv[zero].any(), "entry of b with scale 0 is not 0"
    if (~zero).any():
        eb = max(eb, float((diff[~zero] / s[~zero]).max()))
    return eH, eb


def input_hash(cfg, obst, via, batch, b):
    """sha256 over the scene: everything but the edge list that the reference (and the code under test) reads"""
    h = hashlib.sha256()
    n = int(batch.n[b])
    h.update(bytes(cfg.to_c()))
    for a in (obst.type, obst.ax, obst.ay, obst.bx, obst.by, obst.radius, obst.vx, obst.vy, obst.dynamic, obst.vert_offset, obst.vert_x,
              obst.vert_y):
        h.update(np.asarray(a, np.float64).tobytes())
    h.update(np.asarray(via, np.float64).tobytes())
    for a in (batch.x[b, :n], batch.y[b, :n], batch.theta[b, :n], batch.dt[b, :n], batch.vel_start[b], batch.vel_goal[b]):
        h.update(np.ascontiguousarray(a, np.float64).tobytes())
    h.update(np.asarray([n, batch.has_vel_start[b], batch.has_vel_goal[b], batch.prefer_rotdir[b], batch.via_points_enabled[b]],
                        np.int64).tobytes())
    return h.hexdigest()


def edges_hash(irec):
    return hashlib.sha256(np.ascontiguousarray(irec, np.int32).tobytes()).hexdigest()
