"""Exact reference of the DECISIONS of the exploration graph: which vertices exist and which ordered pairs carry an edge. NOT a test file.

It restates lrKeyPointGraph::createGraph (src/graph_search.cpp:93-213) and ProbRoadmapGraph::createGraph (:220-340) of the reference
planner with Obstacle::checkLineIntersection of all five obstacle types (obstacles.h:339-354, 483-498, 647-650, 794-797,
src/obstacles.cpp:178-191) and check_line_segments_intersection_2d (distance_calculations.h:97-127) as plain loops. The loops are
written ONCE over a number type and run in two ways:
  mode "float": every operation one Python float operation. All of them are IEEE + - * / sqrt (and libm's cos / sin / atan2 on the
                host side), so this is what a correct fp64 implementation without contraction must compute;
  mode "both":  every value carries its fp64 evaluation AND its evaluation with mpmath at 80 digits on the same fp64 inputs, plus the
                magnitude it would have had without cancellation (the sum of the absolute values of what was added or subtracted).
Every comparison is recorded with its kind, its relative margin |a - b| / max(magnitude of a, magnitude of b), its outcome, and one of
three classes:
  SEPARATED  relative margin >= REL = 1e-9 (the admissibility rule of tests/hp_association.py): any fp64 evaluation decides alike;
             the fp64 outcome must equal the 80-digit one;
  EXACT      both fp64 operands equal their 80-digit values: a tie or one ulp is then legitimate, both evaluations agree; or the two
             operands tie in BOTH evaluations (the same operations on bit-equal inputs, as for two obstacles at one distance);
  RUNG       the case placed a threshold (or a coordinate) k ulp from the fp64-evaluated quantity on purpose and names the kind in
             case["rungs"]: the expectation is the op-by-op fp64 outcome.
Anything else raises InadmissibleError. No comparison and no case is ever dropped.

A division by zero gives what IEEE gives (an obstacle exactly on the start: 0 / 0 = NaN, every comparison with it false - the obstacle
gets its key points; a zero-length edge against a point obstacle: t = NaN, no hit).

`mut` names one deliberate error of the restatement (MUTATIONS): the CPU test shows that each changes the graph of at least one case.
"""
import math
import sys

import numpy as np

try:
    import mpmath
    from mpmath import mpf
except ImportError:   # the GPU test reads fixtures only
    mpmath, mpf = None, None

DPS = 80
REL = 1e-9
SEPARATED, EXACT, RUNG = 0, 1, 2
KINDS = ["goal_tol", "norm0", "front", "near", "fwd", "head", "tlo", "thi", "dmin", "denom0", "s_lo", "t_lo", "s_hi", "t_hi", "draw"]
KIND_ID = {k: i for i, k in enumerate(KINDS)}
OB_POINT, OB_CIRCULAR, OB_LINE, OB_PILL, OB_POLYGON = 0, 1, 2, 3, 4   # checked against _abi in the CPU test

MUTATIONS = {
    "fwd_lt": "'<' for '<=' in the forward test",
    "head_lt": "'<' for '<=' in the start-heading test",
    "dmin_le": "'<=' for '<' against min_dist",
    "no_lo_clamp": "t not clamped at 0",
    "no_hi_clamp": "t not clamped at 1",
    "no_radius": "radius of a circular obstacle ignored",
    "denom_ge": "'>=' for '>' against denom",
    "denom0_cross": "denom == 0 taken as a crossing",
    "no_closing": "closing edge of a polygon dropped",
    "no_half": "0.5 * dropped from the key-point graph's min_dist",
    "front_le": "'<=' for '<' against 0.1",
    "near_le": "a tie for the nearest obstacle resolved towards the later one",
    "fma": "cross products fused: fma(a, b, -(c * d))",
}
_OPS = {"<": lambda a, b: a < b, "<=": lambda a, b: a <= b, ">": lambda a, b: a > b, ">=": lambda a, b: a >= b, "==": lambda a, b: a == b}
_MUT_OP = {"fwd_lt": ("fwd", "<"), "head_lt": ("head", "<"), "dmin_le": ("dmin", "<="), "front_le": ("front", "<="), "near_le": ("near", "<=")}


class InadmissibleError(ValueError):
    pass


def _fdiv(a, b):
    """IEEE a / b on Python floats"""
    if b == 0:
        if a == 0 or a != a:
            return math.nan
        return math.copysign(math.inf, a) * math.copysign(1.0, b)
    return a / b


class Dual:
    """f: the fp64 evaluation, m: the 80-digit one, s: the magnitude without cancellation"""
    __slots__ = ("f", "m", "s")

    def __init__(self, f, m=None, s=None):
        self.f = f
        self.m = mpf(f) if m is None else m
        self.s = abs(self.m) if s is None else s

    def __add__(a, b):
        b = _dual(b)
        return Dual(a.f + b.f, a.m + b.m, a.s + b.s)
    __radd__ = __add__

    def __sub__(a, b):
        b = _dual(b)
        return Dual(a.f - b.f, a.m - b.m, a.s + b.s)

    def __rsub__(a, b):
        return _dual(b) - a

    def __mul__(a, b):
        b = _dual(b)
        return Dual(a.f * b.f, a.m * b.m, a.s * b.s)
    __rmul__ = __mul__

    def __truediv__(a, b):
        b = _dual(b)
        if b.m == 0:
            return Dual(_fdiv(a.f, b.f), mpmath.nan if a.m == 0 or mpmath.isnan(a.m) else mpmath.inf * mpmath.sign(a.m), mpmath.inf)
        return Dual(_fdiv(a.f, b.f), a.m / b.m, a.s / abs(b.m))

    def __rtruediv__(a, b):
        return _dual(b) / a

    def __neg__(a):
        return Dual(-a.f, -a.m, a.s)


def _dual(x):
    return x if isinstance(x, Dual) else Dual(float(x))


def _f(x):
    return x.f if isinstance(x, Dual) else x


class MT19937:
    """std::mt19937 / boost::random::mt19937 with the default seed 5489: the 32-bit outputs"""

    def __init__(self, seed=5489):
        self.mt = [0] * 624
        self.mt[0] = seed & 0xffffffff
        for i in range(1, 624):
            self.mt[i] = (1812433253 * (self.mt[i - 1] ^ (self.mt[i - 1] >> 30)) + i) & 0xffffffff
        self.idx = 624

    def __call__(self):
        if self.idx >= 624:
            mt = self.mt
            for i in range(624):
                y = (mt[i] & 0x80000000) | (mt[(i + 1) % 624] & 0x7fffffff)
                mt[i] = mt[(i + 397) % 624] ^ (y >> 1) ^ (0x9908b0df if y & 1 else 0)
            self.idx = 0
        y = self.mt[self.idx]
        self.idx += 1
        y ^= y >> 11
        y ^= (y << 7) & 0x9d2c5680
        y ^= (y << 15) & 0xefc60000
        y ^= y >> 18
        return y & 0xffffffff


class Graph:
    """createGraph of one scene. case: dict(keypoint, start [3], goal [3], dist_to_obst, thr, obst (ObstacleTable-like columns),
    no_samples, area_width, length_scale, xy_goal_tolerance, rungs: set of kinds)."""

    def __init__(self, case, mode="both", mut=None):
        assert mode in ("both", "float") and (mut is None or mut in MUTATIONS)
        self.c, self.hp, self.mut = case, mode == "both", mut
        self.rungs = set(case.get("rungs", ()))
        self.records = []          # (kind id, class, relative margin, outcome, tie in fp64, sign of a - b in fp64)
        self.units = []            # the unit samples in the order drawn
        self.probe = {}            # fp64 values of the deciding quantities, for the case builders: (kind, i, j[, o]) -> value
        self._at = None
        ob = case["obst"]
        self.M = len(ob.type)
        self.ob = ob

    # ---- numbers
    def num(self, x):
        return Dual(float(x)) if self.hp else float(x)

    def sqrt(self, x):
        if not self.hp:
            return math.sqrt(x) if x == x and x >= 0 else math.nan
        if mpmath.isnan(x.m):
            return Dual(math.nan, mpmath.nan, mpmath.nan)
        return Dual(math.sqrt(x.f), mpmath.sqrt(x.m), mpmath.sqrt(x.s))

    def div(self, a, b):
        return a / b if self.hp else _fdiv(a, b)

    def libm(self, name, *args):
        """cos / sin / atan2 of the host's libm; at 80 digits on the 80-digit arguments"""
        if not self.hp:
            return getattr(math, name)(*args)
        f = getattr(math, name)(*[a.f for a in args])
        m = getattr(mpmath, name)(*[a.m for a in args])
        return Dual(f, m, max(abs(m), mpf(1)) if name != "atan2" else abs(m))

    def cross(self, a, b, c, d):
        """a * b - c * d"""
        if self.mut == "fma":
            p = _f(c) * _f(d)
            with mpmath.workdps(DPS):
                r = float(mpf(_f(a)) * mpf(_f(b)) - mpf(p))   # one rounding
            return Dual(r, a.m * b.m - c.m * d.m, a.s * b.s + c.s * d.s) if self.hp else r
        return a * b - c * d

    # ---- the recorded comparison
    def cmp(self, kind, a, op, b):
        if self.mut in _MUT_OP and _MUT_OP[self.mut][0] == kind:
            op = _MUT_OP[self.mut][1]
        if self.mut == "denom_ge" and kind in ("s_hi", "t_hi"):
            op = ">="
        af, bf = _f(a), _f(b)
        rf = _OPS[op](af, bf)
        if not self.hp:
            return rf
        a, b = _dual(a), _dual(b)
        sgn = (af > bf) - (af < bf)
        if af != af or bf != bf:
            if not (mpmath.isnan(a.m) or mpmath.isnan(b.m)):
                raise InadmissibleError("%s: NaN in fp64 only" % kind)
            self.records.append((KIND_ID[kind], EXACT, 0.0, False, False, 0))
            return False
        rm = _OPS[op](a.m, b.m)
        scale = max(a.s, b.s)
        rel = float(abs(a.m - b.m) / scale) if scale != 0 else (0.0 if a.m == b.m else math.inf)
        if rel >= REL:
            if rf != rm:
                raise InadmissibleError("%s: separated by %.3g and fp64 decides differently (%r %s %r)" % (kind, rel, af, op, bf))
            cls = SEPARATED
        elif (mpf(af) == a.m and mpf(bf) == b.m) or (af == bf and a.m == b.m):
            assert rf == rm
            cls = EXACT
        elif kind in self.rungs:
            cls = RUNG
        else:
            raise InadmissibleError("%s: relative margin %.3g < %g, operands not exact in fp64, no rung declared (%r %s %r; %s, %s)"
                                    % (kind, rel, REL, af, op, bf, mpmath.nstr(a.m, 25), mpmath.nstr(b.m, 25)))
        self.records.append((KIND_ID[kind], cls, rel, bool(rf), af == bf, sgn))
        return rf

    # ---- Eigen normalize(): v /= sqrt(squaredNorm) when squaredNorm > 0
    def normalize(self, x, y):
        z = x * x + y * y
        if self.cmp("norm0", z, ">", 0.0):
            n = self.sqrt(z)
            return self.div(x, n), self.div(y, n)
        return x, y

    # ---- check_line_segments_intersection_2d
    def segments_intersect(self, s1, e1, s2, e2):
        l1x, l1y = e1[0] - s1[0], e1[1] - s1[1]
        l2x, l2y = e2[0] - s2[0], e2[1] - s2[1]
        denom = self.cross(l1x, l2y, l2x, l1y)
        if self.cmp("denom0", denom, "==", 0.0):
            return self.mut == "denom0_cross"
        dp = _f(denom) > 0   # the sign of a number that is not zero: decided by the comparison above
        auxx, auxy = s1[0] - s2[0], s1[1] - s2[1]
        s_numer = self.cross(l1x, auxy, l1y, auxx)
        self.probe[("s_numer",) + self._at] = _f(s_numer)
        if self.cmp("s_lo", s_numer, "<", 0.0) == dp:
            return False
        t_numer = self.cross(l2x, auxy, l2y, auxx)
        if self.cmp("t_lo", t_numer, "<", 0.0) == dp:
            return False
        if self.cmp("s_hi", s_numer, ">", denom) == dp:
            return False
        if self.cmp("t_hi", t_numer, ">", denom) == dp:
            return False
        return True

    # ---- Obstacle::checkLineIntersection
    def line_hits_obstacle(self, o, s, e, min_dist):
        ob, ty = self.ob, int(self.ob.type[o])
        if ty in (OB_POINT, OB_CIRCULAR):
            ax, ay = e[0] - s[0], e[1] - s[1]
            px, py = self.num(ob.ax[o]), self.num(ob.ay[o])
            bx, by = px - s[0], py - s[1]
            t = self.div(ax * bx + ay * by, ax * ax + ay * ay)
            if self.cmp("tlo", t, "<", 0.0):
                if self.mut != "no_lo_clamp":
                    t = self.num(0.0)
            elif self.cmp("thi", t, ">", 1.0):
                if self.mut != "no_hi_clamp":
                    t = self.num(1.0)
            nx, ny = s[0] + ax * t, s[1] + ay * t
            dx, dy = nx - px, ny - py
            d = self.sqrt(dx * dx + dy * dy)
            if ty == OB_CIRCULAR and self.mut != "no_radius":
                d = d - self.num(ob.radius[o])
            self.probe[("dmin",) + self._at + (o,)] = _f(d)
            return self.cmp("dmin", d, "<", min_dist)
        if ty in (OB_LINE, OB_PILL):
            return self.segments_intersect(s, e, (self.num(ob.ax[o]), self.num(ob.ay[o])), (self.num(ob.bx[o]), self.num(ob.by[o])))
        V = [(self.num(ob.vert_x[k]), self.num(ob.vert_y[k])) for k in range(ob.vert_offset[o], ob.vert_offset[o + 1])]
        for i in range(len(V) - 1):
            if self.segments_intersect(s, e, V[i], V[i + 1]):
                return True
        if len(V) == 2 or self.mut == "no_closing":
            return False
        return self.segments_intersect(s, e, V[-1], V[0])

    # ---- getCentroid
    def centroid(self, o):
        ob, ty = self.ob, int(self.ob.type[o])
        if ty in (OB_POINT, OB_CIRCULAR):
            return self.num(ob.ax[o]), self.num(ob.ay[o])
        if ty in (OB_LINE, OB_PILL):
            return 0.5 * (self.num(ob.ax[o]) + self.num(ob.bx[o])), 0.5 * (self.num(ob.ay[o]) + self.num(ob.by[o]))
        V = [(self.num(ob.vert_x[k]), self.num(ob.vert_y[k])) for k in range(ob.vert_offset[o], ob.vert_offset[o + 1])]
        m = len(V)
        if m == 1:
            return V[0]
        if m == 2:
            return 0.5 * (V[0][0] + V[1][0]), 0.5 * (V[0][1] + V[1][1])
        A = self.num(0.0)   # PolygonObstacle::calcCentroid, src/obstacles.cpp:56-121
        for i in range(m - 1):
            A = A + (V[i][0] * V[i + 1][1] - V[i + 1][0] * V[i][1])
        A = A + (V[m - 1][0] * V[0][1] - V[0][0] * V[m - 1][1])
        A = A * 0.5
        assert _f(A) != 0, "degenerate polygon: not restated here"
        cx, cy = self.num(0.0), self.num(0.0)
        for i in range(m):
            p, q = V[i], V[(i + 1) % m]
            aux = p[0] * q[1] - q[0] * p[1]
            cx = cx + (p[0] + q[0]) * aux
            cy = cy + (p[1] + q[1]) * aux
        return self.div(cx, 6 * A), self.div(cy, 6 * A)

    # ---- createGraph
    def run(self):
        """dict(vertices [N, 2] fp64, adjacency [N, N] uint8, near: (u, v) or (-1, -1)); N = 0: returned before the graph"""
        if self.hp:
            with mpmath.workdps(DPS):
                return self._run()
        return self._run()

    def _run(self):
        c = self.c
        sx, sy, sth = (self.num(v) for v in c["start"])
        gx, gy = self.num(c["goal"][0]), self.num(c["goal"][1])
        dist_to_obst, thr = self.num(c["dist_to_obst"]), self.num(c["thr"])
        dfx, dfy = gx - sx, gy - sy
        start_goal_dist = self.sqrt(dfx * dfx + dfy * dfy)
        if self.cmp("goal_tol", start_goal_dist, "<", c["xy_goal_tolerance"]):
            return dict(vertices=np.zeros((0, 2)), adjacency=np.zeros((0, 0), np.uint8), near=(-1, -1))
        nx, ny = self.normalize(-dfy, dfx)
        V = [(sx, sy)]
        near = (-1, -1)
        thr_on = _f(thr) != 0
        if c["keypoint"]:
            nx, ny = nx * dist_to_obst, ny * dist_to_obst
            dfx, dfy = self.normalize(dfx, dfy)
            min_d = self.num(sys.float_info.max)   # DBL_MAX
            for o in range(self.M):
                cx, cy = self.centroid(o)
                ox, oy = cx - sx, cy - sy
                dist = self.sqrt(ox * ox + oy * oy)
                q = self.div(ox * dfx + oy * dfy, dist)
                self.probe[("front", o)] = _f(q)
                if self.cmp("front", q, "<", 0.1):
                    continue
                V.append((cx + nx, cy + ny)); V.append((cx - nx, cy - ny))
                if thr_on and self.cmp("near", dist, "<", min_d):
                    min_d, near = dist, (len(V) - 2, len(V) - 1)
            min_dist = dist_to_obst if self.mut == "no_half" else 0.5 * dist_to_obst
        else:
            area_width, scale = self.num(c["area_width"]), self.num(c["length_scale"])
            length = start_goal_dist * scale
            phi = self.libm("atan2", dfy, dfx)
            w2 = 0.5 * area_width
            if float(c["length_scale"]) != 1.0:
                ux, uy = self.normalize(dfx, dfy)
                f = 0.5 * (1.0 - scale) * start_goal_dist
                ox, oy = (sx + f * ux) - w2 * nx, (sy + f * uy) - w2 * ny
            else:
                ox, oy = sx - w2 * nx, sy - w2 * ny
            dfx, dfy = self.normalize(dfx, dfy)
            gen = MT19937()

            def draw(b):   # boost::random::uniform_real_distribution<double>(0, b) on the 32-bit engine
                while True:
                    u = gen() / 4294967296.0
                    result = self.num(u) * (b - 0.0) + 0.0
                    if self.cmp("draw", result, "<", b):
                        self.units.append(u)
                        return result
            cphi, sphi = self.libm("cos", phi), self.libm("sin", phi)
            for _ in range(int(c["no_samples"])):
                uy = draw(area_width)   # GCC evaluates Eigen::Vector2d(distribution_x(g), distribution_y(g)) right to left
                ux = draw(length)
                V.append((ox + (cphi * ux - sphi * uy), oy + (sphi * ux + cphi * uy)))
            min_dist = dist_to_obst
        V.append((gx, gy))
        N = len(V)
        sox, soy = self.libm("cos", sth), self.libm("sin", sth)
        adj = np.zeros((N, N), np.uint8)
        for i in range(N - 1):
            for j in range(N):
                if i == j:
                    continue
                dx, dy = self.normalize(V[j][0] - V[i][0], V[j][1] - V[i][1])
                dot = dx * dfx + dy * dfy
                self.probe[("fwd", i, j)] = _f(dot)
                if self.cmp("fwd", dot, "<=", thr):
                    continue
                if c["keypoint"] and thr_on and i == 0 and near[0] >= 0 and j in near:
                    kx, ky = self.normalize(V[j][0] - sx, V[j][1] - sy)
                    dot = sox * kx + soy * ky
                    self.probe[("head", j)] = _f(dot)
                    if self.cmp("head", dot, "<=", thr):
                        continue
                self._at = (i, j)
                if any(self.line_hits_obstacle(o, V[i], V[j], min_dist) for o in range(self.M)):
                    continue
                adj[i, j] = 1
        return dict(vertices=np.array([[_f(v[0]), _f(v[1])] for v in V], np.float64).reshape(N, 2), adjacency=adj, near=near)

    # ---- what the records hold
    def record_array(self):
        """[n, 6] float64: kind id, class, relative margin, outcome, tie in fp64, sign of a - b in fp64"""
        return np.array(self.records, np.float64).reshape(-1, 6)


def summary(rec):
    """(comparisons, exact ones, ties, rungs, smallest relative margin of the separated ones)"""
    sep = rec[rec[:, 1] == SEPARATED, 2]
    return len(rec), int((rec[:, 1] == EXACT).sum()), int(rec[:, 4].sum()), int((rec[:, 1] == RUNG).sum()), float(sep.min()) if len(sep) else math.inf


# ---- fp64 helpers for the case builders -------------------------------------------------------------------------------------------------
def ulps(x, k):
    """x moved by k ulp"""
    for _ in range(abs(k)):
        x = math.nextafter(x, math.inf if k > 0 else -math.inf)
    return x


def ulp_distance(a, b):
    """the distance of two fp64 arrays in units in the last place (of their ordered-integer images), elementwise"""
    def key(v):
        i = np.ascontiguousarray(v, np.float64).view(np.int64)
        return np.where(i < 0, np.int64(-2 ** 63) - i, i)
    return np.abs(key(a) - key(b))


# ---- the fixture layout: per family one array per field, the cases one after the other (a zip entry per case and field would cost more
# than the data) --------------------------------------------------------------------------------------------------------------------------
SHAPES = {"vertices": (-1, 2), "ob_rows": (-1, 5), "ob_verts": (-1, 2)}


def pack(records):
    """records: {case name: {field: array}} -> {"names", "<field>", "<field>_off"}"""
    names = list(records)
    out = {"names": np.array(names)}
    for f in records[names[0]]:
        parts = [np.ascontiguousarray(records[n][f]).ravel() for n in names]
        out[f] = np.concatenate(parts)
        out[f + "_off"] = np.cumsum([0] + [len(q) for q in parts]).astype(np.int64)
    return out


def unpack(npz):
    """the inverse of pack: {case name: {field: array}}; adjacency comes back [N, N]"""
    names = [str(n) for n in npz["names"]]
    fields = [f[:-4] for f in npz.files if f.endswith("_off")]
    out = {}
    for k, n in enumerate(names):
        d = {}
        for f in fields:
            off = npz[f + "_off"]
            d[f] = npz[f][off[k]:off[k + 1]]
            if f in SHAPES:
                d[f] = d[f].reshape(SHAPES[f])
        N = len(d["vertices"])
        d["adjacency"] = d["adjacency"].reshape(N, N)
        out[n] = d
    return out
