"""Exact reference of the DECISIONS of the feasibility check: which cell a coordinate falls into, which cells an outline edge reads, which
return code wins, how many additional samples a segment gets, where the look-ahead ends. NOT a test file.

It restates TebOptimalPlanner::isTrajectoryFeasible (src/optimal_planner.cpp:1250-1308 of the reference planner) with, from the navigation
stack's published noetic sources (what oracle/grid_costmap.h cites), WorldModel::footprintCost(x, y, theta, spec),
CostmapModel::footprintCost / lineCost / pointCost, base_local_planner::LineIterator and costmap_2d::Costmap2D::worldToMap, and
g2o::normalize_theta, as plain loops. The loops are written ONCE over a number type and run in two ways (the scheme and the number type
of tests/hp_explore_graph.py):
  mode "float": every operation one Python float operation - the reference's arithmetic;
  mode "both":  every value carries its fp64 evaluation AND its evaluation with mpmath at 80 digits on the same fp64 inputs, plus the
                magnitude it would have had without cancellation.
Every comparison is recorded: (kind, class, relative margin, outcome, tie in fp64, sign). The kinds:
  w_lt_o      wx < ox, wy < oy                                  idx        cell index against the grid size (integers: always exact)
  trunc       distance of (w - o) / res from the nearest integer - the truncation decision; sign: fp64 quotient minus the exact one
  rot, dist   |delta_rot| > ang, dnorm > inscribed_radius       ceil_rot, ceil_dist   distance of the ceil argument from an integer
  max         which ceil wins (integers; tie: equal)            look       hypot(...) > lookahead_distance
  norm_lo / norm_hi / norm_floor / fix_hi / fix_lo              the branches of normalize_theta, on EVERY call
and one of three classes:
  SEPARATED  relative margin >= REL = 1e-9: any fp64 evaluation (any correct libm) decides alike; the fp64 outcome must equal the 80-digit one;
  EXACT      the fp64 operands equal their 80-digit values: a tie or one ulp is then legitimate;
  RUNG       the case named the kind in case["rungs"]: a quotient such as (wx - ox) / 0.05 or dnorm / r whose fp64 value lands on an
             integer that the exact quotient misses (or the like); the expectation is the op-by-op fp64 outcome.
Anything else raises InadmissibleError. No comparison and no case is ever dropped. A kind that goes through libm (look; every kind of a
case with a rotated outline) can never be a RUNG: LIBM_KINDS, asserted by the generator.

Besides the comparisons the run counts EVENTS (self.events): the return code of every footprint test, the negative codes that lay BEHIND
the deciding one (on the same edge / on a later edge: the precedence pairs), the octant of every rasterised edge, the diagonal tie, the
zero-length edge.

(int) of a NaN or of a value beyond the int range is formally undefined; x86 (cvttsd2si) gives INT_MIN, which worldToMap's unsigned
comparison turns into "off the map". That is what trunc() restates.

`mut` names one deliberate error of the restatement (MUTATIONS); the CPU test shows which cases notice each.
"""
import collections
import math

import numpy as np

from hp_explore_graph import DPS, REL, SEPARATED, EXACT, RUNG, Dual, InadmissibleError, _dual, _f, _fdiv, ulps  # noqa: F401

try:
    import mpmath
    from mpmath import mpf
except ImportError:   # the GPU test reads fixtures only
    mpmath, mpf = None, None

KINDS = ["w_lt_o", "idx", "trunc", "rot", "dist", "ceil_rot", "ceil_dist", "max", "look", "norm_lo", "norm_hi", "norm_floor", "fix_hi", "fix_lo"]
KIND_ID = {k: i for i, k in enumerate(KINDS)}
LIBM_KINDS = ("look",)
INT_MIN = -2 ** 31
LANES = 256   # kFeasThreads of csrc/teb_feasibility.hpp (checked in the CPU test)

MUTATIONS = {
    "rot_ge": "'>=' for '>' in the angular interpolation trigger",
    "dist_ge": "'>=' for '>' in the distance interpolation trigger",
    "w2m_recip": "* (1 / res) for / res in world_to_map",
    "w2m_floor": "floor for the truncating cast",
    "no_guard": "the wx < ox / wy < oy guard missing",
    "mx_le_sx": "mx <= sx accepted",
    "no_closing": "the closing edge dropped",
    "tie_ymajor": "the Bresenham tie deltax == deltay taken y-major",
    "num_round": "num = (den + 1) / 2",
    "253_lethal": "253 treated as lethal on an outline",
    "255_collision": "255 treated as a collision",
    "offmap_collision": "an off-map vertex or centre treated as a collision",
    "later_lethal": "a lethal cell seen although an earlier cell or vertex already returned -2 or -3",
    "closed_form": "additional samples in closed form p + k * delta / (n + 1)",
    "look_sqrt": "hypot replaced by sqrt(dx * dx + dy * dy)",
    "look_no_override": "the look-ahead distance only ever lowers look_ahead_idx",
    "lane_min": "the verdict of the lowest lane of the 256 instead of the lowest test",
    "bsearch_off": "a pose's own test attributed to the segment before it (one more step of that segment's recurrence)",
    "fleet_neighbour": "a scene of the per-scene call reads its neighbour's grid",
}
# Four of these cannot change any answer inside the scope (finite poses, positive parameters); the CPU test asserts that NO case notices
# them and says why: a trigger at the tie asks for max(ceil(<= 1), ..) - 1 samples, which the untriggered branch gives as well; floor and
# the cast differ only below zero, which the guard excludes; on the diagonal num = den / 2 < den and numadd = den, so the minor coordinate
# steps with every cell whichever axis is called major.
EQUIVALENT = ("rot_ge", "dist_ge", "w2m_floor", "tie_ymajor")
_OPS = {"<": lambda a, b: a < b, ">": lambda a, b: a > b, ">=": lambda a, b: a >= b}


class Grid:
    def __init__(self, cells, res, ox, oy):
        self.cells = np.ascontiguousarray(cells, np.uint8)
        self.sy, self.sx = self.cells.shape
        self.flat = self.cells.ravel()
        self.res, self.ox, self.oy = float(res), float(ox), float(oy)
        # what oracle.oracle_py.Costmap offers
        self.size_x, self.size_y, self.resolution, self.origin_x, self.origin_y = self.sx, self.sy, self.res, self.ox, self.oy


def line_cells(x0, x1, y0, y1, mut=None, events=None):
    """base_local_planner::LineIterator from (x0, y0) to (x1, y1): the cells in the order read"""
    deltax, deltay = abs(x1 - x0), abs(y1 - y0)
    x, y = x0, y0
    xinc1 = xinc2 = 1 if x1 >= x0 else -1
    yinc1 = yinc2 = 1 if y1 >= y0 else -1
    xmajor = deltax > deltay if mut == "tie_ymajor" else deltax >= deltay
    if xmajor:
        xinc1 = 0; yinc2 = 0; den = deltax; numadd = deltay
    else:
        xinc2 = 0; yinc1 = 0; den = deltay; numadd = deltax
    num = (den + 1) // 2 if mut == "num_round" else den // 2
    if events is not None:
        events["octant:%s%s%s" % ("+" if x1 >= x0 else "-", "+" if y1 >= y0 else "-", "x" if xmajor else "y")] += 1
        events["line:zero" if den == 0 else "line:diagonal" if deltax == deltay else "line:horizontal" if deltay == 0 else
               "line:vertical" if deltax == 0 else "line:off_by_one" if abs(deltax - deltay) == 1 else "line:general"] += 1
        events["line:den_%s" % ("odd" if den % 2 else "even")] += 1
    out = []
    for _ in range(den + 1):
        out.append((x, y))
        num += numadd
        if num >= den:
            num -= den; x += xinc1; y += yinc1
        x += xinc2; y += yinc2
    return out


def line_cells_closed_form(x0, x1, y0, y1):
    """The same cells with no loop state: step k has major offset k and minor offset floor((den // 2 + k * numadd) / den)"""
    dx, dy = x1 - x0, y1 - y0
    sx, sy = (1 if dx >= 0 else -1), (1 if dy >= 0 else -1)
    ax, ay = abs(dx), abs(dy)
    if ax >= ay:
        return [(x0 + sx * k, y0 + sy * ((ax // 2 + k * ay) // ax if ax else 0)) for k in range(ax + 1)]
    return [(x0 + sx * ((ay // 2 + k * ax) // ay), y0 + sy * k) for k in range(ay + 1)]


class Check:
    """isTrajectoryFeasible of the bands of one case. case: dict(bands [(x, y, th)], grid: Grid, fp [(x, y)], r, ang, look, dist,
    rungs: set of kinds)."""

    def __init__(self, case, mode="both", mut=None, grid=None):
        assert mode in ("both", "float") and (mut is None or mut in MUTATIONS)
        self.c, self.hp, self.mut = case, mode == "both", mut
        self.g = case["grid"] if grid is None else grid
        self.rungs = set(case.get("rungs", ()))
        self.records = []
        self.events = collections.Counter()

    # ---- numbers
    def num(self, x):
        return Dual(float(x)) if self.hp else float(x)

    def div(self, a, b):
        return a / b if self.hp else _fdiv(a, b)

    def sqrt(self, x):
        if not self.hp:
            return math.sqrt(x) if x >= 0 else math.nan
        if mpmath.isnan(x.m):
            return Dual(math.nan, mpmath.nan, mpmath.nan)
        return Dual(math.sqrt(x.f), mpmath.sqrt(x.m), mpmath.sqrt(x.s))

    def fabs(self, x):
        return Dual(abs(x.f), abs(x.m), x.s) if self.hp else abs(x)

    def libm(self, name, a):
        if not self.hp:
            return getattr(math, name)(a) if a == a else math.nan
        if a.f != a.f:
            return Dual(math.nan, mpmath.nan, mpmath.nan)
        m = getattr(mpmath, name)(a.m)
        return Dual(getattr(math, name)(a.f), m, max(abs(m), mpf(1)))

    def hypot(self, a, b):
        if self.mut == "look_sqrt":
            return self.sqrt(a * a + b * b)
        if not self.hp:
            return math.hypot(a, b)
        if a.f != a.f or b.f != b.f:
            return Dual(math.nan, mpmath.nan, mpmath.nan)
        return Dual(math.hypot(a.f, b.f), mpmath.sqrt(a.m * a.m + b.m * b.m), mpmath.sqrt(a.s * a.s + b.s * b.s))

    def _classify(self, kind, rel, exact, agree, what):
        if rel >= REL:
            if not agree:
                raise InadmissibleError("%s: separated by %.3g and fp64 decides differently (%s)" % (kind, rel, what))
            return SEPARATED
        if exact:
            assert agree
            return EXACT
        if kind in self.rungs and kind not in LIBM_KINDS:
            return RUNG
        raise InadmissibleError("%s: relative margin %.3g < %g, operands not exact in fp64, no rung declared (%s)" % (kind, rel, REL, what))

    # ---- the recorded comparison
    def cmp(self, kind, a, op, b):
        af, bf = _f(a), _f(b)
        rf = _OPS[op](af, bf)
        if not self.hp:
            return rf
        a, b = _dual(a), _dual(b)
        if af != af or bf != bf:
            if not (mpmath.isnan(a.m) or mpmath.isnan(b.m)):
                raise InadmissibleError("%s: NaN in fp64 only" % kind)
            self.records.append((KIND_ID[kind], EXACT, 0.0, False, False, 0))
            return False
        scale = max(a.s, b.s)
        rel = float(abs(a.m - b.m) / scale) if scale != 0 else (0.0 if a.m == b.m else math.inf)
        cls = self._classify(kind, rel, mpf(af) == a.m and mpf(bf) == b.m, rf == _OPS[op](a.m, b.m), "%r %s %r" % (af, op, bf))
        self.records.append((KIND_ID[kind], cls, rel, bool(rf), af == bf, (af > bf) - (af < bf)))
        return rf

    def to_int(self, kind, q, fn):
        """fn (int: the truncating cast, math.floor, math.ceil) of q, recorded as the distance of q from the nearest integer. Returns the
        fp64 outcome (an int; INT_MIN where x86's cast gives it)."""
        f = _f(q)
        if f != f or abs(f) >= 2.0 ** 31:
            if self.hp:
                if f == f and (self.hp and float(abs(_dual(q).m)) < 2.0 ** 31):
                    raise InadmissibleError("%s: beyond the int range in fp64 only" % kind)
                self.records.append((KIND_ID[kind], EXACT, 0.0, False, False, 0))
            return INT_MIN
        r = int(fn(f))
        if self.hp:
            m, s = q.m, (q.s if q.s != 0 else mpf(1))
            rel = float(abs(m - mpmath.nint(m)) / max(s, mpf(1)))
            rm = int({int: lambda v: v, math.floor: mpmath.floor, math.ceil: mpmath.ceil}[fn](m))   # exactly, not through a float
            cls = self._classify(kind, rel, mpf(f) == m, r == rm, "%r, exactly %s" % (f, mpmath.nstr(m, 25)))
            self.records.append((KIND_ID[kind], cls, rel, cls == RUNG and r != rm, f == math.floor(f), (mpf(f) > m) - (mpf(f) < m)))
        return r

    def int_cmp(self, kind, a, b, outcome):
        if self.hp:
            self.records.append((KIND_ID[kind], EXACT, 0.0 if a == b else abs(a - b) / max(abs(a), abs(b)), bool(outcome), a == b, (a > b) - (a < b)))
        return outcome

    # ---- g2o::normalize_theta
    def normalize_theta(self, theta):
        pi = math.pi
        lo, hi = self.cmp("norm_lo", theta, ">=", -pi), self.cmp("norm_hi", theta, "<", pi)
        if lo and hi:
            return theta
        if _f(theta) != _f(theta):
            return theta
        multiplier = self.to_int("norm_floor", self.div(theta, 2 * pi), math.floor)
        theta = theta - self.num(multiplier) * 2 * pi
        if self.cmp("fix_hi", theta, ">=", pi):
            theta = theta - 2 * pi
        if self.cmp("fix_lo", theta, "<", -pi):
            theta = theta + 2 * pi
        return theta

    # ---- costmap_2d::Costmap2D::worldToMap
    def world_to_map(self, wx, wy):
        g = self.g
        if self.mut != "no_guard":
            bx, by = self.cmp("w_lt_o", wx, "<", g.ox), self.cmp("w_lt_o", wy, "<", g.oy)
            if bx or by:
                return None
        cast = math.floor if self.mut == "w2m_floor" else int
        if self.mut == "w2m_recip":
            inv = self.div(self.num(1.0), self.num(g.res))
            mx, my = self.to_int("trunc", (wx - g.ox) * inv, cast), self.to_int("trunc", (wy - g.oy) * inv, cast)
        else:
            mx, my = self.to_int("trunc", self.div(wx - g.ox, self.num(g.res)), cast), self.to_int("trunc", self.div(wy - g.oy, self.num(g.res)), cast)
        if self.mut == "mx_le_sx":
            ok = 0 <= mx <= g.sx and 0 <= my <= g.sy
        else:   # the unsigned comparison: a negative index is a huge one
            okx, oky = self.int_cmp("idx", mx, g.sx, 0 <= mx < g.sx), self.int_cmp("idx", my, g.sy, 0 <= my < g.sy)
            ok = okx and oky
        return (mx, my) if ok else None

    def cell(self, x, y):
        k = y * self.g.sx + x
        return int(self.g.flat[k]) if k < len(self.g.flat) else 0   # only the mx <= sx mutation can ask beyond the grid

    # ---- WorldModel::footprintCost -> CostmapModel::footprintCost
    def footprint_cost(self, x, y, theta):
        fp = self.c["fp"]
        nf = len(fp)
        c = self.world_to_map(x, y)
        if c is None:
            return self._code(-3, ())
        if nf < 3:
            cost = self.cell(*c)
            return self._code(-2 if cost == 255 else -1 if cost in (254, 253) else cost, ())
        cos_th, sin_th = self.libm("cos", theta), self.libm("sin", theta)
        V = [(x + (self.num(px) * cos_th - self.num(py) * sin_th), y + (self.num(px) * sin_th + self.num(py) * cos_th)) for px, py in fp]
        seen = []   # (edge, code) of every vertex off the map and every cell read, in order, as if nothing returned early
        for i in range(nf - 1 if self.mut == "no_closing" else nf):
            j = i + 1 if i + 1 < nf else 0
            a, b = self.world_to_map(*V[i]), self.world_to_map(*V[j])
            if a is None or b is None:
                seen.append((i, -3))
                continue
            for cx, cy in line_cells(a[0], b[0], a[1], b[1], self.mut, self.events):
                cost = self.cell(cx, cy)
                seen.append((i, -2 if cost == 255 else -1 if cost == 254 or (cost == 253 and self.mut == "253_lethal") else cost))
        neg = [k for k, (_, code) in enumerate(seen) if code < 0]
        if not neg:
            return self._code(max(code for _, code in seen), ())
        if self.mut == "later_lethal" and any(code == -1 for _, code in seen):
            return -1
        e0, c0 = seen[neg[0]]
        return self._code(c0, {(c0, code, "same_edge" if e == e0 else "later_edge") for e, code in (seen[k] for k in neg[1:])})

    def _code(self, code, behind):
        self.events["code:%d" % min(code, 0)] += 1
        for first, later, where in behind:
            if later != first:
                self.events["behind:%d_hides_%d_%s" % (first, later, where)] += 1
        return code

    def collides(self, x, y, theta):
        code = self.footprint_cost(x, y, theta)
        return code == -1 or (code == -2 and self.mut == "255_collision") or (code == -3 and self.mut == "offmap_collision")

    # ---- isTrajectoryFeasible
    def look_ahead(self, x, y):
        n, c = len(x), self.c
        look = c["look"]
        if look < 0 or look >= n:
            look = n - 1
        if c["dist"] > 0:
            for i in range(1, n):
                d = self.hypot(self.num(x[i]) - self.num(x[0]), self.num(y[i]) - self.num(y[0]))
                if self.cmp("look", d, ">", c["dist"]):
                    look = min(look, i - 1) if self.mut == "look_no_override" else i - 1
                    break
        return look

    def tests(self, b):
        """(index in the reference's order, pose) of every footprint test, one after the other"""
        x, y, th = self.c["bands"][b]
        c = self.c
        look = self.look_ahead(x, y)
        self.look = look
        q = 0
        carried = None
        for i in range(look + 1):
            own = (self.num(x[i]), self.num(y[i]), self.num(th[i]))
            yield q, (carried if self.mut == "bsearch_off" and carried is not None else own)
            q += 1
            if i == look:
                break
            delta_rot = self.normalize_theta(self.normalize_theta(self.num(th[i + 1])) - self.normalize_theta(self.num(th[i])))
            ddx, ddy = self.num(x[i + 1]) - self.num(x[i]), self.num(y[i + 1]) - self.num(y[i])
            dnorm = self.sqrt(ddx * ddx + ddy * ddy)
            arot = self.fabs(delta_rot)
            t_rot = self.cmp("rot", arot, ">=" if self.mut == "rot_ge" else ">", c["ang"])
            t_dist = self.cmp("dist", dnorm, ">=" if self.mut == "dist_ge" else ">", c["r"])
            nadd = 0
            if t_rot or t_dist:
                a = self.to_int("ceil_rot", self.div(arot, self.num(c["ang"])), math.ceil)
                d = self.to_int("ceil_dist", self.div(dnorm, self.num(c["r"])), math.ceil)
                if a == INT_MIN:        # std::max(NaN, d) is NaN, and (int)(NaN - 1) is INT_MIN on x86: no sample
                    nadd = INT_MIN
                else:
                    nadd = (d if self.int_cmp("max", a, d, a < d) else a) - 1
                self.events["max:%s" % ("rot" if a > d else "dist" if d > a else "equal")] += 1
            self.events["nadd:%d" % max(nadd, 0)] += 1
            px, py, pth = own
            div = self.num(nadd + 1.0)
            for step in range(nadd):
                if self.mut == "closed_form":
                    px, py = own[0] + (step + 1) * self.div(ddx, div), own[1] + (step + 1) * self.div(ddy, div)
                else:
                    px, py = px + self.div(ddx, div), py + self.div(ddy, div)
                pth = self.normalize_theta(pth + self.div(delta_rot, div))
                yield q, (px, py, pth)
                q += 1
            if self.mut == "bsearch_off":   # one more step of this segment's recurrence stands in for the next pose
                d1 = self.num(max(nadd, 0) + 1.0)
                carried = (px + self.div(ddx, d1), py + self.div(ddy, d1), self.normalize_theta(pth + self.div(delta_rot, d1)))

    def run(self, b=0):
        """(feasible, first_infeasible) of band b"""
        if self.hp:
            with mpmath.workdps(DPS):
                return self._run(b)
        return self._run(b)

    def _run(self, b):
        if self.mut == "lane_min":   # every lane stops at its first collision; the lowest LANE answers
            hits = [q for q, p in self.tests(b) if self.collides(*p)]
            return (False, min(hits, key=lambda q: (q % LANES, q))) if hits else (True, -1)
        for q, p in self.tests(b):
            if self.collides(*p):
                return False, q
        return True, -1

    def record_array(self):
        return np.array(self.records, np.float64).reshape(-1, 6)


def summary(rec):
    """[len(KINDS), 8] float64 per kind: comparisons, exact ones, ties in fp64, rungs with the fp64 value above / not above the exact one,
    separated with outcome true / false, the smallest separated margin (inf: none)"""
    out = np.zeros((len(KINDS), 8))
    out[:, 7] = np.inf
    for k in range(len(KINDS)):
        r = rec[rec[:, 0] == k]
        sep = r[r[:, 1] == SEPARATED]
        out[k, :7] = [len(r), (r[:, 1] == EXACT).sum(), r[:, 4].sum(), ((r[:, 1] == RUNG) & (r[:, 5] > 0)).sum(), ((r[:, 1] == RUNG) & (r[:, 5] <= 0)).sum(),
                      (sep[:, 3] == 1).sum(), (sep[:, 3] == 0).sum()]
        if len(sep):
            out[k, 7] = sep[:, 2].min()
    return out


# ---- the fixture layout: per family one array per field, the cases one after the other -------------------------------------------------------
def pack(records):
    names = list(records)
    out = {"names": np.array(names)}
    for f in records[names[0]]:
        parts = [np.ascontiguousarray(records[n][f]).ravel() for n in names]
        out[f] = np.concatenate(parts)
        out[f + "_off"] = np.cumsum([0] + [len(q) for q in parts]).astype(np.int64)
    return out


def unpack(npz):
    """{case name: {field: array}}; bands come back as a list of (x, y, th), the grid as [sy, sx]"""
    names = [str(n) for n in npz["names"]]
    fields = [f[:-4] for f in npz.files if f.endswith("_off")]
    out = {}
    for k, n in enumerate(names):
        d = {f: npz[f][npz[f + "_off"][k]:npz[f + "_off"][k + 1]] for f in fields}
        sx, sy = int(d["grid"][0]), int(d["grid"][1])
        d["cells"] = d["cells"].reshape(sy, sx)
        off = np.concatenate([[0], np.cumsum(d["band_n"])])
        d["bands"] = [tuple(d["poses"].reshape(-1, 3)[off[b]:off[b + 1], j].copy() for j in range(3)) for b in range(len(d["band_n"]))]
        d["fp"] = d["fp"].reshape(-1, 2)
        d["expected"] = d["expected"].reshape(-1, 2)
        out[n] = d
    return out
