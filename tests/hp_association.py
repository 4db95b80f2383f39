"""Exact reference of the DECISIONS of the graph build: which pose carries which obstacle / via-point edge. NOT a test file.

tests/hp_linearize.py pins the arithmetic of every edge and takes the edge list as given; this module pins the list. It restates
AddEdgesObstacles of the reference planner (src/optimal_planner.cpp:444-548) over mpmath at 80 digits on top of the distance functions
of hp_linearize (_footprint_distance and below - there is no second set):
  poses first_vertex .. n - 2 (first_vertex = 0 if weight_velocity_obstacle_ratio != 0 else 1), dynamic obstacles left out when
  include_dynamic_obstacles is set; dist < min_obstacle_dist * force_factor: forced, in table order; dist > min_obstacle_dist *
  cutoff_factor: dropped; else the side is cross2d(orientationUnitVec, centroid - position) > 0 (left) and a strict '<' keeps the FIRST
  minimum per side; left is appended before right;
the via-point attachment (AddEdgesViaPoints :675-718 with findClosestTrajectoryPose, src/timed_elastic_band.cpp:455-478: strict '<' on
the squared distance from start_pose_idx, index > n - 2 -> n - 2, index < 1 -> 1 when ordered, no edge otherwise) and the legacy rule
(AddEdgesObstaclesLegacy :551-643: the closest pose of every obstacle, n / 2 for all when obstacle_poses_affected >= n, skipped unless
1 < index <= n - 2, one edge at index and then edges at index +- nb for nb = 0 .. floor(poses_affected / 2) - 1).

Admissibility. EVERY comparison the rule makes is recorded with its relative margin |a - b| / max(|a|, |b|) (the cross product against
0: relative to |ox vy| + |vx oy|): each dist against force and against cutoff, the cross product against 0, each dist against the
running minimum of its side, each arg-min winner against every other candidate. A comparison is admissible if it is
  well separated: relative margin >= REL = 1e-9 (1e7 x fp64 rounding: any fp64 evaluation decides alike), or
  exact:          both operands evaluated with every operation rounded to 53 bits (mpmath at prec = 53: round to nearest even, what
                  fp64 does) EQUAL their 80-digit values - then an fp64 implementation holds the very same two numbers and the
                  comparison may be a tie or one ulp off.
Anything else raises InadmissibleError. No decision and no case is ever dropped.
"""
import numpy as np

import hp_linearize as hp

try:
    import mpmath
    from mpmath import mpf
except ImportError:   # same_lists() and the mutations are all the GPU test uses
    mpmath, mpf = None, None

DPS = hp.DPS
REL = 1e-9


class InadmissibleError(ValueError):
    pass


class Reference:
    """one band of one scene; associate() / via_points() / legacy() fill self.records:
    (what, pose, obstacle or via-point, relative margin, exact: True / None (not needed), outcome of a < b, a == b)"""

    def __init__(self, cfg, obst, via, batch, b=0):
        self.cfg, self.obst_table, self.via = cfg, obst, [(float(v[0]), float(v[1])) for v in via]
        with mpmath.workdps(DPS):
            self.P = hp._Params(cfg, 1.0)
            self.ob = [hp._Obstacle(obst, k) for k in range(len(obst))]
        self.n = n = int(batch.n[b])
        self.X = [(float(batch.x[b, i]), float(batch.y[b, i]), float(batch.theta[b, i])) for i in range(n)]
        o = cfg.obstacles
        self.force_factor, self.cutoff_factor = float(o.obstacle_association_force_inclusion_factor), float(o.obstacle_association_cutoff_factor)
        self.static = [k for k in range(len(obst)) if not (o.include_dynamic_obstacles and obst.dynamic[k])]
        self.cx = hp._Ctx(False)
        self.cx.on = False
        self.cache, self.records = {}, []

    # ---- operands: a token names an expression, evaluated at 80 digits or with every operation rounded to 53 bits
    def _centroid(self, k):
        ob = self.ob[k]
        if ob.type in (hp.OB_POINT, hp.OB_CIRCULAR):
            return ob.a
        if ob.type in (hp.OB_LINE, hp.OB_PILL):
            return (mpf(0.5) * (ob.a[0] + ob.b[0]), mpf(0.5) * (ob.a[1] + ob.b[1]))
        V = ob.verts   # PolygonObstacle::calcCentroid, src/obstacles.cpp:56-121
        m = len(V)
        if m == 1:
            return V[0]
        if m == 2:
            return (mpf(0.5) * (V[0][0] + V[1][0]), mpf(0.5) * (V[0][1] + V[1][1]))
        A = mpf(0)
        for i in range(m - 1):
            A += V[i][0] * V[i + 1][1] - V[i + 1][0] * V[i][1]
        A += V[m - 1][0] * V[0][1] - V[0][0] * V[m - 1][1]
        A *= mpf(0.5)
        assert A != 0, "degenerate polygon: not restated here"
        c = [mpf(0), mpf(0)]
        for i in range(m):
            p, q = V[i], V[(i + 1) % m]
            aux = p[0] * q[1] - q[0] * p[1]
            c[0] += aux * (p[0] + q[0]); c[1] += aux * (p[1] + q[1])
        return (c[0] / (6 * A), c[1] / (6 * A))

    def _eval(self, tok):
        kind = tok[0]
        P = self.P
        if kind == "force":
            return P.min_obstacle_dist * mpf(self.force_factor)
        if kind == "cutoff":
            return P.min_obstacle_dist * mpf(self.cutoff_factor)
        if kind == "zero":
            return mpf(0)
        x, y, th = (mpf(v) for v in self.X[tok[1]])
        if kind == "dist":
            return hp._footprint_distance(self.cx, P, x, y, th, self.ob[tok[2]], None)
        if kind in ("cross", "cross_scale"):   # cross2d(a, b) = a.x b.y - b.x a.y (misc.h:119-123)
            c = self._centroid(tok[2])
            ox, oy, vx, vy = mpmath.cos(th), mpmath.sin(th), c[0] - x, c[1] - y
            return ox * vy - vx * oy if kind == "cross" else abs(ox * vy) + abs(vx * oy)
        if kind == "sq":   # squared distance of pose tok[1] to the point (tok[2], tok[3])
            dx, dy = mpf(tok[2]) - x, mpf(tok[3]) - y
            return dx * dx + dy * dy
        if kind == "sqc":   # ... to the centroid of obstacle tok[2]
            c = self._centroid(tok[2])
            dx, dy = c[0] - x, c[1] - y
            return dx * dx + dy * dy
        if kind == "shape":   # findClosestTrajectoryPose(obstacle): the distance of the pose's position to the line / polygon
            ob = self.ob[tok[2]]
            return hp._pt_seg((x, y), ob.a, ob.b)[0] if ob.type == hp.OB_LINE else hp._pt_poly((x, y), ob.verts)[0]
        raise KeyError(tok)

    def value(self, tok, fp64=False):
        key = (tok, fp64)
        if key not in self.cache:
            with (mpmath.workprec(53) if fp64 else mpmath.workdps(DPS)):
                self.cache[key] = self._eval(tok)
        return self.cache[key]

    def compare(self, what, pose, item, ta, tb, scale=None):
        """records a against b, returns (a < b, a == b) taken at 80 digits"""
        with mpmath.workdps(DPS):
            a, b = self.value(ta), self.value(tb)
            s = max(abs(a), abs(b)) if scale is None else self.value(scale)
            rel = float(abs(a - b) / s) if s != 0 else (0.0 if a == b else float("inf"))
        exact = None
        if rel < REL:
            exact = self.value(ta, True) == a and self.value(tb, True) == b
            if not exact:
                raise InadmissibleError("%s, pose %d, item %d: relative margin %.3g < %g and the operands are not exact in fp64 (%s, %s)"
                                        % (what, pose, item, rel, REL, mpmath.nstr(a, 25), mpmath.nstr(b, 25)))
        self.records.append((what, pose, item, rel, exact, bool(a < b), bool(a == b)))
        return a < b, a == b

    # ---- AddEdgesObstacles
    def associate(self):
        """dict(assoc_pose, assoc_obst: the lists as oracle.associate gives them (pose 0 and n - 1 carry no edge), forced {pose: [k]},
        left / right {pose: k}, ties [(pose, kept k, rejected k)]: equal distances on one side, decided by table order)"""
        n = self.n
        first = 0 if float(self.cfg.optim.weight_velocity_obstacle_ratio) != 0 else 1
        ap, ao, forced, left, right, ties = [], [], {}, {}, {}, []
        for i in range(first, n - 1):
            fl, best = [], {True: None, False: None}
            for k in self.static:
                if self.compare("dist < force", i, k, ("dist", i, k), ("force",))[0]:
                    fl.append(k)
                    continue
                lt, eq = self.compare("dist > cutoff", i, k, ("dist", i, k), ("cutoff",))
                if not lt and not eq:
                    continue
                lt, eq = self.compare("cross > 0", i, k, ("cross", i, k), ("zero",), ("cross_scale", i, k))
                on_left = not lt and not eq
                if best[on_left] is None:
                    best[on_left] = k
                    continue
                lt, eq = self.compare("dist < side minimum", i, k, ("dist", i, k), ("dist", i, best[on_left]))
                if eq:
                    ties.append((i, best[on_left], k))
                if lt:
                    best[on_left] = k
            forced[i], left[i], right[i] = fl, best[True], best[False]
            if i == 0:
                continue
            lst = fl + [k for k in (best[True], best[False]) if k is not None]
            ap += [i] * len(lst); ao += lst
        return dict(assoc_pose=np.array(ap, np.int32), assoc_obst=np.array(ao, np.int32), forced=forced, left=left, right=right, ties=ties)

    # ---- arg-min with strict '<': the first minimum
    def _argmin(self, what, item, toks, poses):
        win = 0
        for q in range(1, len(toks)):
            with mpmath.workdps(DPS):
                if self.value(toks[q]) < self.value(toks[win]):
                    win = q
        for q in range(len(toks)):
            if q != win:
                self.compare(what, poses[q], item, toks[win], toks[q])
        return poses[win]

    def _closest_pose_point(self, what, item, tok, begin):
        if begin < 0 or begin >= self.n:
            return -1
        poses = list(range(begin, self.n))
        return self._argmin(what, item, [tok(i) for i in poses], poses)

    def via_points(self):
        """pose index per via-point, -1: no edge"""
        n, ordered = self.n, bool(self.cfg.trajectory.via_points_ordered)
        out, start = [], 0
        for v, p in enumerate(self.via):
            index = self._closest_pose_point("via-point arg-min", v, lambda i: ("sq", i, p[0], p[1]), start)
            if ordered:
                start = index + 2
            if index > n - 2:
                index = n - 2
            if index < 1:
                index = 1 if ordered else -1
            out.append(index)
        return np.array(out, np.int32)

    def legacy(self):
        """(assoc_pose, assoc_obst) in the order of oracle.associate: obstacle-major, the edge at index, then index + nb, index - nb"""
        n, pa = self.n, int(self.cfg.obstacles.obstacle_poses_affected)
        ap, ao, closest = [], [], {}

        def add(i, k):
            if 0 < i < n - 1:   # an edge whose only vertex is fixed is never activated
                ap.append(i); ao.append(k)
        for k in self.static:
            ob = self.ob[k]
            if pa >= n:
                index = n // 2
            elif ob.type == hp.OB_LINE or (ob.type == hp.OB_POLYGON and len(ob.verts) >= 2):
                poses = list(range(n))
                index = self._argmin("legacy arg-min", k, [("shape", i, k) for i in poses], poses)
            else:
                index = self._closest_pose_point("legacy arg-min", k, lambda i: ("sqc", i, k), 0)
            closest[k] = index
            if index <= 1 or index > n - 2:
                continue
            add(index, k)
            for nb in range(pa // 2):
                if index + nb < n:
                    add(index + nb, k)
                if index - nb >= 0:
                    add(index - nb, k)
        return np.array(ap, np.int32), np.array(ao, np.int32), closest

    def summary(self):
        """(comparisons, exact ones, ties among them, smallest relative margin of the well separated ones)"""
        ex = [r for r in self.records if r[4]]
        sep = [r[3] for r in self.records if not r[4]]
        return len(self.records), len(ex), sum(r[6] for r in ex), min(sep) if sep else float("inf")


# ---- the comparison the GPU test uses, and the mutations it must reject (no mpmath needed) -------------------------------------------
def canonical(pose, obst, legacy=False):
    """The new association compares the lists as they are (pose-major, within a pose: forced in table order, left, right). The legacy
    lists are a multiset per pose (the reference adds them obstacle by obstacle, the device collects them pose by pose): sorted by
    (pose, obstacle)."""
    pose, obst = np.asarray(pose, np.int64), np.asarray(obst, np.int64)
    if legacy:
        order = np.lexsort((obst, pose))
        pose, obst = pose[order], obst[order]
    return pose, obst


def same_lists(pose, obst, want_pose, want_obst, legacy=False):
    a, b = canonical(pose, obst, legacy), canonical(want_pose, want_obst, legacy)
    return a[0].shape == b[0].shape and bool((a[0] == b[0]).all()) and bool((a[1] == b[1]).all())


def mutate_swap_within_pose(pose, obst, i, a, b):
    """entries a and b of pose i's list swapped (a tie resolved the other way, a forced entry moved behind left / right)"""
    obst = np.array(obst)
    at = np.flatnonzero(np.asarray(pose) == i)
    obst[at[a]], obst[at[b]] = obst[at[b]], obst[at[a]]
    return np.array(pose), obst


def mutate_replace(pose, obst, i, old, new):
    obst = np.array(obst)
    at = [q for q in np.flatnonzero(np.asarray(pose) == i) if obst[q] == old]
    assert at
    obst[at[0]] = new
    return np.array(pose), obst


def mutate_drop(pose, obst, i, k):
    pose, obst = np.asarray(pose), np.asarray(obst)
    at = [q for q in np.flatnonzero(pose == i) if obst[q] == k]
    assert at
    keep = np.ones(len(pose), bool)
    keep[at[0]] = False
    return pose[keep], obst[keep]


def mutate_reverse_chunk(obst_positions, M, chunk=32):
    """what a bit order reversed within one chunk of 32 list positions does to a list of positions: p -> the mirrored position of its
    chunk (the last chunk mirrors within its own length)"""
    out = []
    for p in obst_positions:
        lo = (int(p) // chunk) * chunk
        hi = min(lo + chunk, M)
        out.append(lo + (hi - 1 - int(p)))
    return np.array(out, np.int32)
