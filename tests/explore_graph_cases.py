"""The smallest scenes on which the exploration graph (createGraph: graph_vertices on the host, graph_edges_kernel /
graph_edges_fleet_kernel on the device) can still go wrong. NOT a test file; shared by tests/golden/make_hp_explore_graph.py and
tests/test_hp_explore_graph.py. The GPU test reads the fixtures only.

Coordinates are dyadic and start -> goal runs along an axis wherever the decision under test allows it, so that cross products and many
norms are exact in fp64; where a quantity cannot be exact (a 3-4-5 direction, sqrt(0.3125), the samples of the roadmap) the threshold is
put ON its fp64 evaluation and a ladder about it (tie, +-1 / +-4 ulp, relative +-2^-41, +-2^-36): rounded rungs in the sense of
tests/hp_explore_graph.py. Where the threshold is fixed (0.1 of "in front of the start") the obstacle moves instead.

Families (the first word of a case name; one fixture file each):
  fwd    dot <= thr of the forward test: perpendicular ties at thr = 0, the 3-4-5 ladder (key points), a ladder on a roadmap pair,
         coincident vertices at thr = 0 and thr < 0 (the zero-length edge reaches the obstacle test)
  head   the start-heading test on the nearest obstacle's key points: ladder, thr = 0, nothing in front, bit-equal distances, nearest second
  front  (start2obst . diff) / dist < 0.1 on the host: ladder, obstacle on the start (NaN), abeam, behind
  disc   point and circular obstacles against min_dist: t < 0, t > 1, t = 0, t = 1, interior; 0.5 * dist_to_obst and dist_to_obst; radius
  seg    line, pill and polygon obstacles: crossing, the four T-junctions, shared end point, parallel, collinear, all orientations,
         crossings missed and made by a few ulp, closing edges, polygons of 1 and 2 vertices
  lanes  N = 2, 8, 9, 16, 17, 23 (N^2 = 529 > 2 * kThreads); the deciding pair at idx 63 / 64 / 255 / 256 / the last pair with an edge
         (idx N^2 - 1 is goal -> goal: never an edge); a wave without a heading survivor beside one with a single lane
  table  1, 63, 64, 65, 130 obstacles of all types, the deciding one first, in the middle, last; hit and tie
  fleet  the members of two launches (FLEETS): key-point graphs of N = 2 (M = 0), N = 18, M = 130 and a scene at its goal; roadmaps of
         N = 17 over one set of samples against three different tables and a scene at its goal
"""
import math

import numpy as np

import hp_explore_graph as HG
from teb_local_planner_amd import _abi
from teb_local_planner_amd.config import TebConfig

K_THREADS = 256   # csrc/teb_device.hpp, read back by the CPU test
FAMILIES = ["fwd", "head", "front", "disc", "seg", "lanes", "table", "fleet"]
LADDER = ["0", "+1ulp", "-1ulp", "+4ulp", "-4ulp", "+2^-41", "-2^-41", "+2^-36", "-2^-36"]
SHORT = ["0", "+1ulp", "-1ulp"]
_BUILDERS, _BUILT = {}, {}
CASES = []
FLEETS = {"fleetk": ["fleet_k_empty", "fleet_k_n18", "fleet_k_m130", "fleet_k_atgoal"],
          "fleetr": ["fleet_r_block", "fleet_r_empty", "fleet_r_other", "fleet_r_atgoal"]}


def rung(x, label):
    """x on the rung `label` of the ladder"""
    if label == "0":
        return x
    if label.endswith("ulp"):
        return HG.ulps(x, int(label[:-3]))
    return x * (1.0 + math.copysign(2.0 ** int(label[3:]), float(label[0] + "1")))


def _reg(name, fn):
    assert name not in _BUILDERS and name.split("_")[0] in FAMILIES, name
    _BUILDERS[name] = fn
    CASES.append(name)


def build(name):
    """the case, built once and left unchanged"""
    if name not in _BUILT:
        c = _BUILDERS[name]()
        c["name"], c["family"] = name, name.split("_")[0]
        _BUILT[name] = c
    return _BUILT[name]


def table(rows):
    """rows: ('p', x, y) | ('c', x, y, r) | ('l', x1, y1, x2, y2) | ('i', x1, y1, x2, y2, r) | ('g', [(x, y), ...])"""
    ob = _abi.ObstacleTable()
    for r in rows:
        if r[0] == "p":
            ob.add_point(r[1], r[2])
        elif r[0] == "c":
            ob.add_circle(r[1], r[2], r[3])
        elif r[0] == "l":
            ob.add_line(*r[1:5])
        elif r[0] == "i":
            ob.add_pill(*r[1:6])
        else:
            ob._add(_abi.OBST_POLYGON, verts=[tuple(map(float, v)) for v in r[1]])   # taken as given, no closure fix
    return ob


def case(rows, keypoint=True, start=(0.0, 0.0, 0.0), goal=(8.0, 0.0, 0.0), dist_to_obst=0.5, thr=0.0, no_samples=0, area_width=4.0,
         length_scale=1.0, rungs=(), max_classes=1, max_paths=8, xy_goal_tolerance=0.2):
    return dict(rows=list(rows), obst=table(rows), keypoint=bool(keypoint), start=[float(v) for v in start], goal=[float(v) for v in goal],
                dist_to_obst=float(dist_to_obst), thr=float(thr), no_samples=int(no_samples), area_width=float(area_width),
                length_scale=float(length_scale), rungs=sorted(rungs), max_classes=int(max_classes), max_paths=int(max_paths),
                xy_goal_tolerance=float(xy_goal_tolerance))


def config(c, max_classes=None):
    cfg = TebConfig()
    h = cfg.hcp
    h.simple_exploration = c["keypoint"]
    h.obstacle_heading_threshold = c["thr"]
    h.roadmap_graph_no_samples = c["no_samples"]
    h.roadmap_graph_area_width = c["area_width"]
    h.roadmap_graph_area_length_scale = c["length_scale"]
    h.max_number_classes = c["max_classes"] if max_classes is None else max_classes
    cfg.goal_tolerance.xy_goal_tolerance = c["xy_goal_tolerance"]
    return cfg


def probe(c):
    """(result, probe) of the op-by-op fp64 restatement"""
    g = HG.Graph(c, "float")
    return g.run(), g.probe


def _with(c, **kw):
    d = dict(c)
    d.update(kw)
    if "rows" in kw:
        d["obst"] = table(kw["rows"])
    d["rungs"] = sorted(kw.get("rungs", c["rungs"]))
    return d


# ---- fwd ----------------------------------------------------------------------------------------------------------------------------------
_FWD_ROWS = [("p", 2.0, -1.0), ("p", 5.0, 3.0)]   # key points 1 = (2, -0.5), 2 = (2, -1.5), 3 = (5, 3.5), 4 = (5, 2.5): 1 -> 3 and 2 -> 4 are (3, 4)
# key points 1 = (4, 2.5) and 4 = (4, 2.75): perpendicular to start -> goal, 0.5 from either obstacle - only the tie 0 <= 0 removes 1 <-> 4
_reg("fwd_perpendicular_thr0", lambda: case([("p", 4.0, 2.0), ("p", 4.0, 3.25)]))


def _fwd_345(label):
    base = case(_FWD_ROWS, thr=0.25)
    d = probe(base)[1][("fwd", 1, 3)]
    assert d == 3.0 / 5.0 and probe(base)[1][("fwd", 2, 4)] == d
    return _with(base, thr=rung(d, label), rungs=["fwd"])


def _roadmap_rows():
    return [("p", 4.0, 1.0), ("c", 2.0, -1.5, 0.25)]


def _fwd_roadmap(label):
    base = case(_roadmap_rows(), keypoint=False, no_samples=6, thr=0.25)
    pr = probe(base)[1]
    (i, j), d = min(((k[1:], v) for k, v in pr.items() if k[0] == "fwd" and 0.3 < v < 0.7), key=lambda kv: abs(kv[1] - 0.5))
    return _with(base, thr=rung(d, label), rungs=["fwd"], pair=(i, j))


for _l in LADDER:
    _reg("fwd_345_" + _l, lambda _l=_l: _fwd_345(_l))
    _reg("fwd_roadmap_" + _l, lambda _l=_l: _fwd_roadmap(_l))
# two obstacles with one centroid (key points 1 = 3, 2 = 4) and a key point on the goal (5 = goal = 7)
_COINCIDENT = [("p", 4.0, 2.0), ("c", 4.0, 2.0, 0.125), ("p", 8.0, -0.5)]
_reg("fwd_coincident_thr0", lambda: case(_COINCIDENT))
_reg("fwd_coincident_negative", lambda: case(_COINCIDENT, thr=-0.5))

# ---- head: start -> goal along +y, start heading along +x: the two tests see different dots ---------------------------------------------
_HEAD = dict(goal=(0.0, 8.0, 0.0))   # normal = (-0.5, 0): key points of (3.5, 4) are 1 = (3, 4) and 2 = (4, 4)


def _head(label):
    base = case([("p", 3.5, 4.0)], thr=0.25, **_HEAD)
    d = probe(base)[1][("head", 1)]
    assert d == 3.0 / 5.0
    return _with(base, thr=rung(d, label), rungs=["head"])


for _l in LADDER:
    _reg("head_345_" + _l, lambda _l=_l: _head(_l))
_reg("head_disabled_thr0", lambda: case([("p", 3.5, 4.0)], start=(0.0, 0.0, math.pi), **_HEAD))
_reg("head_cuts_both_keypoints", lambda: case([("p", 3.5, 4.0)], thr=0.25, start=(0.0, 0.0, math.pi), **_HEAD))   # heading along -x
_reg("head_none_in_front", lambda: case([("p", 1.0, -2.0), ("p", 3.0, 0.0)], thr=0.25, **_HEAD))
_reg("head_equal_distance", lambda: case([("p", 3.5, 4.0), ("p", -3.5, 4.0)], thr=0.25, **_HEAD))
_reg("head_nearest_second", lambda: case([("p", -3.5, 6.0), ("p", 3.5, 4.0)], thr=0.25, **_HEAD))


# ---- front: the threshold is the literal 0.1, the obstacle moves --------------------------------------------------------------------------
def _front_q(ox, oy):
    return ox / math.sqrt(ox * ox + oy * oy)   # diff = (1, 0): ox * 1 + oy * 0 = ox


def _front(label):
    target = rung(0.1, label)
    best = None
    y0 = math.sqrt(99.0)
    for jx in range(-6, 7):
        ox = HG.ulps(1.0, jx)
        for jy in range(-160, 161):
            oy = HG.ulps(y0, jy)
            e = abs(_front_q(ox, oy) - target)
            if best is None or e < best[0]:
                best = (e, ox, oy)
    assert best[0] == 0 or not label.endswith("ulp") and label != "0", (label, best)
    c = case([("p", best[1], best[2])], rungs=["front"])
    assert probe(c)[1][("front", 0)] == _front_q(best[1], best[2])
    return c


for _l in LADDER:
    _reg("front_ladder_" + _l, lambda _l=_l: _front(_l))
_reg("front_on_start", lambda: case([("p", 0.0, 0.0)]))
_reg("front_abeam", lambda: case([("p", 0.0, 3.0)]))
_reg("front_behind", lambda: case([("p", -2.0, 1.0)]))


# ---- disc: one edge (start -> goal, N = 2), one point or circular obstacle -------------------------------------------------------------------
def _disc(rows, keypoint, label):
    base = case(rows, keypoint=keypoint, dist_to_obst=0.125)
    d = probe(base)[1][("dmin", 0, 1, 0)]
    return _with(base, dist_to_obst=rung(d, label) * (2.0 if keypoint else 1.0), rungs=["dmin"])


for _l in LADDER:
    _reg("disc_before_keypoint_" + _l, lambda _l=_l: _disc([("p", -0.25, 0.5)], True, _l))     # t < 0, d = sqrt(0.3125)
    _reg("disc_before_roadmap_" + _l, lambda _l=_l: _disc([("p", -0.25, 0.5)], False, _l))
for _l in SHORT:
    _reg("disc_beyond_roadmap_" + _l, lambda _l=_l: _disc([("p", 8.25, 0.5)], False, _l))       # t > 1
    _reg("disc_start_keypoint_" + _l, lambda _l=_l: _disc([("p", 0.0, 0.75)], True, _l))        # t = 0 exactly, d = 0.75 exactly
    _reg("disc_end_roadmap_" + _l, lambda _l=_l: _disc([("p", 8.0, 0.75)], False, _l))          # t = 1 exactly
    _reg("disc_interior_roadmap_" + _l, lambda _l=_l: _disc([("p", 4.0, 0.75)], False, _l))
    _reg("disc_interior_keypoint_" + _l, lambda _l=_l: _disc([("p", 0.03125, 0.75)], True, _l))
    _reg("disc_circle_roadmap_" + _l, lambda _l=_l: _disc([("c", 4.0, 1.0, 0.25)], False, _l))  # d - radius = 0.75 exactly
_reg("disc_radius_larger_than_distance", lambda: case([("c", 0.0, 0.75, 1.0)]))


def _disc_radius(label):
    d0 = math.sqrt(0.3125)
    return case([("c", -0.25, 0.5, rung(d0 - 0.25, label))], rungs=["dmin"])   # min_dist = 0.25; d0 - r = 0.25 on the tie


for _l in ["0", "+1ulp", "-1ulp", "+4ulp", "-4ulp"]:
    _reg("disc_radius_rung_" + _l, lambda _l=_l: _disc_radius(_l))

# ---- seg: one edge, one line / pill / polygon obstacle ------------------------------------------------------------------------------------
_SEG = dict(cross=(4.0, -1.0, 4.0, 1.0), s0=(4.0, 0.0, 4.0, 1.0), s1=(4.0, -1.0, 4.0, 0.0), t0=(0.0, -1.0, 0.0, 1.0), t1=(8.0, -1.0, 8.0, 1.0),
            shared=(0.0, 0.0, 0.0, 1.0), parallel=(2.0, 1.0, 6.0, 1.0), collinear=(2.0, 0.0, 6.0, 0.0))


def _seg(what, edge_fwd, obst_fwd):
    a = _SEG[what]
    if not obst_fwd:
        a = a[2:] + a[:2]
    row = ("l",) + a if obst_fwd else ("i",) + a + (0.125,)
    se = dict() if edge_fwd else dict(start=(8.0, 0.0, 0.0), goal=(0.0, 0.0, 0.0))
    return case([row], keypoint=False, **se)


for _w in _SEG:
    for _e in (True, False):
        for _o in (True, False):
            _reg("seg_%s_%s%s" % (_w, "e+" if _e else "e-", "o+" if _o else "o-"), lambda _w=_w, _e=_e, _o=_o: _seg(_w, _e, _o))


def _seg_ulp(tag, k):
    a, b = {"pi": (math.pi, math.e), "sqrt": (3.0 * math.sqrt(2.0), math.sqrt(3.0))}[tag]
    sx, sy = a / 2, HG.ulps(b / 2, k)   # the obstacle starts k ulp off the middle of the edge (0, 0) -> (a, b) and leaves to one side
    return case([("l", sx, sy, sx - 1.0, sy + 2.0)], keypoint=False, goal=(a, b, 0.0), rungs=["s_lo"])


for _t in ("pi", "sqrt"):
    for _k in range(-3, 4):
        _reg("seg_ulp_%s_%+d" % (_t, _k), lambda _t=_t, _k=_k: _seg_ulp(_t, _k))


def _seg_parallel_ulp(k):
    """l1 = (1 + 2^-k, 1) against l2 = (1, 1 - 2^-k) through each other's middle: denom = -2^-2k exactly. k = 30: the fp64 product
    rounds to 1 and denom is 0 (parallel, no crossing) where a fused cross product sees a crossing; k = 26: -2^-52 in fp64 too"""
    e = 2.0 ** -k
    return case([("l", e / 2, 0.5 * e, 1.0 + e / 2, 1.0 - 0.5 * e)], keypoint=False, goal=(1.0 + e, 1.0, 0.0), rungs=["denom0"])


_reg("seg_nearly_parallel_2^-30", lambda: _seg_parallel_ulp(30))
_reg("seg_nearly_parallel_2^-26", lambda: _seg_parallel_ulp(26))
_reg("seg_triangle_closing_edge_only", lambda: case([("g", [(6.0, -1.0), (10.0, -1.0), (9.0, 1.0)])], keypoint=False))
_reg("seg_quad_closing_edge_only", lambda: case([("g", [(6.0, -1.0), (10.0, -1.0), (10.0, 1.0), (9.0, 1.0)])], keypoint=False))
_reg("seg_triangle_first_edge", lambda: case([("g", [(4.0, -1.0), (4.0, 1.0), (12.0, 4.0)])], keypoint=False))
_reg("seg_triangle_clear", lambda: case([("g", [(3.0, 1.0), (5.0, 1.0), (4.0, 2.0)])], keypoint=False))
_reg("seg_polygon_one_vertex_on_the_edge", lambda: case([("g", [(4.0, 0.0)])], keypoint=False))
_reg("seg_polygon_two_vertices", lambda: case([("g", [(4.0, -1.0), (4.0, 1.0)])], keypoint=False))
_reg("seg_polygon_two_vertices_clear", lambda: case([("g", [(4.0, 1.0), (4.0, 2.0)])], keypoint=False))
_reg("seg_keypoint_line_and_polygon", lambda: case([("l", 3.0, 0.5, 3.0, 2.5), ("g", [(5.0, -2.0), (6.0, -2.0), (6.0, -1.0), (5.0, -1.0)])], thr=0.25))


# ---- lanes --------------------------------------------------------------------------------------------------------------------------------
def _alternating(n, y=1.5):
    return [("p", 0.75 + 6.5 * k / max(n - 1, 1), y if k % 2 == 0 else -y) for k in range(n)]


_reg("lanes_n2_no_obstacle", lambda: case([]))
_reg("lanes_n8_keypoint", lambda: case(_alternating(3)))
_reg("lanes_n16_keypoint", lambda: case(_alternating(7), thr=0.25))
_reg("lanes_n9_roadmap", lambda: case(_roadmap_rows(), keypoint=False, no_samples=7))
# the only frame that is not exact in libm (atan2, cos, sin rounded): every decision separated, vertices within 4 ulp on the device
_reg("lanes_n9_roadmap_oblique", lambda: case([("p", 3.0, 3.5), ("c", 1.0, 2.0, 0.25)], keypoint=False, no_samples=7, goal=(6.0, 5.0, 0.5), start=(0.0, 0.0, 0.75), length_scale=0.75))
_reg("lanes_n17_roadmap", lambda: case(_roadmap_rows(), keypoint=False, no_samples=15, thr=0.25))
_reg("lanes_n24_keypoint", lambda: case(_alternating(11), thr=0.25))
N23 = 23
FULL_WAVES = (N23 - 1) * N23 // 64   # the waves that hold no pair of the goal's row (it never has an edge)
IDX = {"63": 63, "64": 64, "255": K_THREADS - 1, "256": K_THREADS, "last": (N23 - 2) * N23 + N23 - 1}


def _lanes_idx(which, label):
    """every ordered pair passes the heading test (thr = -2); a point obstacle beside pair idx, dist_to_obst on a rung
    about the pair's evaluated distance: this lane alone changes between the rungs"""
    base = case([], keypoint=False, no_samples=N23 - 2, thr=-2.0)
    V = probe(base)[0]["vertices"]
    i, j = divmod(IDX[which], N23)
    assert i != j and i != N23 - 1
    d = V[j] - V[i]
    n = np.array([-d[1], d[0]]) / math.hypot(d[0], d[1])
    for frac, side in [(f, s) for f in (0.5, 0.75, 0.25) for s in (0.375, -0.375)]:
        p = np.round((V[i] + frac * d + side * n) * 1024.0) / 1024.0
        c = _with(base, rows=[("p", float(p[0]), float(p[1]))], dist_to_obst=1.0 / 64)
        dd = probe(c)[1][("dmin", i, j, 0)]
        c = _with(c, dist_to_obst=rung(dd, label), rungs=["dmin"], pair=(i, j))
        if probe(c)[0]["adjacency"][0, N23 - 1]:   # start -> goal stays free: the first path ends every enumeration
            return c
    raise AssertionError(which)


for _w in IDX:
    for _l in SHORT:
        _reg("lanes_idx%s_%s" % (_w, _l), lambda _w=_w, _l=_l: _lanes_idx(_w, _l))


def wave_survivors(c):
    """per wave of 64 pairs: (pairs that pass the heading tests, pairs with an edge)"""
    g = HG.Graph(c, "float")
    r = g.run()
    N = len(r["vertices"])
    thr = c["thr"]
    alive = np.zeros(N * N, bool)
    for k, v in g.probe.items():
        if k[0] == "fwd" and v > thr:
            alive[k[1] * N + k[2]] = True
    for k, v in g.probe.items():
        if k[0] == "head" and v <= thr:
            alive[k[1]] = False
    edge = r["adjacency"].ravel() != 0
    W = (N * N + 63) // 64
    return [(int(alive[64 * w:64 * w + 64].sum()), int(edge[64 * w:64 * w + 64].sum())) for w in range(W)]


def _lanes_waves():
    far = [("p", 4.0, 10.0), ("c", 4.0, -10.0, 0.5), ("l", -5.0, -1.0, -5.0, 1.0)]
    base = case(far, keypoint=False, no_samples=N23 - 2, thr=0.25)
    dots = sorted(v for k, v in probe(base)[1].items() if k[0] == "fwd")
    for a, b in reversed(list(zip(dots[:-1], dots[1:]))):
        if b - a < 1e-6:
            continue
        c = _with(base, thr=round(0.5 * (a + b), 9))
        w = wave_survivors(c)
        if any(s == (0, 0) for s in w[:FULL_WAVES]) and any(s == (1, 1) for s in w[:FULL_WAVES]) and probe(c)[0]["adjacency"][0, N23 - 1]:
            return c
    raise AssertionError("no threshold leaves a wave empty beside a wave with one lane")


_reg("lanes_empty_wave_beside_single_lane", _lanes_waves)


# ---- table --------------------------------------------------------------------------------------------------------------------------------
def _filler(k):
    y = 3.0 + k / 16.0
    return [("p", 4.0, y), ("c", 2.0, y, 0.125), ("l", 1.0, y, 7.0, y), ("i", 1.0, y, 7.0, y + 0.5, 0.125),
            ("g", [(3.0, y), (5.0, y), (4.0, y + 0.25)])][k % 5]


def _table(M, pos, hit):
    rows = [_filler(k) for k in range(M)]
    rows[pos] = ("p", 4.0, 0.75)   # d = 0.75 exactly
    return case(rows, keypoint=False, dist_to_obst=HG.ulps(0.75, 1) if hit else 0.75)


TABLE_SIZES = [1, 63, 64, 65, 130]
for _m in TABLE_SIZES:
    for _p in sorted({0, _m // 2, _m - 1}):
        for _h in (True, False):
            _reg("table_m%d_p%d_%s" % (_m, _p, "hit" if _h else "tie"), lambda _m=_m, _p=_p, _h=_h: _table(_m, _p, _h))

# ---- fleet members: one launch shares thr, dist_to_obst, the graph type and the number of samples ------------------------------------------
_FK = dict(thr=0.25)
_reg("fleet_k_empty", lambda: case([], **_FK))
_reg("fleet_k_n18", lambda: case(_alternating(8), **_FK))
_reg("fleet_k_m130", lambda: case([("p", 3.0, 1.5), ("c", 5.0, -1.5, 0.25)] + [("p", -1.0 - k / 16.0, 0.5 * ((k % 5) - 2)) for k in range(128)], **_FK))
_reg("fleet_k_atgoal", lambda: case([("p", 3.0, 1.5)], goal=(0.125, 0.0, 0.0), **_FK))
_FR = dict(keypoint=False, no_samples=15)
_reg("fleet_r_block", lambda: case([("p", 4.0, 0.25)], **_FR))
_reg("fleet_r_empty", lambda: case([], **_FR))
_reg("fleet_r_other", lambda: case([("c", 2.0, -1.0, 0.25), ("l", 6.0, -1.0, 6.0, 1.0)], **_FR))
_reg("fleet_r_atgoal", lambda: case([("p", 4.0, 0.25)], goal=(0.125, 0.0, 0.0), **_FR))
