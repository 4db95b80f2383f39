"""Cases ON the thresholds of isTrajectoryFeasible for tests/hp_feasibility.py: CASES[name] = dict(bands, grid, fp, r, ang,
look, dist, rungs). Shared by tests/golden/make_hp_feasibility.py and tests/test_hp_feasibility.py; the GPU test reads the fixtures only.

Conventions: grids are dyadic (res = 2^-4, dyadic origin) unless the case is about another resolution; coordinates are dyadic; poses sit
at cell centres unless the case is about a boundary; the footprint is a point (the centre cell alone) unless the case is about an outline,
so that a heading never reaches libm where it is not meant to. The ladders put tie, +-1 ulp, +-4 ulp, +-2^-41 and +-2^-36 (relative) on a
PARAMETER about an exactly representable quantity. Where a lethal cell lies under a LATER pose than the laddered segment, the index of
the first infeasible test is 1 + the number of additional samples before it: the decision shows, not only the verdict.

Families (the name up to the first "_"):
  cell    which cell a coordinate falls into: pose centre and outline vertex on the ladder about a cell boundary, in x and in y, the single
          lethal cell in column k - 1 or k; w == o, w = o - 1 ulp (off the map on an all-lethal grid), index == size and one ulp below;
          res 0.05 / 0.025 / 0.1 with origin -2: quotients whose fp64 value is an integer the exact one misses (found by search)
  codes   -1 / -2 / -3 and their precedence along an edge and across edges, 253 on an outline, nf = 1 / 2, centre off the map, a blob
          inside the outline, the closing edge, nf = 3 and 64
  raster  29 directions of the first edge of a thin triangle (all octants, the diagonal, off by one, even and odd den, zero length): one
          band per stamp on one costmap - every outline cell lethal on its own collides, every cell OFF the outline lethal does not;
          rotated outlines (every vertex separated from the cell boundaries)
  interp  the number of additional samples: ladders of inscribed_radius about dnorm, dnorm / 2, fl(dnorm / 3) and of ang about
          |delta_rot| likewise, radii found by search whose fp64 quotient is an integer the exact one misses, which ceil wins, headings
          that wrap, look_ahead_idx ending the interpolation, the recurrence against its closed form
  look    look_ahead_idx and feasibility_check_lookahead_distance: every index rule, ladders about an exact hypot, the first pose beyond
          at 1, 2, 255, 256, 257, 513, leaving and coming back, both given, the rule off
  lanes   more tests than the 256 lanes: the one colliding test at q = 0, 255, 256, 257, 511, 512, total - 1, two colliding tests in
          different sweeps, 600 additional samples between segments with none, n = 2, 3, 257, 944
  fleet   two sets of four scenes whose grids differ in res, origin and size: every scene's neighbour's grid gives another answer
  limits  a NaN pose and a NaN heading among finite ones (the 2^22 capacity cases are built by the generator: their expectation is the
          oracle's)
"""
import fractions
import math

import numpy as np

from hp_feasibility import Grid, line_cells, ulps

R = 2.0 ** -4
PI = math.pi
POINT = [(0.0, 0.0)]
LADDER = {"0": ("ulp", 0), "+1ulp": ("ulp", 1), "-1ulp": ("ulp", -1), "+4ulp": ("ulp", 4), "-4ulp": ("ulp", -4),
          "+2^-41": ("rel", 2.0 ** -41), "-2^-41": ("rel", -2.0 ** -41), "+2^-36": ("rel", 2.0 ** -36), "-2^-36": ("rel", -2.0 ** -36)}
CASES = {}
FLEETS = {}     # name -> (member case names, bands of the per-scene call)
MAX_POSES = 944


def rung(v, label):
    how, k = LADDER[label]
    return ulps(v, k) if how == "ulp" else v * (1.0 + k)


def case(name, bands, cells, ox, oy, fp=POINT, r=1.0, ang=PI, look=-1, dist=-1.0, res=R, rungs=()):
    assert name not in CASES, name
    bands = [tuple(np.asarray(a, np.float64) for a in b) for b in bands]
    CASES[name] = dict(bands=bands, grid=Grid(cells, res, ox, oy), fp=[(float(a), float(b)) for a, b in fp], r=float(r), ang=float(ang),
                       look=int(look), dist=float(dist), rungs=set(rungs))
    return CASES[name]


def transposed(name, c):
    """the same case with x and y exchanged (all headings are 0: the outline is exchanged with it)"""
    g = c["grid"]
    assert all((b[2] == 0).all() for b in c["bands"])
    return case(name, [(b[1], b[0], b[2]) for b in c["bands"]], g.cells.T.copy(), g.oy, g.ox, [(q, p) for p, q in c["fp"]], c["r"], c["ang"],
                c["look"], c["dist"], g.res, c["rungs"])


def zeros(sx, sy, fill=0):
    return np.full((sy, sx), fill, np.uint8)


def centre(o, k, res=R):
    """the centre of cell k"""
    return o + (k + 0.5) * res


def along_x(n, x0, y0, step=R, th=0.0):
    return (x0 + step * np.arange(n), np.full(n, y0), np.full(n, th))


# ================================================================ cell ========================================================================
def _cell_cases():
    ox, oy, sx, sy = -1.0, -0.5, 32, 16
    y0 = centre(oy, 8)
    for label in LADDER:
        for k, side in ((12, "k"), (12, "k-1")):
            B = ox + k * R                                     # -0.25: a negative world coordinate against a negative origin
            cells = zeros(sx, sy)
            cells[8, k if side == "k" else k - 1] = 254
            # the pose centre: pose 0 far away in a free cell, pose 1 on the ladder
            c = case("cell_centre_x_%s_%s" % (side, label), [([centre(ox, 2), rung(B, label)], [y0, y0], [0, 0])], cells, ox, oy, r=4.0,
                     rungs=("trunc", "w_lt_o"))
            transposed("cell_centre_y_%s_%s" % (side, label), c)
            # a vertex of a triangle whose two other vertices lie two columns to the left, three rows up and down: the column of the
            # laddered vertex decides which of the two cells of row 8 the outline reads. The pose is the origin of the world: w = fx.
            oy2 = -centre(0.0, 8)
            fp = [(rung(B, label), 0.0), (centre(ox, k - 3), 3 * R), (centre(ox, k - 3), -3 * R)]
            c = case("cell_vertex_x_%s_%s" % (side, label), [([0.0, 0.0], [0.0, 0.0], [0, 0])], cells, ox, oy2, fp, r=4.0, rungs=("trunc", "w_lt_o"))
            transposed("cell_vertex_y_%s_%s" % (side, label), c)
    # an origin of zero: w - o is w, every rung is exact
    for label in ("0", "+1ulp", "-1ulp"):
        for side in ("k", "k-1"):
            cells = zeros(16, 8)
            cells[4, 4 if side == "k" else 3] = 254
            c = case("cell_origin0_x_%s_%s" % (side, label), [([centre(0, 1), rung(4 * R, label)], [centre(0, 4)] * 2, [0, 0])], cells, 0.0, 0.0, r=4.0)
            transposed("cell_origin0_y_%s_%s" % (side, label), c)
    # w == o is cell 0; one ulp below is off the map, which is no collision even on an all-lethal grid
    first = zeros(8, 8); first[0, 0] = 254
    c = case("cell_w_equals_o_x", [([centre(-1.0, 3), -1.0], [centre(-0.5, 3), -0.5], [0, 0])], first, -1.0, -0.5, r=4.0)
    c = case("cell_w_above_o_x", [([centre(-1.0, 3), ulps(-1.0, 1)], [centre(-0.5, 3)] * 2, [0, 0])], first + np.uint8(254) * (np.arange(8) == 3)[:, None] * (np.arange(8) == 0)[None, :], -1.0, -0.5, r=4.0)
    transposed("cell_w_above_o_y", c)
    lethal = zeros(8, 8, 254); lethal[3, 3] = 0
    c = case("cell_w_below_o_x", [([centre(-1.0, 3), ulps(-1.0, -1)], [centre(-0.5, 3)] * 2, [0, 0])], lethal, -1.0, -0.5, r=4.0)
    transposed("cell_w_below_o_y", c)
    # index == size is off the map, one ulp below is the last cell
    for label, what in (("0", "size"), ("-1ulp", "last")):
        c = case("cell_index_%s_x" % what, [([centre(-1.0, 3), rung(-1.0 + 8 * R, label)], [centre(-0.5, 3)] * 2, [0, 0])], lethal, -1.0, -0.5, r=4.0)
        transposed("cell_index_%s_y" % what, c)
    # other resolutions: (w - o) / res in fp64 against the exact quotient of the same fp64 numbers
    F = fractions.Fraction
    for res in (0.05, 0.025, 0.1):
        o, sx = -2.0, 120
        found = {}
        for k in range(1, sx - 1):
            for d in range(-3, 4):
                w = ulps(o + k * res, d)
                qf, qx = (w - o) / res, F(w - o) / F(res)
                if qf == k and qx < k:
                    found.setdefault("fp64_on_integer_exact_below", (k, w))
                if qf == k and qx > k:
                    found.setdefault("fp64_on_integer_exact_above", (k, w))
                if int((w - o) * (1.0 / res)) != int(qf):
                    found.setdefault("reciprocal_differs", (k, w))
        assert set(found) >= {"fp64_on_integer_exact_below", "fp64_on_integer_exact_above"}, (res, found)
        for what, (k, w) in found.items():
            cells = zeros(sx, 4)
            cells[1, int((w - o) / res)] = 254
            c = case("cell_res%g_%s" % (res, what), [([centre(o, 1, res), w], [centre(o, 1, res)] * 2, [0, 0])], cells, o, o, r=8.0, res=res,
                     rungs=("trunc",))
            transposed("cell_res%g_%s_y" % (res, what), c)


# ================================================================ codes =======================================================================
TRI = [(-4 * R, -3 * R), (4 * R, -3 * R), (0.0, 4 * R)]                       # at cell (16, 16): vertices in (12, 13), (20, 13), (16, 20)
QUAD = [(-4 * R, -3 * R), (4 * R, -3 * R), (5 * R, 4 * R), (-3 * R, 3 * R)]   # (12, 13), (20, 13), (21, 20), (13, 19)


def outline(fp, at=(16, 16)):
    """the cells of every edge of an outline whose vertices are cell centres, pose at the centre of cell `at`, heading 0"""
    V = [(at[0] + math.floor(0.5 + px / R), at[1] + math.floor(0.5 + py / R)) for px, py in fp]
    return [line_cells(V[i][0], V[(i + 1) % len(V)][0], V[i][1], V[(i + 1) % len(V)][1]) for i in range(len(V))]


def _codes_cases():
    ox = oy = -1.0
    pose = [([centre(ox, 16)] * 2, [centre(oy, 16)] * 2, [0, 0])]

    def put(name, fp, values, sx=32, sy=32, fill=0, bands=pose, **kw):
        cells = zeros(sx, sy, fill)
        for (x, y), v in values.items():
            cells[y, x] = v
        return case("codes_" + name, bands, cells, ox, oy, fp, r=4.0, **kw)

    for tag, fp in (("tri", TRI), ("quad", QUAD)):
        E = outline(fp)
        inner = [[c for c in e[1:-1] if sum(c in f for f in E) == 1] for e in E]   # cells of one edge alone
        assert all(len(q) >= 2 for q in inner)
        last = len(fp) - 1
        put(tag + "_free", fp, {})
        put(tag + "_255_before_254_on_edge0", fp, {inner[0][0]: 255, inner[0][1]: 254})
        put(tag + "_254_before_255_on_edge0", fp, {inner[0][0]: 254, inner[0][1]: 255})
        put(tag + "_254_on_edge1_behind_255_on_edge0", fp, {inner[0][0]: 255, inner[1][0]: 254})
        put(tag + "_254_on_last_edge_behind_255_on_edge0", fp, {inner[0][0]: 255, inner[last][0]: 254})
        put(tag + "_254_on_edge1_before_255_on_last_edge", fp, {inner[1][0]: 254, inner[last][0]: 255})
        put(tag + "_253_on_the_outline", fp, {inner[0][0]: 253, inner[1][0]: 253, E[0][0]: 253})
        put(tag + "_252_everywhere", fp, {}, fill=252)
        put(tag + "_closing_edge_only", fp, {inner[last][0]: 254})
        put(tag + "_first_vertex_cell", fp, {E[0][0]: 254})
        put(tag + "_blob_inside", fp, {(16, 16): 254, (15, 16): 254, (16, 15): 254, (17, 16): 254})
        put(tag + "_everything_off_the_outline_unknown_or_lethal", fp,
            {(x, y): (254 if (x + y) % 2 else 255) for x in range(32) for y in range(32) if not any((x, y) in e for e in E)})
    E = outline(TRI)
    # vertex 1 (column 20) off a map of 20 columns: edge 0 returns -3 before the lethal cell of edge 2 is read
    put("tri_offmap_vertex_on_edge0_lethal_on_edge2", TRI, {E[2][2]: 254}, sx=20)
    put("tri_lethal_on_edge0_offmap_vertex_on_edge1", [TRI[0], TRI[1], (0.0, 20 * R)], {E[0][3]: 254})
    E = outline(QUAD)
    # vertex 2 (column 21): edges 1 and 2 have it, edge 3 is read after them
    put("quad_offmap_vertex_on_edge1_lethal_on_edge3", QUAD, {E[3][2]: 254}, sx=21)
    put("quad_lethal_on_edge0_offmap_vertex_on_edge2", [QUAD[0], QUAD[1], QUAD[2], (-3 * R, 20 * R)], {E[0][3]: 254})
    put("quad_all_lethal_first_vertex_offmap", [(-20 * R, -3 * R)] + QUAD[1:], {}, fill=254)
    # fewer than three vertices: the centre cell alone, where 253 is lethal as well
    for nf, fp in ((1, POINT), (2, [(-2 * R, 0.0), (3 * R, 0.0)])):
        for v in (252, 253, 254, 255):
            put("nf%d_centre_%d" % (nf, v), fp, {(16, 16): v})
    put("nf2_lethal_under_the_second_vertex", [(-2 * R, 0.0), (3 * R, 0.0)], {(19, 16): 254, (14, 16): 254})
    # the centre off the map, every vertex on it and on lethal cells
    put("centre_offmap_vertices_on_lethal", [(6 * R, -R), (9 * R, -R), (8 * R, 2 * R)], {}, fill=254,
        bands=[([centre(ox, -3)] * 2, [centre(oy, 16)] * 2, [0, 0])])
    put("centre_onmap_same_outline", [(6 * R, -R), (9 * R, -R), (8 * R, 2 * R)], {}, fill=254,
        bands=[([centre(ox, 2)] * 2, [centre(oy, 16)] * 2, [0, 0])])
    # 64 vertices (the ABI's limit): 63 along the bottom edge, an eighth of a cell apart, the apex last
    fp64 = [(-4 * R + i * R / 8, -3 * R) for i in range(63)] + [(0.0, 4 * R)]
    E = outline(fp64)
    only_closing = [c for c in E[63][1:-1] if sum(c in e for e in E) == 1]
    put("nf64_closing_edge_only", fp64, {only_closing[0]: 254})
    put("nf64_unknown_on_edge0_lethal_on_the_closing_edge", fp64, {E[0][0]: 255, only_closing[0]: 254})
    put("nf64_free", fp64, {E[0][0]: 253})


# ================================================================ raster ======================================================================
DIRECTIONS = [(8, 0), (-8, 0), (0, 7), (0, -7), (5, 5), (-5, 5), (5, -5), (-5, -5), (6, 6), (6, 5), (5, 6), (-6, 5), (-5, 6), (6, -5), (5, -6),
              (-6, -5), (-5, -6), (8, 3), (3, 8), (-7, 2), (2, -7), (-8, -3), (-3, -8), (7, -2), (-2, 7), (0, 0), (1, 0), (1, 1), (-1, 2)]
STAMP = 11


def raster_outline(dx, dy, c0):
    """cells of the thin triangle (c0, c0 + d, c0 + d again): the edge, a zero-length edge, and the way back"""
    c1 = (c0[0] + dx, c0[1] + dy)
    return [line_cells(c0[0], c1[0], c0[1], c1[1]), line_cells(c1[0], c1[0], c1[1], c1[1]), line_cells(c1[0], c0[0], c1[1], c0[1])]


def _raster_cases():
    ox, oy = -0.5, -0.25
    for dx, dy in DIRECTIONS:
        c0 = (1 + max(0, -dx), 1 + max(0, -dy))
        cells_on = sorted(set(c for e in raster_outline(dx, dy, c0) for c in e))
        n = len(cells_on) + 1
        grid = zeros(n * STAMP, STAMP)
        bands = []
        for k, c in enumerate(cells_on):            # stamp k: that cell alone
            grid[c[1], k * STAMP + c[0]] = 254
        k = n - 1                                   # the last stamp: every cell OFF the outline
        grid[:, k * STAMP:] = 254
        for c in cells_on:
            grid[c[1], k * STAMP + c[0]] = 0
        for k in range(n):
            x, y = centre(ox, k * STAMP + c0[0]), centre(oy, c0[1])
            bands.append(([x, x], [y, y], [0, 0]))
        case("raster_dir_%+d_%+d" % (dx, dy), bands, grid, ox, oy, [(0.0, 0.0), (dx * R, dy * R), (dx * R, dy * R)], r=4.0)
    # rotated outlines: through libm, so every vertex must be SEPARATED from the cell boundaries (asserted from the records)
    quad = [(-0.27, -0.19), (0.41, -0.16), (0.36, 0.22), (-0.21, 0.17)]
    for th in (0.3, 1.0, 2.5, -2.0, 3.0):
        pose = (centre(-1.0, 16) + 0.013, centre(-1.0, 16) - 0.008, th)
        V = [(pose[0] + (px * math.cos(th) - py * math.sin(th)), pose[1] + (px * math.sin(th) + py * math.cos(th))) for px, py in quad]
        C = [(int((vx + 1.0) / R), int((vy + 1.0) / R)) for vx, vy in V]
        on = set(c for i in range(4) for c in line_cells(C[i][0], C[(i + 1) % 4][0], C[i][1], C[(i + 1) % 4][1]))
        band = [([pose[0]] * 2, [pose[1]] * 2, [th, th])]
        off = zeros(32, 32, 254)
        for c in on:
            off[c[1], c[0]] = 0
        case("raster_rotated_%g_off_the_outline" % th, band, off, -1.0, -1.0, quad, r=4.0)
        for which, c in (("first", min(on)), ("last", max(on))):
            one = zeros(32, 32)
            one[c[1], c[0]] = 254
            case("raster_rotated_%g_%s_cell" % (th, which), band, one, -1.0, -1.0, quad, r=4.0)


# ================================================================ interp ======================================================================
def _interp_band(ddx, ddy, th0=0.0, th1=0.0, tail=1):
    """pose 0 at the centre of cell (8, 8) of a grid at (-0.5, -0.5), pose 1 = pose 0 + delta, then `tail` poses a cell apart"""
    x0 = y0 = centre(-0.5, 8)
    xs = [x0, x0 + ddx] + [x0 + ddx + (k + 1) * R for k in range(tail)]
    return (xs, [y0, y0 + ddy] + [y0 + ddy] * tail, [th0, th1] + [th1] * tail)


def _lethal_under(band, i, sx=32, sy=32, o=-0.5):
    cells = zeros(sx, sy)
    cells[int((band[1][i] - o) / R), int((band[0][i] - o) / R)] = 254
    return cells


def _interp_cases():
    o = -0.5
    DX, DY, DN = 3 * 2.0 ** -3, 4 * 2.0 ** -3, 0.625
    band = _interp_band(DX, DY)
    under2 = _lethal_under(band, 2)
    for div, about in ((1, DN), (2, DN / 2), (3, DN / 3)):
        for label in LADDER:
            case("interp_radius_dnorm/%d_%s" % (div, label), [band], under2, o, o, r=rung(about, label), rungs=("ceil_dist",))
    # radii whose fp64 quotient is an integer that the exact quotient misses, on either side
    F = fractions.Fraction
    found = {}
    for k in range(3, 60):
        for d in range(-4, 5):
            r = ulps(DN / k, d)
            qf, qx = DN / r, F(DN) / F(r)
            if qf == k and qx > k:
                found.setdefault("exact_above", (k, r))
            if qf == k and qx < k:
                found.setdefault("exact_below", (k, r))
    assert len(found) == 2, found
    for what, (k, r) in found.items():
        case("interp_radius_fp64_integer_%d_%s" % (k, what), [band], under2, o, o, r=r, rungs=("ceil_dist",))
    # the same on ang about an exact |delta_rot| = 0.5 (dyadic headings), the poses a quarter cell apart
    turn = _interp_band(R / 4, 0.0, 0.25, 0.75)
    t2 = _lethal_under(turn, 2)
    for div, about in ((1, 0.5), (2, 0.25), (3, 0.5 / 3)):
        for label in LADDER:
            case("interp_ang_rot/%d_%s" % (div, label), [turn], t2, o, o, r=1.0, ang=rung(about, label), rungs=("ceil_rot",))
    found = {}
    for k in range(3, 60):
        for d in range(-4, 5):
            a = ulps(0.5 / k, d)
            qf, qx = 0.5 / a, F(0.5) / F(a)
            if qf == k and qx != k:
                found.setdefault("exact_above" if qx > k else "exact_below", (k, a))
    assert len(found) == 2, found
    for what, (k, a) in found.items():
        case("interp_ang_fp64_integer_%d_%s" % (k, what), [turn], t2, o, o, r=1.0, ang=a, rungs=("ceil_rot",))
    back = _interp_band(R / 4, 0.0, 0.75, 0.25)
    case("interp_ang_negative_turn_tie", [back], _lethal_under(back, 2), o, o, r=1.0, ang=0.25)
    case("interp_ang_negative_turn_-1ulp", [back], _lethal_under(back, 2), o, o, r=1.0, ang=ulps(0.25, -1), rungs=("ceil_rot",))
    # which ceil wins: rot 3 / dist 2, rot 2 / dist 3, both 3; and one trigger alone
    both = _interp_band(DX, DY, 0.25, 0.75)
    b2 = _lethal_under(both, 2)
    for name, r, ang in (("rot_wins", 0.5, 0.2), ("dist_wins", 0.15, 0.3), ("equal", 0.25, 0.2), ("rot_alone", 1.0, 0.125), ("dist_alone", 0.25, 1.0),
                         ("none", 1.0, 1.0)):
        case("interp_max_" + name, [both], b2, o, o, r=r, ang=ang)
    # headings that wrap: 3 -> -3 and back (delta_rot = -+(6 - 2 pi), samples cross +-pi), a pose heading of exactly pi
    for name, th0, th1 in (("3_to_-3", 3.0, -3.0), ("-3_to_3", -3.0, 3.0), ("pi_to_pi", PI, PI), ("pi_to_-3", PI, -3.0), ("-3_to_pi", -3.0, PI),
                           ("7_to_-7", 7.0, -7.0), ("-pi_to_3", -PI, 3.0)):
        w = _interp_band(R / 4, 0.0, th0, th1)
        case("interp_wrap_" + name, [w], _lethal_under(w, 2), o, o, r=1.0, ang=0.1)
    # look_ahead_idx = 1: the segment 1 -> 2 is not interpolated. The lethal cell lies under its first sample only.
    far = (band[0][:2] + [band[0][1] + DX], band[1][:2] + [band[1][1] + DY], [0.0] * 3)
    cells = zeros(32, 32)
    cells[int((far[1][1] + DY / 2 - o) / R), int((far[0][1] + DX / 2 - o) / R)] = 254
    for look in (1, 2, -1):
        case("interp_stops_at_look_%d" % look, [far], cells, o, o, r=0.5, look=look)
    # the recurrence p += delta / (n + 1) against the closed form p + k * (delta / (n + 1)): a step, a k and a cell boundary between the two
    hit = None
    for n1 in (3, 7):
        for j in range(1, 64):
            for m in range(1, 40):
                p0, d = j * 2.0 ** -6, m * 2.0 ** -5
                s, p = d / n1, p0
                for k in range(1, n1):
                    p = p + s
                    q = p0 + k * s
                    if p != q and hit is None and p0 >= 0.25 and q - p0 < 1.5 * R:   # so that hi - 2 * R is exact and pose 0 on the map
                        hit = (n1, p0, d, k, p, q)
    assert hit is not None
    n1, p0, d, k, p, q = hit
    hi = max(p, q)
    col = 2
    ox = hi - col * R                    # the larger of the two is exactly the lower boundary of column col
    assert ox + col * R == hi and (hi - ox) / R == float(col) and int((min(p, q) - ox) / R) == col - 1 and p0 > ox
    y0 = centre(o, 2)
    cells = zeros(col + int(d / R) + 4, 4)
    cells[2, int((p - ox) / R)] = 254
    case("interp_recurrence_not_closed_form", [([p0, p0 + d], [y0] * 2, [0.0] * 2)], cells, ox, o, r=ulps(d / n1, 2), rungs=("trunc", "ceil_dist"))
    CASES["interp_recurrence_not_closed_form"]["note"] = (n1, k)


# ================================================================ look ========================================================================
def _look_cases():
    o = -0.5
    S = 2.0 ** -6

    def triple(a, b, n):
        x0 = y0 = centre(o, 2)
        return ([x0 + a * S * i for i in range(n)], [y0 + b * S * i for i in range(n)], [0.0] * n)

    def under(band, i, sx=40, sy=40):
        return _lethal_under(band, i, sx, sy, o)

    n = 6
    band = triple(3, 4, n)       # poses 5 / 64 apart: no additional samples at r = 0.125
    for look in (-1, 0, 1, n - 2, n - 1, n, 1000):
        eff = n - 1 if look < 0 or look >= n else look
        for where in ("look", "look+1"):
            i = eff if where == "look" else eff + 1
            if i < n:
                case("look_idx_%d_lethal_under_%s" % (look, where), [band], under(band, i), o, o, r=0.125, look=look)
    for a, b, c in ((3, 4, 5), (5, 12, 13)):
        band = triple(a, b, 6)
        for label in LADDER:    # pose 3 is at c * 3 / 64 exactly: at the tie it is not beyond, the last checked pose is 3; below, 2
            case("look_dist_%d%d%d_%s" % (a, b, c, label), [band], under(band, 3), o, o, r=0.25, dist=rung(c * 3 * S, label))
    # the first pose beyond at 1 (nothing interpolated), 2, 255, 256, 257, 513: n = 600 along x, a cell apart
    long = along_x(600, centre(o, 1), centre(o, 1))
    for i in (1, 2, 255, 256, 257, 513):
        for where, j in (("last_checked", i - 1), ("first_beyond", i)):
            cells = zeros(604, 3)
            cells[1, 1 + j] = 254
            case("look_beyond_%d_lethal_under_%s" % (i, where), [long], cells, o, o, r=R, dist=(i - 0.5) * R)
    # out and back: the first exceedance wins although later poses are inside again
    back = ([centre(o, 2 + k) for k in (0, 1, 2, 3, 4, 4, 3, 2, 1)], [centre(o, 2)] * 5 + [centre(o, 3)] * 4, [0.0] * 9)
    for name, dist, cell in (("beyond", 3.5 * R, (6, 2)), ("inside_again", 3.5 * R, (4, 3)), ("last_inside", 3.5 * R, (5, 2)),
                             ("tie_at_pose_4", 4 * R, (6, 2)), ("far_enough", 100 * R, (4, 3))):
        cells = zeros(16, 8)
        cells[cell[1], cell[0]] = 254
        case("look_leaves_and_returns_" + name, [back], cells, o, o, r=R, dist=dist)
    # no pose beyond: look_ahead_idx stands; both given, in both orders; the rule off
    band = along_x(8, centre(o, 1), centre(o, 1))
    for name, look, dist, j in (("none_beyond_idx_stands", 3, 100.0, 4), ("none_beyond_idx_stands_hit", 3, 100.0, 3),
                                ("dist_raises_idx", 2, 4.5 * R, 4), ("dist_raises_idx_clear", 2, 4.5 * R, 5),
                                ("dist_lowers_idx", 6, 2.5 * R, 3), ("dist_lowers_idx_hit", 6, 2.5 * R, 2),
                                ("dist_zero_is_off", 3, 0.0, 3), ("dist_zero_is_off_clear", 3, 0.0, 4),
                                ("dist_negative_is_off", -1, -2.5 * R, 7), ("dist_tiny", -1, 2.0 ** -1000, 0), ("dist_tiny_clear", -1, 2.0 ** -1000, 1)):
        cells = zeros(12, 3)
        cells[1, 1 + j] = 254
        case("look_" + name, [band], cells, o, o, r=R, look=look, dist=dist)
    # hypot must not square: 3-4-5 scaled by 2^-600 squares to zero, its hypot is 5 * 2^-600 > 4.5 * 2^-600. All poses share one cell.
    T = 2.0 ** -600
    tiny = ([-3 * T, 0.0, 3 * T, 6 * T], [-4 * T, 0.0, 4 * T, 8 * T], [0.0] * 4)      # pose 0 is off a map that begins at (0, 0)
    for name, dist in (("cut_at_0", 4.5 * T), ("tie_at_1", 5 * T)):
        case("look_hypot_does_not_square_" + name, [tiny], zeros(4, 4, 254), 0.0, 0.0, r=R, dist=dist)


# ================================================================ lanes =======================================================================
def _lanes_cases():
    o = -0.5
    n = 600
    hits = [[0], [255], [256], [257], [511], [512], [n - 1], [45, 300], [300, 513], [300, 557], [257, 512], []]
    cells = zeros(n + 4, 2 * len(hits) + 1)
    bands = []
    for k, qs in enumerate(hits):
        bands.append(along_x(n, centre(o, 1), centre(o, 2 * k + 1)))
        for q in qs:
            cells[2 * k + 1, 1 + q] = 254
    case("lanes_600_tests_one_per_pose", bands, cells, o, o, r=R)
    # 600 additional samples in one segment between segments with none: 3 poses a cell apart, a segment of 601 cells, 3 poses
    def long_segment(length_cells, row, x_off=0.0):
        x0 = centre(o, 1) + x_off
        xs = [x0, x0 + R, x0 + 2 * R]
        xs += [xs[-1] + length_cells * R + k * R for k in range(3)]
        return (xs, [centre(o, row)] * 6, [0.0] * 6)
    bands, cells = [], zeros(612, 9)
    for k, col in enumerate((3 + 1, 3 + 600, 3 + 601, 3 + 602)):       # its first sample, its last one, the pose after it, the one after that
        bands.append(long_segment(601, 2 * k + 1))
        cells[2 * k + 1, col] = 254
    case("lanes_600_samples_between_segments_with_none", bands, cells, o, o, r=R)
    # the same with a step that is no dyadic number, and the pose after the long segment exactly ON a cell boundary: the recurrence,
    # carried one step further, ends beside that pose (found by search: below it)
    hit = None
    x3 = o + 610 * R                          # a boundary
    for extra in (0.25, 0.375, 0.125, 0.4375, 0.3125, 0.1875):
        x2 = x3 - (600 + extra) * R
        p, s = x2, (x3 - x2) / 601.0
        for _ in range(601):
            p = p + s
        if p < x3 and hit is None:
            hit = (x2, x3)
    assert hit is not None
    x2, x3 = hit
    xs = [x2 - 2 * R, x2 - R, x2, x3, x3 + R, x3 + 2 * R]
    cells = zeros(616, 3)
    cells[1, 610] = 254
    case("lanes_pose_on_a_boundary_after_600_samples", [(xs, [centre(o, 1)] * 6, [0.0] * 6)], cells, o, o, r=R)
    # n = 2, 3, 257, 944: the lethal cell under the last pose
    for n in (2, 3, 257, MAX_POSES):
        cells = zeros(n + 2, 3)
        cells[1, n] = 254
        case("lanes_n%d_last_pose" % n, [along_x(n, centre(o, 1), centre(o, 1))], cells, o, o, r=R)
    # 944 poses 2^-6 apart on the strip, every segment with one additional sample (r just below the spacing): 1887 tests, the last collides
    S = 2.0 ** -6
    cells = zeros(240, 3)
    cells[1, int((centre(o, 1) + 943 * S - o) / R)] = 254
    band = along_x(MAX_POSES, centre(o, 1), centre(o, 1), S)
    case("lanes_n944_one_sample_per_segment", [band], cells, o, o, r=ulps(S, -1), rungs=("ceil_dist",))


# ================================================================ fleet =======================================================================
def _fleet_cases():
    band = along_x(12, 0.03125, 0.03125, 0.0625)
    specs = {"fleeta": [(R, -0.5, -0.5, 40, 20, 5), (R / 2, -0.25, -0.125, 70, 30, 7), (2 * R, -1.0, -0.5, 24, 12, 3), (R, -0.75, -0.25, 44, 16, 9)],
             "fleetb": [(R / 2, -0.5, -0.5, 80, 40, 2), (R, -0.5, -0.5, 40, 20, 11), (R, -0.25, -0.5, 36, 20, 6), (2 * R, -0.5, -1.0, 20, 20, None)]}
    for fleet, grids in specs.items():
        members = []
        for s, (res, ox, oy, sx, sy, under) in enumerate(grids):
            cells = zeros(sx, sy)
            if under is None:     # a lethal row beside the band: this scene is feasible, on its neighbour's grid it is not
                cells[int((band[1][0] - oy) / res) + 2, :] = 254
            else:
                cells[int((band[1][under] - oy) / res), int((band[0][under] - ox) / res)] = 254
            name = "fleet_%s_scene%d" % (fleet[-1], s)
            case(name, [band], cells, ox, oy, r=0.0625, res=res)
            members.append(name)
        FLEETS[fleet] = (members, [0, 1, 2, 3] if fleet == "fleeta" else [0, 1, -1, 3])


# ================================================================ limits ======================================================================
def _limits_cases():
    o = -0.5
    nan = math.nan
    x, y, th = along_x(6, centre(o, 1), centre(o, 1))
    for name, i, col in (("nan_x", 2, 0), ("nan_y", 2, 1), ("nan_heading", 2, 2)):
        for where, j in (("hit_behind_it", 4), ("hit_before_it", 1), ("clear", None)):
            b = [x.copy(), y.copy(), th.copy()]
            b[col][i] = nan
            cells = zeros(8, 3)
            if j is not None:
                cells[1, 1 + j] = 254
            cells[0, :] = 254; cells[:, 0] = 254   # where a conversion of NaN to 0 would look
            case("limits_%s_%s" % (name, where), [tuple(b)], cells, o, o, r=R)
    # a NaN heading beside segments that ARE interpolated: std::max(NaN, d) is its first argument, and x86's cast of NaN - 1 asks for no sample
    b = (x.copy(), y.copy(), th.copy()); b[2][2] = nan
    cells = zeros(8, 3); cells[1, 5] = 254; cells[0, :] = 254; cells[:, 0] = 254
    case("limits_nan_heading_interpolated_segments", [b], cells, o, o, r=R / 2)
    # a NaN heading under an outline: every vertex is NaN, the test is off the map
    b = (x.copy(), y.copy(), th.copy()); b[2][2] = nan
    cells = zeros(8, 3, 254)
    cells[1, 1:3] = 0; cells[1, 4:7] = 0
    case("limits_nan_heading_outline", [b], cells, o, o, fp=[(0.0, 0.0), (R / 4, 0.0), (0.0, R / 4)], r=R)


FAMILIES = ["cell", "codes", "raster", "interp", "look", "lanes", "fleet", "limits"]
for _f in (_cell_cases, _codes_cases, _raster_cases, _interp_cases, _look_cases, _lanes_cases, _fleet_cases, _limits_cases):
    _f()
