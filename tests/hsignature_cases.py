"""Small scenes placed ON the thresholds, tiles and ranges of the H-signature kernels (csrc/teb_hsig.hpp), for the exact reference of
tests/hp_hsignature.py. NOT a test file. tests/test_hp_hsignature.py (CPU) and tests/test_gpu_hp_hsignature.py (device) run every case;
tests/golden/make_hp_hsignature.py writes their fixtures.

A case is one obstacle table (points, some moving) and ONE LIST of bands; it runs in the 2-D mode (HSignature), the 3-D mode
(HSignature3d) or both. Coordinates are dyadic where a tie is wanted; time differences are dyadic so that their running sums are exact.

  shapes2d   M = 0, 1, 2, 5, 6, 7, 8 (m = max(M - 1, 5); a = ceil(m / 2), b = m - a at odd and even m); M = 255, 256, 257, 513 with n = 3
             (one and two or more obstacles per lane of the 256, lanes without a term in the tree; obstacles on a circle, so that every
             |A_l| has the same order and a lost term shows); n = 2, 3, 257, 300 with M = 3 (the staging loop beyond 256 poses).
             M = 257 with its 2 segments also runs in 3-D: two workgroups in x of the wide kernel.
  shapes3d   M = 1, 15, 16, 17, 33, each with bands of 1, 15, 16, 17, 33 segments (the 16-obstacle tile and the 16-segment chunk of
             hsig3d_small_kernel, K_HS_TILE / K_HS_CHUNK); n = 300 with M = 2.
  range      a 5 x 5 cluster 2^-4 m apart next to obstacles metres away (product exponents 2^40 and more apart); 400 obstacles on two
             dyadic lattices 49 m apart (the running value f0 / prod leaves the fp64 range - below 2^-1090 - and returns: S ~ 2^-773,
             the terms cancel to |H| ~ 2^-1050); an obstacle exactly on the map corner bl and one on tr (f0 = 0: a term whose mantissa
             is 0 and whose exponent is the product's) - once with bl the CENTRE of the cluster, where the product exponent is the
             largest of the table, once alone; a band that returns to its start the way it came (sum_i log = 0 exactly).
  thr2d      pairs of obstacles on a common axis at 0.05 exactly and +-1 ulp, +-4 ulp, +-2^-41, +-2^-36 from it; start and goal on
             the y axis at 3.0 and the same rungs (the map guess switches form, every A_l with it); a pose exactly on a centroid
             (first, middle, last); a segment with an end point on the ray y = o_y, x < o_x from above (+0) and from below (-0), and one
             straddling it by an ulp; segments with |arg difference| = pi exactly (horizontal, vertical, reversed); a band winding once
             and twice around an obstacle, both senses.
  thr3d      consecutive poses equal with dt = 0, 2^-50 apart (below 1e-15) and 2^-49 apart (above), in space and in time only; a
             static and two moving obstacles (|v| up to max_vel_x); a static obstacle exactly on a pose (its conductor passes through an
             integration point: H_l is not finite, the band is not valid, its neighbours are untouched); a closed loop, one and a
             half loops and a clockwise loop around a static obstacle (value > 1.0).
  classes2d / classes3d   six bands and dyadic thresholds (2^-3 next to the default 0.1): pairs of bands equal, unequal, and within
             2^-10 (2-D) / 2^-6 (3-D) of the threshold either side - a goal moved (2-D) or an obstacle moved away (3-D) until the fp64
             evaluation below hits the target; the exact reference then states the margin. 3-D: bands passing an obstacle left and
             right (the sign), a looping band (not reasonable), a band through an obstacle (not valid). best = none, the first, a middle
             band; max_number_plans_in_current_class = 1, 2.

No case exceeds 520 obstacles or 300 poses, and none has both many obstacles and many poses.
"""
import cmath
import collections
import math

import numpy as np

from teb_local_planner_amd import _abi
from teb_local_planner_amd.config import TebConfig

K_THREADS, K_HS_TILE, K_HS_CHUNK = 256, 16, 16   # read back from the sources by tests/test_hp_hsignature.py
SKIP_DIST, MAP_DIST, COINCIDENT, CONDUCTOR_T = 0.05, 3.0, 1e-15, 120.0
DT = 0.25
Q = 2.0 ** -20
FAMILIES = ("shapes2d", "shapes3d", "range", "thr2d", "thr3d", "classes2d", "classes3d")
RUNGS = (("0", 0.0), ("+1ulp", 1.0), ("-1ulp", -1.0), ("+4ulp", 4.0), ("-4ulp", -4.0),
         ("+2^-41", 2.0 ** -41), ("-2^-41", -2.0 ** -41), ("+2^-36", 2.0 ** -36), ("-2^-36", -2.0 ** -36))
CLASS_LISTS = ((2.0 ** -3, -1, 1), (2.0 ** -3, -1, 2), (0.1, -1, 1), (2.0 ** -3, 0, 1), (2.0 ** -3, 0, 2), (2.0 ** -3, 3, 1), (2.0 ** -3, 3, 2),
               (0.1, 3, 2))   # (threshold, best, max_number_plans_in_current_class); best = -1 first: a handle remembers its best class


def rung(base, r):
    """base moved by the rung: a count of ulps of base (|r| >= 1) or an absolute dyadic offset"""
    name, v = r
    return base + (v * np.spacing(base) if abs(v) >= 1 else v)


def _q(v):
    return np.round(np.asarray(v, np.float64) / Q) * Q


def sine(n, amp, length=4.0, x0=0.0, y0=0.0):
    s = np.linspace(0.0, 1.0, n)
    return _q(x0 + length * s), _q(y0 + amp * np.sin(math.pi * s)), np.full(n - 1, DT)


def path(points, dt=DT):
    p = np.asarray(points, np.float64)
    return p[:, 0].copy(), p[:, 1].copy(), np.full(len(p) - 1, dt)


def ring(M, R, cx, cy, phase=0.1):
    """M points on a circle, on a grid of 2^-32 (an ulp of the library's cos / sin then changes no input)"""
    g = lambda v: round(v * 2.0 ** 32) / 2.0 ** 32
    return [(g(cx + R * math.cos(phase + 2 * math.pi * k / M)), g(cy + R * math.sin(phase + 2 * math.pi * k / M)), 0.0, 0.0) for k in range(M)]


def loop(turns, sense, r=1.0, per_turn=8, phase=0.25):
    """a polygon of `per_turn` dyadic-ish points per turn around the origin, `turns` turns (may be fractional), sense = +-1"""
    k = int(round(turns * per_turn))
    ang = [phase + sense * 2 * math.pi * i / per_turn for i in range(k + 1)]
    return path([(float(_q(r * math.cos(a))), float(_q(r * math.sin(a)))) for a in ang], 0.5)


# ---- fp64 evaluations, used only to PLACE a goal or an obstacle next to a class threshold (the exact reference states the margin) ------
def float_2d(obst, band, prescaler=1.0):
    x, y, _ = band
    O = [complex(o[0], o[1]) for o in obst]
    M = len(O)
    m = max(M - 1, 5); a = math.ceil(m / 2.0); b = m - a
    start, end = complex(x[0], y[0]), complex(x[-1], y[-1])
    d = end - start
    nrm = complex(-d.imag, d.real)
    bl, tr = (start + complex(0, -3), start + complex(3, 3)) if abs(d) < 3.0 else (start - nrm, start + d + nrm)
    H = 0j
    for l in range(M):
        A = prescaler * a * (O[l] - bl) * b * (O[l] - tr)
        for j in range(M):
            if j != l and abs(O[l] - O[j]) >= 0.05:
                A /= O[l] - O[j]
        for i in range(len(x) - 1):
            z1, z2 = complex(x[i], y[i]) - O[l], complex(x[i + 1], y[i + 1]) - O[l]
            if abs(z1) == 0 or abs(z2) == 0:
                continue
            da = cmath.phase(z2) - cmath.phase(z1)
            da = min((da, da + 2 * math.pi, da - 2 * math.pi, da + 4 * math.pi, da - 4 * math.pi), key=abs)
            H += A * complex(math.log(abs(z2)) - math.log(abs(z1)), da)
    return H


def float_3d(o, band):
    x, y, dt = band
    s1 = np.array([o[0], o[1], 0.0]); s2 = np.array([o[0] + 120 * o[2], o[1] + 120 * o[3], 120.0])
    ds = s2 - s1
    t = np.concatenate([[0.0], np.cumsum(dt)])
    H = 0.0
    for i in range(len(x) - 1):
        d = np.array([x[i + 1] - x[i], y[i + 1] - y[i], dt[i]])
        if np.linalg.norm(d) < 1e-15:
            continue
        dl = d / 10
        for k in range(10):
            r = np.array([x[i], y[i], t[i]]) + k * dl
            p1, p2 = s1 - r, s2 - r
            dd = np.cross(ds, np.cross(p1, p2)) / ds.dot(ds)
            phi = (np.cross(dd, p2) / np.linalg.norm(p2) - np.cross(dd, p1) / np.linalg.norm(p1)) / dd.dot(dd)
            H += phi.dot(dl)
    return H / (4 * math.pi)


def _bisect(f, lo, hi, target, grid):
    """f monotone on [lo, hi] through `target`: the grid point next to the crossing"""
    flo = f(lo) - target
    assert flo * (f(hi) - target) < 0, (f(lo), f(hi), target)
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        if (f(mid) - target) * flo > 0:
            lo = mid
        else:
            hi = mid
    return round(0.5 * (lo + hi) / grid) * grid


# ---- the cases --------------------------------------------------------------------------------------------------------------------------
def _case(family, obst, bands, modes=(2, 3), prescaler=1.0, class_lists=(), claims=None):
    return dict(family=family, obst=[tuple(map(float, o)) for o in obst], bands=bands, modes=tuple(modes), prescaler=float(prescaler),
                class_lists=tuple(class_lists), claims=claims or {})


def shapes2d_M(M):
    if M >= 255:   # a circle of radius 1: the two (M <= 257) / four (513) nearest neighbours either side are closer than 0.05
        return _case("shapes2d", ring(M, 1.0, 1.5, 0.25), [path([(-1.0, 0.3125), (1.5, 0.6875), (4.0, 0.125)])], modes=(2, 3) if M == 257 else (2,),
                     claims=dict(lanes=True))
    return _case("shapes2d", ring(M, 1.5, 2.0, 0.25) if M else [], [sine(9, 0.5), sine(4, -0.25)], modes=(2, 3) if M else (2,), claims=dict(ab=True))


def shapes2d_n(n):
    return _case("shapes2d", [(1.0, 1.0, 0, 0), (2.0, -0.75, 0, 0), (3.0, 0.875, 0, 0)], [sine(n, 0.5)], modes=(2,))


def shapes3d_M(M):
    obst = [(o[0], o[1], (0.02 if k % 3 == 1 else 0.0), (-0.01 if k % 3 == 1 else 0.0)) for k, o in enumerate(ring(M, 1.25, 2.0, 0.0, 0.37))]
    return _case("shapes3d", obst, [sine(s + 1, 0.5 if s % 2 else -0.5) for s in (1, 15, 16, 17, 33)], claims=dict(tiles=True))


def shapes3d_n300():
    return _case("shapes3d", [(1.0, 1.0, 0, 0), (3.0, -0.5, 0.01, 0.02)], [sine(300, 0.5)])


def _cluster(cx, cy, k=5):
    h = (k - 1) / 2.0
    return [(cx + (i - h) * 2.0 ** -4, cy + (j - h) * 2.0 ** -4, 0, 0) for j in range(k) for i in range(k)]


def range_cluster():
    return _case("range", _cluster(2.0, 1.5) + [(-6.0, 3.0, 0, 0), (9.0, -4.0, 0, 0), (2.5, -7.0, 0, 0)], [sine(12, 0.5), sine(7, -0.75)], modes=(2,),
                 claims=dict(exponent_spread=40))


def range_corner_cluster():
    # start (0, 0), goal (4, 0): bl = (0, -4), tr = (4, 4). Row 12 of the cluster is its centre: exactly on bl
    obst = _cluster(0.0, -4.0) + [(4.0, 4.0, 0, 0), (2.0, 1.5, 0, 0), (1.0, -1.25, 0, 0)]
    return _case("range", obst, [sine(12, 0.5), sine(7, -0.75)], modes=(2,), claims=dict(zero_terms=[12, 25], largest_exponent=12))


def range_corner_alone():
    return _case("range", [(0.0, -4.0, 0, 0), (4.0, 4.0, 0, 0), (2.0, 1.5, 0, 0)], [sine(12, 0.5), sine(7, -0.75)], modes=(2,), claims=dict(zero_terms=[0, 1]))


def range_lattice400():
    def lattice(cx, cy):
        return [(cx + i * 2.0 ** -4, cy + j * 2.0 ** -4, 0, 0) for j in range(20) for i in range(10)]
    return _case("range", lattice(-48.0, 2.0) + lattice(1.0, 1.0), [sine(5, 0.5), sine(3, -0.5)], modes=(2,), claims=dict(out_of_range=True))


def range_closed_band():
    out = [(0.0, 0.0), (1.0, 0.375), (2.0, 0.5), (3.0, 0.375), (4.0, 0.0)]
    return _case("range", [(2.0, 1.5, 0, 0), (1.0, -1.25, 0, 0), (3.5, 0.75, 0, 0)], [path(out + out[-2::-1]), sine(9, 0.5)], modes=(2,),
                 claims=dict(zero_sum=0))


def thr2d_skip():
    obst, want = [], []
    for k, r in enumerate(RUNGS):
        d = rung(SKIP_DIST, r)
        if k % 2 == 0:   # on a line parallel to the x axis / to the y axis in turn
            obst += [(0.0, 0.5 * k, 0, 0), (d, 0.5 * k, 0, 0)]
        else:
            obst += [(8.0 + 0.5 * k, 0.0, 0, 0), (8.0 + 0.5 * k, d, 0, 0)]
        want.append((r[0], 2 * k, 2 * k + 1, bool(d < SKIP_DIST)))
    return _case("thr2d", obst, [path([(-1.0, -1.0), (-1.25, 2.0), (-1.0, 5.0)]), path([(-1.0, -1.0), (6.0, -1.5), (14.0, -1.0)])], modes=(2,),
                 claims=dict(skip_rungs=want))


def thr2d_map():
    bands = [path([(0.0, 0.0), (0.25, 1.5), (0.0, rung(MAP_DIST, r))]) for r in RUNGS]
    return _case("thr2d", [(1.0, 1.0, 0, 0), (-1.0, 2.0, 0, 0), (0.5, 2.5, 0, 0)], bands, modes=(2,),
                 claims=dict(map_rungs=[(r[0], b, bool(rung(MAP_DIST, r) < MAP_DIST)) for b, r in enumerate(RUNGS)]))


def thr2d_on_centroid():
    obst = [(0.0, 0.0, 0, 0), (2.0, 0.5, 0, 0), (4.0, 0.0, 0, 0), (1.0, 1.5, 0, 0)]
    mid = [(0.0, 0.0), (1.0, 0.375), (2.0, 0.5), (3.0, 0.375), (4.0, 0.0)]
    return _case("thr2d", obst, [path([(0.0, 0.0), (1.0, -0.5), (2.0, -0.75), (3.0, -0.5), (4.0, -0.25)]), path([(0.0, 0.25)] + mid[1:4] + [(4.0, 0.25)]),
                                 path([(0.0, -0.25), (1.0, -0.5), (2.0, -0.75), (3.0, -0.5), (4.0, 0.0)])],
                 claims=dict(on_centroid=[(0, 0, 0), (1, 2, 1), (2, 4, 2)]))   # (band, pose, obstacle)


def thr2d_ray():
    u = 2.0 ** -53
    obst = [(1.0, 0.0, 0, 0), (0.5, 1.5, 0, 0), (-0.5, -2.0, 0, 0)]
    bands = [path([(-1.0, 0.5), (0.0, 0.0), (-1.0, -0.5), (3.0, -1.0)]),     # an end point on the ray, +0: atan2(+0, -) = +pi
             path([(-1.0, 0.5), (0.0, -0.0), (-1.0, -0.5), (3.0, -1.0)])]    # -0: atan2(-0, -) = -pi
    obst2 = [(1.0, 0.5, 0, 0)] + obst[1:]
    return [_case("thr2d", obst, bands, modes=(2,), claims=dict(ray=[(0, 1, 0, +1), (1, 1, 0, -1)])),
            _case("thr2d", obst2, [path([(-1.0, 1.0), (0.0, 0.5 + 2 * u), (-0.125, 0.5 - u), (3.0, -1.0)])], modes=(2,), claims=dict(straddle=(0, 1, 0)))]


def thr2d_pi_tie():
    obst = [(0.0, 0.0, 0, 0), (0.75, 1.5, 0, 0), (-0.5, -2.0, 0, 0)]
    bands = [path([(1.0, 0.0), (-1.0, 0.0), (-2.0, 1.0)]), path([(0.0, -1.0), (0.0, 1.0), (1.0, 2.0)]), path([(-1.0, 0.0), (1.0, 0.0), (2.0, 1.0)])]
    return _case("thr2d", obst, bands, modes=(2,), claims=dict(pi_ties=[(0, 0, 0, 0), (1, 0, 0, 0), (2, 0, 0, 0)]))   # (band, segment, obstacle, winner)


def thr2d_winding():
    obst = [(0.0, 0.0, 0, 0), (2.5, 0.5, 0, 0), (-0.5, -2.75, 0, 0)]
    return _case("thr2d", obst, [loop(1.125, +1), loop(1.125, -1), loop(2.125, +1), loop(2.125, -1)], modes=(2,), claims=dict(windings=[1, -1, 2, -2]))


def thr3d_coincident():
    def band(dx, dtt):
        x = [0.0, 0.25, 0.5, 0.5 + dx, 0.75, 1.0]
        y = [0.0, 0.125, 0.25, 0.25, 0.125, 0.0]
        return np.array(x), np.array(y), np.array([DT, DT, dtt, DT, DT])
    lo, hi = 2.0 ** -50, 2.0 ** -49
    bands = [band(0.0, 0.0), band(lo, 0.0), band(hi, 0.0), band(0.0, lo), band(0.0, hi)]
    return _case("thr3d", [(0.5, 1.0, 0, 0), (0.75, -1.0, 0.4, 0.0)], bands, claims=dict(coincident=[(0, True), (1, True), (2, False), (3, True), (4, False)]))


def thr3d_moving():
    v = TebConfig().robot.max_vel_x
    return _case("thr3d", [(2.0, 1.0, 0, 0), (1.0, -1.0, v, 0.0), (3.0, 1.5, -0.5 * v, 0.5 * v)], [sine(12, 0.5), sine(7, -0.5)], modes=(3,), claims=dict(moving=v))


def thr3d_on_conductor():
    return _case("thr3d", [(2.0, 0.5, 0, 0), (1.0, -1.5, 0, 0), (3.0, 1.75, 0.01, 0.0)],
                 [sine(9, 0.75), path([(0.0, 0.0), (1.0, 0.375), (2.0, 0.5), (3.0, 0.375), (4.0, 0.0)]), sine(9, -0.5)], modes=(3,),
                 class_lists=((2.0 ** -3, -1, 1), (2.0 ** -3, 1, 1)), claims=dict(not_finite=[(1, 0)]))   # (band, obstacle)


def thr3d_loops():
    return _case("thr3d", [(0.0, 0.0, 0, 0), (3.0, 0.5, 0, 0)], [loop(1.0, +1), loop(1.5, +1), loop(1.0, -1)],
                 class_lists=((2.0 ** -3, -1, 1),), claims=dict(above_one=[(1, 0)], loops=[0, 1, 2]))


def classes2d():
    obst = [(2.0, 0.0, 0, 0), (1.0, 1.75, 0, 0), (3.0, -1.75, 0, 0)]
    thr = 2.0 ** -3
    base = sine(9, 0.75)

    def moved(e):   # the goal moved by e along (1, 1) / 2
        x, y, dt = (v.copy() for v in base)
        x[-1] += e; y[-1] += 0.5 * e
        return x, y, dt
    H0 = float_2d(obst, base)

    def gap(e):
        d = float_2d(obst, moved(e)) - H0
        return max(abs(d.real), abs(d.imag))
    inside = _bisect(gap, 0.0, 2.0 ** -3, thr * (1 - 2.0 ** -10), 2.0 ** -40)
    outside = _bisect(gap, 0.0, 2.0 ** -3, thr * (1 + 2.0 ** -10), 2.0 ** -40)
    bands = [base, sine(9, 0.5), sine(9, -0.75), moved(inside), moved(outside), sine(7, -0.5)]
    return _case("classes2d", obst, bands, modes=(2,), class_lists=CLASS_LISTS, claims=dict(near=[(0, 3, True), (0, 4, False)], equal=[(0, 1), (2, 5)], unequal=[(0, 2)]))


def classes3d():
    thr = 2.0 ** -3
    base = sine(9, 0.75)
    f = lambda d, s: abs(float_3d((2.0, s * d, 0, 0), base))   # |H_l| of an obstacle abeam the band's middle, d metres off the axis
    above = _bisect(lambda d: f(d, -1), 0.25, 12.0, thr * (1 + 2.0 ** -6), 2.0 ** -30)
    below = _bisect(lambda d: f(d, +1), 1.0, 12.0, thr * (1 - 2.0 ** -6), 2.0 ** -30)
    obst = [(2.0, 0.0, 0, 0), (2.0, -above, 0, 0), (2.0, below, 0, 0), (1.0, 0.125, 0.002, 0.001)]
    through = path([(0.0, 0.0), (1.0, 0.375), (2.0, 0.0), (3.0, -0.375), (4.0, 0.0)])   # its middle pose is obstacle 0
    around = path([(0.0, 0.0), (1.0, -0.5), (2.0, -1.0), (3.0, 0.0), (2.0, 1.0), (1.0, 0.0), (2.0, -1.0), (3.0, 0.0), (2.0, 1.0), (1.0, 0.5), (4.0, 0.0)], 0.5)   # counter-clockwise around obstacle 0
    bands = [base, sine(9, 0.5), sine(9, -0.75), sine(7, -0.5), through, around]
    return _case("classes3d", obst, bands, modes=(3,), class_lists=CLASS_LISTS,
                 claims=dict(near3=[(0, 1, False), (0, 2, True)], sides=[(0, 2, 0)], not_finite=[(4, 0)], loops=[5]))


def _table():
    t = collections.OrderedDict()
    for M in (0, 1, 2, 5, 6, 7, 8, 255, 256, 257, 513):
        t["shapes2d_M%d" % M] = lambda M=M: shapes2d_M(M)
    for n in (2, 3, 257, 300):
        t["shapes2d_n%d" % n] = lambda n=n: shapes2d_n(n)
    for M in (1, 15, 16, 17, 33):
        t["shapes3d_M%d" % M] = lambda M=M: shapes3d_M(M)
    t["shapes3d_n300"] = shapes3d_n300
    for f in (range_cluster, range_corner_cluster, range_corner_alone, range_lattice400, range_closed_band, thr2d_skip, thr2d_map, thr2d_on_centroid):
        t[f.__name__] = f
    t["thr2d_ray_endpoint"] = lambda: thr2d_ray()[0]
    t["thr2d_ray_straddle"] = lambda: thr2d_ray()[1]
    for f in (thr2d_pi_tie, thr2d_winding, thr3d_coincident, thr3d_moving, thr3d_on_conductor, thr3d_loops):
        t[f.__name__] = f
    t["classes2d_goal"] = classes2d
    t["classes3d_abeam"] = classes3d
    return t


CASES = _table()
_BUILT = {}


def build(name):
    """the case with its host objects: `table` (ObstacleTable), `batch` (TebBatchHost), cfg(mode)"""
    if name not in _BUILT:
        c = CASES[name]()
        c["name"] = name
        t = _abi.ObstacleTable()
        for x, y, vx, vy in c["obst"]:
            t.add_point(x, y, vel=(vx, vy) if (vx != 0 or vy != 0) else None)
        nmax = max(len(b[0]) for b in c["bands"])
        batch = _abi.TebBatchHost(len(c["bands"]), max(8, -(-nmax // 8) * 8))
        for k, (x, y, dt) in enumerate(c["bands"]):
            batch.set_teb(k, x, y, np.zeros(len(x)), dt)
        c["table"], c["batch"] = t, batch
        assert len(c["obst"]) <= 520 and nmax <= 300 and not (len(c["obst"]) > 40 and nmax > 40), name
        _BUILT[name] = c
    return _BUILT[name]


def config(mode):
    cfg = TebConfig()
    cfg.obstacles.include_dynamic_obstacles = (mode == 3)   # HomotopyClassPlanner::calculateEquivalenceClass picks the class by this flag
    return cfg


def fleet_sets():
    """scene sets for the fleet forms: three cases of different M per set (their band lists one after the other), M = 0 or 1 next to
    M = 257 so that workgroups beyond a scene's own tiles take the early return; (mode, [case names])"""
    return [(2, ["shapes2d_M0", "shapes2d_M257", "classes2d_goal"]), (2, ["range_corner_cluster", "shapes2d_M1", "shapes2d_M513"]),
            (3, ["shapes2d_M1", "shapes2d_M257", "classes3d_abeam"]), (3, ["shapes3d_M33", "thr3d_on_conductor", "shapes3d_M17"])]
