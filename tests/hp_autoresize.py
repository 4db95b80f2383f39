"""A plain restatement of TimedElasticBand::autoResize (reference src/timed_elastic_band.cpp:227-286) with 80-digit headings.
NOT a test file (tests/test_hp_autoresize.py and tests/test_gpu_hp_autoresize.py use it; tests/golden/make_hp_autoresize.py stores it).

The loop of the reference on Python lists: list.insert / del for insertPose, insertTimeDiff, deletePose, deleteTimeDiff, `i -= 1` for
`i--`. No edit script, no stack of waiting halves, no chains: nothing of the oracle's (oracle/teb_oracle.cpp) or the device's
(csrc/teb_kernel.hpp, csrc/teb_autoresize_chain.hpp) formulation.

  time differences, x, y   Python floats do the reference's own IEEE operations - 0.5 * dt (:245), dt(i+1) += dt(i) - dt_ref (:258),
                           TimeDiff(i+1) + TimeDiff(i) (:269), TimeDiff(i-1) += TimeDiff(i) (:276), (a + b) / 2 (pose_se2.h:266-269) -
                           and no multiply-add: n, dt, x, y are EXACT expectations.
  headings                 PoseSE2::average takes g2o::average_angle = atan2(sin a + sin b, cos a + cos b). Every pose carries its heading
                           twice: the fp64 one (math.sin / cos / atan2, what the reference computes) and an mpmath one at 80 digits that
                           goes through the whole split tree - and from sweep to sweep - without intermediate rounding. err_ref[pose] is
                           the distance of the two (0 for input poses): the fp64 restatement's own error.
  comparisons              every comparison of the loop is recorded: which threshold (dt_ref + hyst :239, 2 dt_ref :243, dt_ref - hyst :263,
                           max_samples :239, min_samples :263), the provenance of the operand (an input interval of this sweep, one an excess
                           was pushed onto, a merged one, a half) and whether the operand EQUALS the threshold, is its upper or lower
                           fp64 neighbour, or is further away. The thresholds are formed as the reference forms them, in fp64: with the
                           defaults 0.3 - 0.1 = 0.19999999999999998, so dt = 0.2 is not too short.
  sweeps                   the band after every sweep of the outer loop is returned; with `capacity` the loop stops BEFORE a sweep whose
                           output would have more poses than that (the device returns the band as it was before such a sweep,
                           csrc/teb_kernel.hpp autoresize(): `if (ovf) return n`). restate(fast_mode=False, max_sweeps=k, stop_unmodified=False)
                           is k fast-mode calls in a row: the outer loop (:233) repeats the very same sweep on the band the previous
                           one left; it only stops after a sweep that set `modified` nowhere, which separate calls do not.

The reference has undefined behaviour where the rule of the last interval (:274-279) fires at i = 0: TimeDiff(-1). Such a band is
refused here (Undefined). Infinite time differences are out of scope (the reference splits until max_samples; the device reports
overflow when 64 halves wait): refused as well. NaN passes through - every comparison with it is false.

MUTATIONS: restate(.., mutation=name) is the same loop with one deliberate defect; tests/test_hp_autoresize.py shows that the checker
(check_band) rejects each of them on at least one case.
"""
import hashlib
import math

import numpy as np

try:
    import mpmath as mp
    mp.mp.dps = 80
except ImportError:   # the GPU test needs the fixtures only
    mp = None

EPS = float(np.finfo(float).eps)
BOUND = 256 * EPS          # the project's floor for device arithmetic through libm (tests/test_hp_linearize.py)
THR_HI, THR_BIG, THR_LO, THR_MAX, THR_MIN = range(5)          # :239 dt_ref + hyst, :243 2 dt_ref, :263 dt_ref - hyst, :239 max_samples, :263 min_samples
THR_NAMES = ("dt_ref + hyst", "2 dt_ref", "dt_ref - hyst", "max_samples", "min_samples")
P_INPUT, P_PUSHED, P_MERGED, P_HALVED = range(4)
PROV_NAMES = ("input", "pushed onto", "merged", "halved")
R_EQ, R_UP, R_DOWN, R_FAR = range(4)                           # operand == threshold, its upper neighbour, its lower neighbour, further
MUTATIONS = ("ge_at_hi", "ge_at_big", "lo_literal", "max_guard_off_by_one", "min_guard_off_by_one", "push_at_last", "tail_forward",
             "parent_i_plus_2", "right_half_first")


class Undefined(Exception):
    """the reference's behaviour on this band is undefined (or out of scope)"""


def thresholds(dt_ref, hyst):
    """(hi, big, lo) as the reference forms them"""
    return dt_ref + hyst, 2 * dt_ref, dt_ref - hyst


def relation(v, thr):
    if v == thr:
        return R_EQ
    if v == math.nextafter(thr, math.inf):
        return R_UP
    if v == math.nextafter(thr, -math.inf):
        return R_DOWN
    return R_FAR


def count_relation(size, guard):
    """sizeTimeDiffs() against a sample-count guard: equal, one above, one below, further"""
    return {0: R_EQ, 1: R_UP, -1: R_DOWN}.get(size - guard, R_FAR)


class _Pose:
    __slots__ = ("x", "y", "th", "hp", "new")

    def __init__(self, x, y, th, hp=None, new=False):
        self.x, self.y, self.th, self.hp, self.new = x, y, th, hp, new


def _average(a, b, stats):
    """PoseSE2::average (pose_se2.h:266-269); the 80-digit heading from the parents' 80-digit headings"""
    sx, sy = math.cos(a.th) + math.cos(b.th), math.sin(a.th) + math.sin(b.th)
    th = 0.0 if (sx == 0 and sy == 0) else math.atan2(sy, sx)
    hp = None
    if a.hp is not None:
        hx, hy = mp.cos(a.hp) + mp.cos(b.hp), mp.sin(a.hp) + mp.sin(b.hp)
        stats["conditioning"] = min(stats["conditioning"], float(mp.sqrt(hx * hx + hy * hy)))   # |e^ia + e^ib|: >= 1 for headings <= 2 pi / 3 apart
        hp = mp.atan2(hy, hx)
    return _Pose((a.x + b.x) / 2, (a.y + b.y) / 2, th, hp, True)


def _band(P, d):
    n = len(P)
    hi, lo, err = np.zeros(n), np.zeros(n), np.zeros(n)
    for k, p in enumerate(P):
        if p.hp is None:
            hi[k] = p.th
            continue
        hi[k] = float(p.hp)
        lo[k] = float(p.hp - mp.mpf(hi[k]))
        e = abs(p.hp - mp.mpf(p.th))
        if e > mp.pi:   # (either side of the branch cut)
            e = abs(2 * mp.pi - e)
        err[k] = float(e)
        assert p.new or err[k] == 0.0
    return dict(n=n, x=np.array([p.x for p in P]), y=np.array([p.y for p in P]), theta=np.array([p.th for p in P]),
                dt=np.array(d, np.float64), th_hi=hi, th_lo=lo, err_ref=err, new=np.array([p.new for p in P], bool))


def restate(x, y, theta, dt, dt_ref, hyst, min_samples, max_samples, fast_mode, capacity=None, mutation=None, high_precision=True,
            max_sweeps=100, stop_unmodified=True):
    """dict(sweeps=[band after sweep 1, ..], modified=[..], stopped=bool, records=[per sweep: int64 [5, 4, 4] counts over threshold x
    provenance x relation; for the two guards the relation is that of sizeTimeDiffs() to the guard], conditioning=smallest |e^ia + e^ib|
    of any average). A band: dict(n, x, y, theta (fp64), dt, th_hi, th_lo (the 80-digit heading as two doubles), err_ref, new)."""
    assert mutation is None or mutation in MUTATIONS
    if not np.all(np.isfinite(np.asarray(dt, np.float64)) | np.isnan(np.asarray(dt, np.float64))):
        raise Undefined("infinite time difference")
    hp_on = high_precision and mp is not None
    P = [_Pose(float(a), float(b), float(c), mp.mpf(float(c)) if hp_on else None) for a, b, c in zip(x, y, theta)]
    d = [float(v) for v in dt]
    assert len(d) == len(P) - 1
    hi, big, lo = thresholds(dt_ref, hyst)
    if mutation == "lo_literal":
        lo = 0.2
    gt_hi = (lambda v: v >= hi) if mutation == "ge_at_hi" else (lambda v: v > hi)
    gt_big = (lambda v: v >= big) if mutation == "ge_at_big" else (lambda v: v > big)
    max_g = max_samples + 1 if mutation == "max_guard_off_by_one" else max_samples
    min_g = min_samples - 1 if mutation == "min_guard_off_by_one" else min_samples
    stats = dict(conditioning=math.inf)
    out = dict(sweeps=[], modified=[], records=[], fired=[], splits=[], merges=[], stopped=False)
    modified, rep = True, 0
    while rep < min(100, max_sweeps) and (modified or not stop_unmodified):             # :233 (stop_unmodified = False: separate calls)
        modified = False
        saved = ([_Pose(p.x, p.y, p.th, p.hp, p.new) for p in P], list(d))
        prov = [P_INPUT] * len(d)
        rec = np.zeros((5, 4, 4), np.int64)
        splits = merges = 0
        fired = 0   # rules applied in this sweep (a sweep with none is left before either machine of the device runs)
        i = 0
        while i < len(d):                                                               # :237
            v = d[i]
            rec[THR_HI, prov[i], relation(v, hi)] += 1
            long_ = gt_hi(v)
            if long_:
                rec[THR_MAX, prov[i], count_relation(len(d), max_samples)] += 1
            if long_ and len(d) < max_g:                                                # :239
                fired += 1
                rec[THR_BIG, prov[i], relation(v, big)] += 1
                if gt_big(v):                                                           # :243
                    newtime = 0.5 * v                                                   # :245
                    splits += 1
                    d[i] = newtime
                    other = P[i + 2] if (mutation == "parent_i_plus_2" and i + 2 < len(P)) else P[i + 1]
                    P.insert(i + 1, _average(P[i], other, stats))                       # :248
                    d.insert(i + 1, newtime)                                            # :249
                    prov[i] = P_HALVED
                    prov.insert(i + 1, P_HALVED)
                    if mutation != "right_half_first":
                        i -= 1                                                          # :251
                    modified = True
                else:
                    if i < len(d) - 1:                                                  # :256
                        d[i + 1] += d[i] - dt_ref                                       # :258
                        prov[i + 1] = P_PUSHED
                    elif mutation == "push_at_last" and i > 0:
                        d[i - 1] += d[i] - dt_ref
                    d[i] = dt_ref                                                       # :260
            else:
                rec[THR_LO, prov[i], relation(v, lo)] += 1
                short = v < lo
                if short:
                    rec[THR_MIN, prov[i], count_relation(len(d), min_samples)] += 1
                if short and len(d) > min_g:                                            # :263
                    fired += 1
                    merges += 1
                    if i < len(d) - 1:                                                  # :267
                        d[i + 1] = d[i + 1] + d[i]                                      # :269
                        prov[i + 1] = P_MERGED
                        del d[i]; del prov[i]                                           # :270
                        del P[i + 1]                                                    # :271
                        i -= 1                                                          # :272
                    else:
                        if i == 0:
                            raise Undefined("the rule of the last interval at i = 0 reads TimeDiff(-1)")
                        d[i - 1] += d[i]                                                # :276
                        del d[i]; del prov[i]                                           # :277
                        del P[i + 1 if mutation == "tail_forward" else i]               # :278
                    modified = True
            i += 1
        if capacity is not None and len(P) > capacity:   # (new poses are never deleted again and the emitted count only grows: the output
            P, d = saved                                 #  of the sweep is the largest band the device has to hold)
            out["stopped"] = True
            break
        out["sweeps"].append(_band(P, d))
        out["modified"].append(modified)
        out["records"].append(rec)
        out["fired"].append(fired)
        out["splits"].append(splits)
        out["merges"].append(merges)
        if fast_mode:                                                                   # :284
            break
        rep += 1
    out["final"] = _band(P, d)
    out["conditioning"] = stats["conditioning"]
    return out


def input_hash(x, y, theta, dt, params):
    h = hashlib.sha256()
    for a in (x, y, theta, dt):
        h.update(np.ascontiguousarray(a, np.float64).tobytes())
    h.update(repr(tuple(params)).encode())
    return h.hexdigest()


def heading_bound(err_ref):
    """max(256 eps, 16 x err_ref) per pose: 256 eps is the floor for device arithmetic through libm, the factor 16 the same convention
    (two sincos and one atan2 per level of the split tree)"""
    return np.maximum(BOUND, 16 * np.asarray(err_ref))


def angle_distance(a, b):
    d = np.abs(np.asarray(a) - np.asarray(b))
    return np.minimum(d, np.abs(2 * math.pi - d))


def check_band(got, want, start_goal=None):
    """The checker of both tests. got: (x, y, theta, dt) of a band; want: a band of restate(). Returns the list of complaints (empty: the
    band is accepted) and the largest heading error among the new poses in rad.
      n equal; dt, x, y bit-equal; headings of poses that are input poses bit-equal; new headings within heading_bound(err_ref) of the
      80-digit value; start and goal (x, y, theta) untouched when start_goal = ((x, y, theta), (x, y, theta)) is given"""
    gx, gy, gth, gdt = (np.asarray(a, np.float64) for a in got)
    bad = []
    if len(gx) != want["n"]:
        return ["n = %d, expected %d" % (len(gx), want["n"])], math.nan
    same = lambda a, b: np.array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64))   # bit equality (NaN included, -0 != 0)
    for name, a, b in (("dt", gdt, want["dt"]), ("x", gx, want["x"]), ("y", gy, want["y"])):
        if len(a) != len(b) or not same(a, b):
            k = int(np.argmax(a.view(np.uint64) != b.view(np.uint64))) if len(a) == len(b) else -1
            bad.append("%s differs first at %d" % (name, k))
    new = want["new"]
    if not same(gth[~new], want["th_hi"][~new]):   # (an input heading is its own 80-digit value)
        bad.append("an input heading changed")
    err = angle_distance(gth[new] - want["th_hi"][new], want["th_lo"][new]) if new.any() else np.zeros(0)
    over = err > heading_bound(want["err_ref"][new])
    if over.any() or not np.all(np.isfinite(err)):
        bad.append("%d new headings beyond the bound, worst %.1f eps" % (int(over.sum()), float(np.max(err)) / EPS))
    if start_goal is not None:
        for k, p in ((0, start_goal[0]), (-1, start_goal[1])):
            if not same(np.array([gx[k], gy[k], gth[k]]), np.array(p, np.float64)):
                bad.append("start pose changed" if k == 0 else "goal pose changed")
    return bad, float(np.max(err)) if len(err) else 0.0
