"""Exact reference of the EQUIVALENCE CLASS of a band: its H-signature and the class decisions taken from it. NOT a test file.

It restates, over mpmath at 80 digits and on the fp64 inputs as they are, the text of the reference planner and nothing else:
  HSignature::calculateHSignature    include/teb_local_planner/h_signature.h:96-188   (2-D, complex logarithm)
  HSignature3d::calculateHSignature  include/teb_local_planner/h_signature.h:281-347  (x-y-t, the ten-step rule per segment)
  isEqual / isValid / isReasonable of both (:195-227, :359-411) and the class list of renewAndAnalyzeOldTebs /
  addEquivalenceClassIfNew (src/homotopy_class_planner.cpp:178-254).

2-D.  m = max(M - 1, 5), a = ceil(m / 2), b = m - a; the map guess from |end - start| < 3.0; A_l = prescaler a (o_l - bl) b (o_l - tr)
      prod_{j != l, |o_l - o_j| >= 0.05} 1 / (o_l - o_j); per segment and obstacle log|z2 - o| - log|z1 - o| and the argument
      difference reduced to the FIRST smallest |.| of {+0, +2pi, -2pi, +4pi, -4pi}, with 2pi and 4pi the fp64 values the reference adds;
      a segment with a pose ON the obstacle is skipped (diff == 0). Returned: H, the scale S = sum_l |A_l| sum_i (|log d_i+1| + |log d_i|
      + |arg_i+1| + |arg_i|), per obstacle |A_l| and L_l = sum_i log_value.
      The selection among the five proposals is the one decision of the rule that the reference takes on ROUNDED operands (`double
      arg_diff = std::arg(..) - std::arg(..)`): it is restated on the arguments rounded to fp64 (a rounding of 7e-17 relative, far
      below REL, so a separated selection is the same on the exact arguments). A selection closer than REL is admissible only when
      both points lie on an axis through the obstacle - there every atan2 returns a rounded constant (0, +-pi/2, +-pi) - and the fp64
      replay gives the same operands: this is how |arg difference| = pi is a TIE between arg and arg -+ 2pi that the order of the
      proposals decides, as in the reference, although pi itself is no fp64 number. The sign of a zero imaginary part (atan2(+-0, -)
      = +-pi) is taken from the fp64 subtraction y - o_y, which is exact. The VALUE added is the exact argument difference plus the
      chosen fp64 multiple of 2pi.
3-D.  per obstacle s1 = (centroid, 0), s2 = (centroid + 120 v, 120); transition times are the sums of the time differences, so the
      third component of a segment is its time difference; a segment of norm < 1e-15 is skipped; ten steps r = z1 + k dl, dl = dir / 10:
      d = ds x (p1 x p2) / |ds|^2, phi = (d x p2 / |p2| - d x p1 / |p1|) / |d|^2, H += phi . dl; H_l = H / (4 pi), pi the fp64 value of
      the text. It is the rule, not the line integral. Returned: H_l, the scale T_l = sum_steps (|phi_0 dl_0| + |phi_1 dl_1| +
      |phi_2 dl_2|) / (4 pi). A step with |p1|, |p2| or |d| zero makes H_l NOT FINITE (None), as IEEE arithmetic does (x / 0).

Admissibility (the rule of tests/hp_association.py). EVERY comparison is recorded with its relative margin |a - b| / max(|a|, |b|):
|o_l - o_j| against 0.05, |end - start| against 3.0, each of the five proposals against the winner, diff against 0, the direction norm
against 1e-15, |d|, |p1|, |p2| of an integration step against 0. A comparison is admissible when it is
  separated: relative margin >= REL = 1e-9, or
  exact:     both operands evaluated with every operation rounded to 53 bits (mpmath at prec = 53) EQUAL their 80-digit values; it
             may then be a tie or ulps apart.
Anything else raises InadmissibleError; nothing is dropped. A CLASS decision (|dRe|, |dIm| against the threshold in 2-D; |H_l| against
it, the sign and H_l > 1.0 in 3-D) is measured against the error an implementation is ALLOWED: its margin must exceed
CLASS_GUARD x DEVICE_CAP eps x the scale of the operands (S of both bands, T_l), DEVICE_CAP = 16 x ORACLE_BOUND being the largest error
the device's bound can ever grant. A decision closer than that is a badly built case and raises.

Error units (no mpmath needed from here on: the GPU test uses these): 2-D max(|dRe|, |dIm|) / (eps S) per BAND, 3-D |d| / (eps T_l) per
band and obstacle, against the exact value kept as two doubles (hi + lo). Oracle <= ORACLE_BOUND, device <= max(FLOOR, FACTOR x the
oracle's error on the same case); not finite where and only where the reference is.
"""
import math

import numpy as np

try:
    import mpmath
    from mpmath import mpf, mpc
except ImportError:   # the error units and bounds below are all the GPU test uses
    mpmath, mpf, mpc = None, None, None

DPS = 80
REL = 1e-9
EPS = float(np.finfo(float).eps)
TWO_PI, FOUR_PI = 2 * math.pi, 4 * math.pi          # 2*M_PI, 4*M_PI of the text: fp64
SKIP_DIST, MAP_DIST, COINCIDENT, CONDUCTOR_T, STEPS = 0.05, 3.0, 1e-15, 120.0, 10
ORACLE_BOUND, FLOOR, FACTOR = 4096.0, 256.0, 16.0
DEVICE_CAP = FACTOR * ORACLE_BOUND
CLASS_GUARD = 2.0


class InadmissibleError(ValueError):
    pass


class Recorder:
    """records: (what, index tuple, relative margin, exact: True / None (not needed), a < b, a == b)"""

    def __init__(self):
        self.records = []

    def compare(self, what, idx, a, b, replay=None, extra_ok=True):
        """a against b (80-digit values); replay() -> the same two operands with every operation rounded to 53 bits"""
        s = max(abs(a), abs(b))
        rel = float(abs(a - b) / s) if s != 0 else 0.0
        exact = None
        if rel < REL:
            if replay is None:
                exact = True   # both operands are inputs or literals
            else:
                with mpmath.workprec(53):
                    a53, b53 = replay()
                exact = bool(a53 == a and b53 == b)
            if not (exact and extra_ok):
                raise InadmissibleError("%s %s: relative margin %.3g < %g and the operands are not exact in fp64 (%s, %s)"
                                        % (what, idx, rel, REL, mpmath.nstr(a, 25), mpmath.nstr(b, 25)))
        self.records.append((what, idx, rel, exact, bool(a < b), bool(a == b)))
        return a < b, a == b

    def summary(self, prefix=""):
        """(comparisons, exact ones, ties among them, smallest relative margin of the separated ones)"""
        rs = [r for r in self.records if r[0].startswith(prefix)]
        ex = [r for r in rs if r[3]]
        sep = [r[2] for r in rs if not r[3]]
        return len(rs), len(ex), sum(r[5] for r in ex), min(sep) if sep else float("inf")


def _norm2(re, im):
    return mpmath.sqrt(re * re + im * im)


# ---- 2-D ------------------------------------------------------------------------------------------------------------------------------
def signature_2d(ox, oy, x, y, prescaler, rec, band=0, mutate=None):
    """dict(H mpc, S mpf, A [M] mpc, absA [M] mpf, absP [M] mpf: |prod_j 1 / (o_l - o_j)|, L [M] mpc, a, b, small_map: the
    |end - start| < 3.0 branch, skipped_pairs, skipped_segments [(i, l)], selections {(i, l): index of the winning proposal}).
    mutate: one of ("unwrap", l, i), ("exponent", l), ("swap_ab",), ("b_equals_a",), ("flip_skip", l, j), ("drop_last_segment",),
    ("drop_term", l) - the wrong answers the checker must reject (swap_ab is none: a and b enter the text only as a * b)."""
    mutate = mutate or ("none",)
    M, n = len(ox), len(x)
    with mpmath.workdps(DPS):
        if M == 0:
            return dict(H=mpc(0), S=mpf(0), A=[], absA=[], absP=[], L=[], a=0, b=0, small_map=None, skipped_pairs=[], skipped_segments=[], selections={})
        m = max(M - 1, 5)
        a = int(math.ceil(m / 2.0))
        b = m - a
        if mutate[0] == "swap_ab":
            a, b = b, a
        if mutate[0] == "b_equals_a":
            b = a
        O = [(mpf(float(ox[l])), mpf(float(oy[l]))) for l in range(M)]
        Z = [(mpf(float(x[i])), mpf(float(y[i]))) for i in range(n)]
        start, end = Z[0], Z[n - 1]
        delta = (end[0] - start[0], end[1] - start[1])
        small, _ = rec.compare("2d map guess", (band,), _norm2(*delta), mpf(MAP_DIST),
                               lambda: (_norm2(end[0] - start[0], end[1] - start[1]), mpf(MAP_DIST)))
        if small:
            bl = (start[0] + 0, start[1] - 3)
            tr = (start[0] + 3, start[1] + 3)
        else:   # normal = (-delta.im, delta.re)
            bl = (start[0] + delta[1], start[1] - delta[0])
            tr = (start[0] + delta[0] - delta[1], start[1] + delta[1] + delta[0])
        # the 0.05 skip: |o_l - o_j| is the same number for (l, j) and (j, l); compared once per pair
        skip = set()
        for l in range(M):
            for j in range(l + 1, M):
                dr, di = O[l][0] - O[j][0], O[l][1] - O[j][1]
                if abs(dr) > 1 or abs(di) > 1:   # separated beyond doubt; recorded with its margin all the same
                    rec.records.append(("2d skip", (l, j), 1.0 - SKIP_DIST / float(max(abs(dr), abs(di))), None, False, False))
                    continue
                lt, _ = rec.compare("2d skip", (l, j), _norm2(dr, di), mpf(SKIP_DIST),
                                    lambda: (_norm2(O[l][0] - O[j][0], O[l][1] - O[j][1]), mpf(SKIP_DIST)))
                if lt:
                    skip.add((l, j))
        if mutate[0] == "flip_skip":
            skip ^= {(min(mutate[1:]), max(mutate[1:]))}
        A, absP = [], []
        for l in range(M):
            ol = mpc(*O[l])
            den = mpc(1)
            for j in range(M):
                if j != l and (min(l, j), max(l, j)) not in skip:
                    den *= ol - mpc(*O[j])
            Al = mpf(float(prescaler)) * a * (ol - mpc(*bl)) * b * (ol - mpc(*tr)) / den
            if mutate[0] == "exponent" and mutate[1] == l:
                Al *= 2
            A.append(Al); absP.append(1 / abs(den))
        last = n - 1 - (1 if mutate[0] == "drop_last_segment" else 0)
        H, S, L, skipped, selections = mpc(0), mpf(0), [], [], {}
        consts = [mpf(0), mpf(TWO_PI), -mpf(TWO_PI), mpf(FOUR_PI), -mpf(FOUR_PI)]
        for l in range(M):
            logd, arg, arg64, axis = [], [], [], []
            for i in range(n):
                re, im = Z[i][0] - O[l][0], Z[i][1] - O[l][1]
                d = _norm2(re, im)
                rec.compare("2d diff == 0", (band, i, l), d, mpf(0), None)
                if d == 0:
                    logd.append(None); arg.append(None); arg64.append(None); axis.append(True)
                    continue
                logd.append(mpmath.log(d))
                if im == 0:   # atan2(+-0, x): the sign of the zero is that of the fp64 subtraction, which is exact
                    neg = bool(np.signbit(np.float64(y[i]) - np.float64(oy[l])))
                    th = mpf(0) if re > 0 else (-mpmath.pi if neg else +mpmath.pi)
                else:
                    th = mpmath.atan2(im, re)
                arg.append(th); arg64.append(mpf(float(th))); axis.append(bool(re == 0 or im == 0))
            Ll, Sl = mpc(0), mpf(0)
            for i in range(last):
                if logd[i] is None or logd[i + 1] is None:
                    skipped.append((i, l))
                    continue
                a1, a2 = arg64[i], arg64[i + 1]
                props = [(a2 - a1) + c for c in consts]
                win = 0
                for q in range(1, 5):
                    if abs(props[q]) < abs(props[win]):
                        win = q
                for q in range(5):
                    if q != win:
                        rec.compare("2d proposal", (band, i, l, q), abs(props[win]), abs(props[q]),
                                    lambda q=q: (abs((a2 - a1) + consts[win]), abs((a2 - a1) + consts[q])),
                                    extra_ok=axis[i] and axis[i + 1])
                selections[(i, l)] = win
                log_imag = (arg[i + 1] - arg[i]) + consts[win]
                if mutate[0] == "unwrap" and mutate[1] == l and mutate[2] == i:
                    log_imag += consts[1]
                Ll += mpc(logd[i + 1] - logd[i], log_imag)
                Sl += abs(logd[i + 1]) + abs(logd[i]) + abs(arg[i + 1]) + abs(arg[i])
            L.append(Ll)
            S += abs(A[l]) * Sl
            if not (mutate[0] == "drop_term" and mutate[1] == l):
                H += A[l] * Ll
        return dict(H=H, S=S, A=A, absA=[abs(v) for v in A], absP=absP, L=L, a=a, b=b, small_map=bool(small), skipped_pairs=sorted(skip),
                    skipped_segments=skipped, selections=selections)


# ---- 3-D ------------------------------------------------------------------------------------------------------------------------------
def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _sq(a):
    return a[0] * a[0] + a[1] * a[1] + a[2] * a[2]


def signature_3d(ox, oy, vx, vy, x, y, dt, rec, band=0, mutate=None):
    """dict(H [M] mpf or None (not finite), T [M] mpf, skipped: the segments below 1e-15, not_finite {l: (segment, step)}).
    mutate: ("drop_step", segment, step)."""
    mutate = mutate or ("none",)
    M, n = len(ox), len(x)
    with mpmath.workdps(DPS):
        four_pi = 4 * mpf(math.pi)
        Z = [(mpf(float(x[i])), mpf(float(y[i]))) for i in range(n)]
        t = [mpf(0)]
        for i in range(n - 1):
            t.append(t[-1] + mpf(float(dt[i])))
        segs, skipped = [], []
        def direction(i):
            return (Z[i + 1][0] - Z[i][0], Z[i + 1][1] - Z[i][1], mpf(float(dt[i])))
        for i in range(n - 1):
            d = direction(i)
            lt, _ = rec.compare("3d coincident", (band, i), mpmath.sqrt(_sq(d)), mpf(COINCIDENT),
                                lambda i=i: (mpmath.sqrt(_sq(direction(i))), mpf(COINCIDENT)))
            if lt:
                skipped.append(i)
            else:
                segs.append((i, d, tuple(c / STEPS for c in d)))
        H, T, bad = [], [], {}
        for l in range(M):
            s1 = (mpf(float(ox[l])), mpf(float(oy[l])), mpf(0))
            s2 = (s1[0] + CONDUCTOR_T * mpf(float(vx[l])), s1[1] + CONDUCTOR_T * mpf(float(vy[l])), mpf(CONDUCTOR_T))
            ds = tuple(s2[q] - s1[q] for q in range(3))
            dsq = _sq(ds)
            Hl, Tl = mpf(0), mpf(0)
            for i, d, dl in segs:
                for k in range(STEPS):
                    if mutate[0] == "drop_step" and mutate[1] == i and mutate[2] == k:
                        continue
                    r = (Z[i][0] + k * dl[0], Z[i][1] + k * dl[1], t[i] + k * dl[2])
                    p1 = tuple(s1[q] - r[q] for q in range(3))
                    p2 = tuple(s2[q] - r[q] for q in range(3))
                    dd = tuple(c / dsq for c in _cross(ds, _cross(p1, p2)))
                    n1, n2, nd = mpmath.sqrt(_sq(p1)), mpmath.sqrt(_sq(p2)), mpmath.sqrt(_sq(dd))
                    # the distance of the integration point from the conductor (and its end points) against 0: exactly on it, or clear
                    # of it by REL of its distance from the conductor's start
                    scale = max(n1, mpf(1))
                    for what, v in (("3d |d| == 0", nd), ("3d |p1| == 0", n1), ("3d |p2| == 0", n2)):
                        if v != 0 and v < REL * scale:
                            raise InadmissibleError("%s band %d obstacle %d segment %d step %d: %s of %s" % (what, band, l, i, k, mpmath.nstr(v, 5), mpmath.nstr(scale, 5)))
                    if k == 0 or nd == 0:
                        rec.records.append(("3d |d| == 0", (band, l, i, k), float(nd / scale) if nd != 0 else 0.0, True if nd == 0 else None, False, bool(nd == 0)))
                    if nd == 0 or n1 == 0 or n2 == 0:
                        bad.setdefault(l, (i, k))
                        continue
                    c2, c1 = _cross(dd, p2), _cross(dd, p1)
                    f = 1 / _sq(dd)
                    for q in range(3):
                        term = (c2[q] / n2 - c1[q] / n1) * f * dl[q]
                        Hl += term
                        Tl += abs(term)
            H.append(None if l in bad else Hl / four_pi)
            T.append(Tl / four_pi)
        return dict(H=H, T=T, skipped=skipped, not_finite=bad)


# ---- the class decisions ----------------------------------------------------------------------------------------------------------------
def class_decisions(mode, sig, scale, threshold, best, max_plans, rec, tag=""):
    """mode 2: sig [B] mpc, scale [B] mpf (S); mode 3: sig [B][M] mpf or None, scale [B][M] (T_l). threshold: fp64. best: band index or -1
    (no class remembered from an earlier call). Returns (keep, valid, reasonable) [B] int32 as filter_equivalence_classes does, and
    records every comparison with its margin in units of the guard (>= 1, else InadmissibleError)."""
    B = len(sig)
    with mpmath.workdps(DPS):
        thr = mpf(float(threshold))
        guard = CLASS_GUARD * DEVICE_CAP * EPS

        def decide(what, idx, a, b, allowed):
            """a against b, |a - b| must exceed `allowed` (the error the operands may carry)"""
            margin = abs(a - b)
            if not margin > allowed:
                raise InadmissibleError("%s %s %s: |%s - %s| = %s does not exceed the allowed error %s" %
                                        (tag, what, idx, mpmath.nstr(a, 17), mpmath.nstr(b, 17), mpmath.nstr(margin, 5), mpmath.nstr(allowed, 5)))
            rec.records.append(("class " + what, idx, float(margin / allowed) if allowed != 0 else float("inf"), None, bool(a < b), False))
            return a < b

        valid = [int(all(v is not None for v in sig[b])) if mode == 3 else 1 for b in range(B)]
        reas = []
        for b in range(B):
            ok = 1
            if mode == 3:
                for l, v in enumerate(sig[b]):   # value > 1.0 (a comparison with a NaN is false: a band that is not valid is "reasonable")
                    if v is not None and not decide("H_l > 1", (b, l), v, mpf(1), guard * scale[b][l]) and v > 1:
                        ok = 0
            reas.append(ok)

        def rows_equal(p, q):
            if mode == 2:
                for part, name in ((lambda z: z.real, "|dRe| <= thr"), (lambda z: z.imag, "|dIm| <= thr")):
                    d = abs(part(sig[q]) - part(sig[p]))
                    if not decide(name, (p, q), d, thr, guard * (scale[p] + scale[q])) and d > thr:
                        return False
                return True
            for l in range(len(sig[p])):
                far = False
                for r in (q, p):
                    if decide("|H_l| < thr", (r, l), abs(sig[r][l]), thr, guard * scale[r][l]):
                        far = True
                        break
                if far:
                    continue
                if (sig[p][l] > 0) != (sig[q][l] > 0):   # |H_l| >= thr > the allowed error: the sign is decided
                    return False
            return True

        order = list(range(B))
        has_best = 0 <= best < B
        if has_best:
            order[0], order[best] = order[best], order[0]
        classes, keep = [], [0] * B
        for b in order:
            if not valid[b]:
                continue
            has = any(rows_equal(b, c) for c in classes)
            if has:
                in_best = has_best and rows_equal(order[0], b)
                count = sum(1 for c in classes if rows_equal(order[0], c)) if has_best else 0
                if not in_best or count >= max_plans:
                    continue
            classes.append(b); keep[b] = 1
    return np.array(keep, np.int32), np.array(valid, np.int32), np.array(reas, np.int32)


# ---- exact values as doubles -------------------------------------------------------------------------------------------------------------
def split(v):
    """an 80-digit value as (hi, lo): hi the nearest double, lo the nearest double of the rest - the next 53 bits"""
    if v is None:
        return float("nan"), 0.0
    hi = float(v)
    return hi, float(v - mpf(hi))


def mant_exp(v):
    """a non-negative 80-digit value that may lie outside the fp64 range, as (m, e): v = m 2^e, 0.5 <= m < 1 (0, 0 for 0)"""
    if v == 0:
        return 0.0, 0
    m, e = mpmath.frexp(v)
    return float(m), int(e)


# ---- the comparison the GPU test uses (no mpmath) ---------------------------------------------------------------------------------------
def _units(d, m, e):
    if d == 0:
        return 0.0
    if m == 0 or not math.isfinite(d):
        return float("inf")
    try:
        return math.ldexp(d / (EPS * m), -int(e))
    except OverflowError:
        return float("inf")


def error_2d(got, exact, S):
    """got [2] (re, im); exact [2, 2]: (hi, lo) of re and im; S (m, e). max(|dRe|, |dIm|) / (eps S); inf when got is not finite"""
    d = max(abs((float(got[q]) - float(exact[q][0])) - float(exact[q][1])) for q in range(2))
    if not all(math.isfinite(float(g)) for g in got):
        return float("inf")
    return _units(d, float(S[0]), int(S[1]))


def error_3d(got, exact, T):
    """got [M]; exact [M, 2] (hi = nan: not finite); T [M]. (largest |d| / (eps T_l) over the finite obstacles, finite pattern equal)"""
    got, exact, T = np.asarray(got, np.float64), np.asarray(exact, np.float64), np.asarray(T, np.float64)
    fin = np.isfinite(exact[:, 0]) if len(exact) else np.zeros(0, bool)
    same = bool((np.isfinite(got) == fin).all())
    worst = 0.0
    for l in np.flatnonzero(fin & np.isfinite(got)):
        worst = max(worst, _units(abs((got[l] - exact[l, 0]) - exact[l, 1]), T[l], 0))
    return worst, same


def device_bound(oracle_error):
    return max(FLOOR, FACTOR * float(oracle_error))


def accepts(error, oracle_error, same_pattern=True):
    """what the GPU test asserts of a value"""
    return bool(same_pattern and error <= device_bound(oracle_error))
