"""Exact reference of the DECISIONS of the band producers and read-outs: which samples a band gets, which are
inserted, what is pruned, where the look-ahead ends, which sign and which branch a velocity takes. NOT a test file.

It restates, as plain loops and line by line from the reference planner,
  TimedElasticBand::initTrajectoryToGoal(start, goal, diststep, ...)   src/timed_elastic_band.cpp:325-386      -> Strip.init_line
  ... the plan overload with estimateDeltaT                            src/timed_elastic_band.cpp:389-452, 52-65 -> Strip.init_plan
  ... the template overload                  include/teb_local_planner/timed_elastic_band.hpp:46-183          -> Strip.init_path
  PoseSE2::average                           include/teb_local_planner/pose_se2.h:266-269                     -> Strip.average
  TimedElasticBand::updateAndPruneTEB        src/timed_elastic_band.cpp:555-597                               -> Strip.prune
  TebOptimalPlanner::extractVelocity / getVelocityCommand / getVelocityProfile / getFullTrajectory
                                             src/optimal_planner.cpp:1097-1133, 1135-1168, 1170-1196, 1198-1247
  g2o::normalize_theta, g2o::sign, g2o::average_angle                  g2o/stuff/misc.h
The loops are written ONCE over a number type and run in two ways (the scheme of tests/hp_feasibility.py / tests/hp_explore_graph.py):
  mode "float": every operation of the reference is one Python float operation;
  mode "both":  every value carries its fp64 evaluation AND its evaluation with mpmath at DPS digits on the same fp64 inputs, the
                magnitude it would have had without cancellation, and a flag `t`: a libm result (sin / cos / atan2) fed this value.
Every comparison is recorded: (kind, class, relative margin, outcome, tie in fp64, sign of a - b in fp64, site, libm-fed). The kinds
are KINDS (the table of the issue: back, steps_floor, steps_drop, fill, vel_gt0, theta_gt0, dt_max, acc, ts_le0, avg_zero, look, near,
la_clamp, la_time, dt_le0, dt_eq0, dir_sign, holo and the five branches of every normalize_theta call); the sites are SITES, the
function the comparison stands in. The classes:
  SEPARATED  relative margin >= REL = 1e-9: any fp64 evaluation with any correct libm decides alike; fp64 must agree with 80 digits;
  EXACT      the fp64 operands equal their 80-digit values: a tie or one ulp is then legitimate; or the two operands tie in BOTH
             evaluations (the same operations on mirrored inputs, as for two poses at one distance);
  RUNG       the case names the kind in its `rungs`, the kind is one of RUNG_KINDS (+ - * / sqrt floor only) and NO libm result feeds
             an operand: the expectation is the op-by-op fp64 outcome, which a build without contraction reproduces bit for bit.
Anything else raises InadmissibleError; no comparison and no case is ever dropped. LIBM_KINDS always pass through libm; dt_max and the
norm_* / fix_* kinds do where a yaw was estimated - the flag `t` says so per comparison - and none of these can be a RUNG.

Two places where the reference itself has no defined answer: getFullTrajectory of a band of ONE pose reads TimeDiff(0) of an empty
sequence (:1218), so Strip.full_trajectory refuses n == 1 (the profile of one pose is defined: start and goal velocity); and the template
overload with a path of one point runs its iterators past each other, so Strip.init_path wants two points.

The run also counts EVENTS (self.events) and `mut` names one deliberate error (MUTATIONS); the CPU test shows which cases notice each.
"""
import collections
import math

import numpy as np

from hp_explore_graph import DPS, REL, SEPARATED, EXACT, RUNG, Dual, InadmissibleError, _dual, _f, _fdiv  # noqa: F401

try:
    import mpmath
    from mpmath import mpf
except ImportError:   # the GPU test reads fixtures only
    mpmath, mpf = None, None

KINDS = ["back", "steps_floor", "steps_drop", "fill", "vel_gt0", "theta_gt0", "dt_max", "acc", "ts_le0", "avg_zero", "look", "near", "la_clamp",
         "la_time", "dt_le0", "dt_eq0", "dir_sign", "holo", "norm_lo", "norm_hi", "norm_floor", "fix_hi", "fix_lo"]
KIND_ID = {k: i for i, k in enumerate(KINDS)}
SITES = ["line", "plan", "path", "prune", "cmd", "profile", "traj"]
SITE_ID = {s: i for i, s in enumerate(SITES)}
LIBM_KINDS = ("back", "dir_sign", "avg_zero")
RUNG_KINDS = ("steps_floor", "steps_drop", "near", "la_time", "acc")   # steps_drop compares the quotient steps_floor floors
LANES = 256        # TEB_AMD_THREADS of csrc/teb_device.hpp (checked in the CPU test)
PI = math.pi

MUTATIONS = {
    "back_le": "'<=' for '<' in the backwards test",
    "steps_round": "the quotient rounded to the nearest integer, not floored",
    "steps_no_drop": "the last sample kept where it coincides with the goal",
    "drop_double": "no_steps_d compared with (double) no_steps, not through float",
    "fill_le": "'<=' for '<' against min_samples - 1",
    "tail_timestep_kept": "line overload: timestep not recomputed for an inserted pose",
    "halve_after": "template overload: timestep halved after the insert",
    "dt_min": "std::min for std::max in estimateDeltaT",
    "acc_le": "'<=' for '<' between timestep_vel and timestep_acc",
    "ts_lt0": "'<' for '<=' in timestep <= 0",
    "path_prev_from_band": "the difference taken to the previous PATH point, not to Pose(idx) of the band",
    "look_11": "the nearest-pose search looks 11 poses ahead",
    "look_no_min_samples": "the nearest-pose search ignores min_samples",
    "near_le": "'<=' for '<' in the nearest-pose search",
    "near_no_break": "the nearest-pose search goes on past the first pose that is not nearer",
    "shift_dt_off_by_one": "deleteTimeDiffs(0, k) for deleteTimeDiffs(1, k)",
    "goal_before_prune": "the new goal written before the poses are deleted",
    "goal_at_old_index": "the new goal written to index n - 1 of the band before the poses were deleted",
    "la_no_lower_clamp": "the look-ahead not clamped to 1 from below",
    "la_prevent_ignored": "prevent_look_ahead_poses_near_goal ignored",
    "la_time_gt": "'>' for '>=' in the time cut",
    "la_time_fixed_count": "the time cut against dt_ref * (counter + 1), not dt_ref * look_ahead_poses",
    "dt_lt0": "'<' for '<=' in dt <= 0",
    "sign_pm": "sign(0) = +1",
    "holo_eps": "|max_vel_y| < 1e-9 for max_vel_y == 0",
    "omega_unnormalised": "omega from the raw angle difference",
    "traj_end_mean": "the last trajectory point averaged like a middle one, not given the goal velocity",
    "profile_n": "a profile of n entries: the goal velocity missing",
    "time_pairwise": "time stamps as one correctly rounded sum each, not summed left to right",
}
# Four of these cannot change any answer; the CPU test asserts that NO case notices them and says why:
#   drop_double: (float) no_steps == (double) no_steps for every no_steps < 2^24, and a band holds fewer than 2^10 poses;
#   path_prev_from_band: Pose(idx) holds path point idx bit for bit (positions are copied, never computed), and a refused band leaves
#     nothing behind that a later call reads;
#   acc_le: '<' and '<=' part only where timestep_vel == timestep_acc, and then either branch assigns that one value;
#   goal_before_prune: the poses are deleted from index 1 on and the last pose survives (k <= n - min_samples <= n - 2: with min_samples 1
#     the reference asserts in deleteTimeDiffs), so the goal written first ends on index n - k - 1 all the same. goal_at_old_index is the
#     error that shows.
EQUIVALENT = ("drop_double", "path_prev_from_band", "acc_le", "goal_before_prune")
_OPS = {"<": lambda a, b: a < b, "<=": lambda a, b: a <= b, ">": lambda a, b: a > b, ">=": lambda a, b: a >= b, "==": lambda a, b: a == b}


class T(Dual):
    """Dual with t: a libm result fed this value"""
    __slots__ = ("t",)

    def __init__(self, f, m=None, s=None, t=False):
        Dual.__init__(self, f, m, s)
        self.t = t

    def _w(a, r, b):
        return T(r.f, r.m, r.s, a.t or getattr(b, "t", False))

    def __add__(a, b):
        return a._w(Dual.__add__(a, b), b)
    __radd__ = __add__

    def __sub__(a, b):
        return a._w(Dual.__sub__(a, b), b)

    def __rsub__(a, b):
        return T(float(b)) - a

    def __mul__(a, b):
        return a._w(Dual.__mul__(a, b), b)
    __rmul__ = __mul__

    def __truediv__(a, b):
        return a._w(Dual.__truediv__(a, b), b)

    def __rtruediv__(a, b):
        return T(float(b)) / a

    def __neg__(a):
        return T(-a.f, -a.m, a.s, a.t)


class Refused(Exception):
    """the band needs more poses than the handle holds: TEB_AMD_ERR_CAPACITY, pose count 0"""


class Strip:
    def __init__(self, rungs=(), mode="both", mut=None):
        assert mode in ("both", "float") and (mut is None or mut in MUTATIONS)
        self.hp, self.mut, self.rungs = mode == "both", mut, set(rungs)
        self.records = []
        self.events = collections.Counter()

    def run(self, fn, *args, **kw):
        if self.hp:
            with mpmath.workdps(DPS):
                return fn(self, *args, **kw)
        return fn(self, *args, **kw)

    # ---- numbers
    def num(self, x):
        if isinstance(x, T):
            return x
        return T(float(x)) if self.hp else float(x)

    def div(self, a, b):
        return self.num(a) / self.num(b) if self.hp else _fdiv(a, b)

    def sqrt(self, x):
        if not self.hp:
            return math.sqrt(x)
        return T(math.sqrt(x.f), mpmath.sqrt(x.m), mpmath.sqrt(x.s), x.t)

    def fabs(self, x):
        return T(abs(x.f), abs(x.m), x.s, x.t) if self.hp else abs(x)

    def libm(self, name, *args):
        if not self.hp:
            return getattr(math, name)(*args)
        m = getattr(mpmath, name)(*[a.m for a in args])
        return T(getattr(math, name)(*[a.f for a in args]), m, abs(m) if name == "atan2" else max(abs(m), mpf(1)), True)

    def norm(self, dx, dy):
        """Eigen's Vector2d::norm(): sqrt(x * x + y * y)"""
        return self.sqrt(dx * dx + dy * dy)

    # ---- the recorded comparisons
    def _classify(self, kind, rel, exact, agree, libm, what):
        if rel >= REL:
            if not agree:
                raise InadmissibleError("%s: separated by %.3g and fp64 decides differently (%s)" % (kind, rel, what))
            return SEPARATED
        if exact:
            assert agree
            return EXACT
        if kind in self.rungs and kind in RUNG_KINDS and not libm:
            return RUNG
        raise InadmissibleError("%s: relative margin %.3g < %g, operands not exact in fp64, %s (%s)"
                                % (kind, rel, REL, "libm feeds it" if libm else "no rung declared", what))

    def cmp(self, kind, site, a, op, b, rf=None):
        af, bf = _f(a), _f(b)
        if rf is None:
            rf = _OPS[op](af, bf)
        if not self.hp:
            return rf
        a, b = self.num(a), self.num(b)
        libm = a.t or b.t or kind in LIBM_KINDS
        scale = max(a.s, b.s)
        rel = float(abs(a.m - b.m) / scale) if scale != 0 else 0.0
        cls = self._classify(kind, rel, (mpf(af) == a.m and mpf(bf) == b.m) or (af == bf and a.m == b.m), rf == _OPS[op](a.m, b.m), libm, "%r %s %r" % (af, op, bf))
        self.records.append((KIND_ID[kind], cls, rel, bool(rf), af == bf, (af > bf) - (af < bf), SITE_ID[site], libm))
        return rf

    def int_cmp(self, kind, site, a, b, outcome):
        if self.hp:
            self.records.append((KIND_ID[kind], EXACT, 0.0 if a == b else abs(a - b) / max(abs(a), abs(b)), bool(outcome), a == b, (a > b) - (a < b),
                                 SITE_ID[site], False))
        return outcome

    def floor(self, kind, site, q):
        """floor(q), recorded as the distance of q from the nearest integer; outcome: the fp64 floor differs from the exact one"""
        f = _f(q)
        r = int(math.floor(f))
        if self.hp:
            rel = float(abs(q.m - mpmath.nint(q.m)) / max(q.s, mpf(1)))
            rm = int(mpmath.floor(q.m))
            cls = self._classify(kind, rel, mpf(f) == q.m, r == rm, q.t, "%r, exactly %s" % (f, mpmath.nstr(q.m, 25)))
            self.records.append((KIND_ID[kind], cls, rel, r != rm, f == math.floor(f), (mpf(f) > q.m) - (mpf(f) < q.m), SITE_ID[site], q.t))
        return r

    # ---- g2o/stuff/misc.h
    def normalize_theta(self, site, theta):
        lo, hi = self.cmp("norm_lo", site, theta, ">=", -PI), self.cmp("norm_hi", site, theta, "<", PI)
        if lo and hi:
            return theta
        multiplier = self.floor("norm_floor", site, self.div(theta, 2 * PI))
        theta = theta - self.num(float(multiplier)) * 2 * PI
        if self.cmp("fix_hi", site, theta, ">=", PI):
            theta = theta - 2 * PI
        if self.cmp("fix_lo", site, theta, "<", -PI):
            theta = theta + 2 * PI
        return theta

    def sign(self, site, x):
        """g2o::sign as a number; the decision is admissible (the restatement raised otherwise), so the result is no libm value"""
        if self.mut == "sign_pm":
            return self.num(1.0 if _f(x) >= 0 else -1.0)
        if self.cmp("dir_sign", site, x, ">", 0.0):
            return self.num(1.0)
        if self.cmp("dir_sign", site, x, "<", 0.0):
            return self.num(-1.0)
        return self.num(0.0)

    def average(self, site, p, q):
        """PoseSE2::average(p, q) with g2o::average_angle"""
        two = self.num(2.0)
        ax, ay = self.div(p[0] + q[0], two), self.div(p[1] + q[1], two)
        x = self.libm("cos", p[2]) + self.libm("cos", q[2])
        y = self.libm("sin", p[2]) + self.libm("sin", q[2])
        if self.cmp("avg_zero", site, self.div(self.norm(x, y), two), "==", 0.0, rf=(_f(x) == 0 and _f(y) == 0)):
            return ax, ay, self.num(0.0)
        return ax, ay, self.libm("atan2", y, x)

    def _backwards(self, site, guess, px, py, theta):
        """guess_backwards_motion && point_to_goal.dot(orientationUnitVec()) < 0"""
        if not guess:
            return False
        return self.cmp("back", site, px * self.libm("cos", theta) + py * self.libm("sin", theta), "<=" if self.mut == "back_le" else "<", 0.0)

    def _fill(self, site, n, min_samples):
        return self.int_cmp("fill", site, n, min_samples - 1, n <= min_samples - 1 if self.mut == "fill_le" else n < min_samples - 1)

    def _cap(self, band, cap, where):
        if cap is not None and len(band[0]) + 1 > cap:
            self.events["refuse:" + where] += 1
            raise Refused(where)

    @staticmethod
    def _push(band, x, y, th, dt):
        band[0].append(x); band[1].append(y); band[2].append(th); band[3].append(dt)

    # ---- src/timed_elastic_band.cpp:325-386
    def init_line(self, start, goal, diststep, max_vel_x, min_samples, guess_backwards_motion, cap=None):
        N = self.num
        sx, sy, sth = (N(v) for v in start)
        g = tuple(N(v) for v in goal)
        band = ([sx], [sy], [sth], [])
        timestep = N(0.1)
        if diststep != 0:
            px, py = g[0] - sx, g[1] - sy
            dir_to_goal = self.libm("atan2", py, px)
            dx, dy = N(diststep) * self.libm("cos", dir_to_goal), N(diststep) * self.libm("sin", dir_to_goal)
            orient_init = dir_to_goal
            if self._backwards("line", guess_backwards_motion, px, py, sth):
                orient_init = self.normalize_theta("line", orient_init + PI)
            no_steps_d = self.div(self.norm(px, py), self.fabs(N(diststep)))
            no_steps = self.floor("steps_floor", "line", no_steps_d)
            if self.mut == "steps_round":
                no_steps = int(math.floor(_f(no_steps_d) + 0.5))
            if self.cmp("vel_gt0", "line", max_vel_x, ">", 0.0):
                timestep = self.div(N(diststep), N(max_vel_x))
            for i in range(1, no_steps + 1):
                if i == no_steps:
                    as_float = float(no_steps) if self.mut == "drop_double" else float(np.float32(no_steps))
                    if self.cmp("steps_drop", "line", no_steps_d, "==", as_float) and self.mut != "steps_no_drop":
                        self.events["drop"] += 1
                        break
                self._cap(band, cap, "sample")
                self._push(band, sx + N(float(i)) * dx, sy + N(float(i)) * dy, orient_init, timestep)
        if self._fill("line", len(band[0]), min_samples):
            while self._fill("line", len(band[0]), min_samples):
                back = (band[0][-1], band[1][-1], band[2][-1])
                ax, ay, ath = self.average("line", back, g)
                if self.cmp("vel_gt0", "line", max_vel_x, ">", 0.0) and self.mut != "tail_timestep_kept":
                    timestep = self.div(self.norm(ax - back[0], ay - back[1]), N(max_vel_x))
                self._cap(band, cap, "insert")
                self._push(band, ax, ay, ath, timestep)
                self.events["insert:line"] += 1
        if self.cmp("vel_gt0", "line", max_vel_x, ">", 0.0):
            timestep = self.div(self.norm(g[0] - band[0][-1], g[1] - band[1][-1]), N(max_vel_x))
        self._cap(band, cap, "goal")
        self._push(band, g[0], g[1], g[2], timestep)
        return band

    # ---- src/timed_elastic_band.cpp:52-65
    def estimate_delta_t(self, site, s, e, max_vel_x, max_vel_theta):
        dt = self.num(0.1)
        if self.cmp("vel_gt0", site, max_vel_x, ">", 0.0):
            dt = self.div(self.norm(e[0] - s[0], e[1] - s[1]), self.num(max_vel_x))
        if self.cmp("theta_gt0", site, max_vel_theta, ">", 0.0):
            rot = self.div(self.fabs(self.normalize_theta(site, e[2] - s[2])), self.num(max_vel_theta))
            less = self.cmp("dt_max", site, dt, "<", rot)
            dt = (dt if less else rot) if self.mut == "dt_min" else (rot if less else dt)
        return dt

    # ---- src/timed_elastic_band.cpp:389-452
    def init_plan(self, px, py, pyaw, max_vel_x, max_vel_theta, estimate_orient, min_samples, guess_backwards_motion, cap=None):
        N = self.num
        n = len(px)
        start = (N(px[0]), N(py[0]), N(pyaw[0]))
        g = (N(px[-1]), N(py[-1]), N(pyaw[-1]))
        band = ([start[0]], [start[1]], [start[2]], [])
        backwards = self._backwards("plan", guess_backwards_motion, g[0] - start[0], g[1] - start[1], start[2])
        for i in range(1, n - 1):
            if estimate_orient:
                yaw = self.libm("atan2", N(py[i + 1]) - N(py[i]), N(px[i + 1]) - N(px[i]))
                if backwards:
                    yaw = self.normalize_theta("plan", yaw + PI)
            else:
                yaw = N(pyaw[i])
            pose = (N(px[i]), N(py[i]), yaw)
            dt = self.estimate_delta_t("plan", (band[0][-1], band[1][-1], band[2][-1]), pose, max_vel_x, max_vel_theta)
            self._cap(band, cap, "sample")
            self._push(band, *pose, dt)
        if self._fill("plan", len(band[0]), min_samples):
            while self._fill("plan", len(band[0]), min_samples):
                back = (band[0][-1], band[1][-1], band[2][-1])
                pose = self.average("plan", back, g)
                dt = self.estimate_delta_t("plan", back, pose, max_vel_x, max_vel_theta)
                self._cap(band, cap, "insert")
                self._push(band, *pose, dt)
                self.events["insert:plan"] += 1
        dt = self.estimate_delta_t("plan", (band[0][-1], band[1][-1], band[2][-1]), g, max_vel_x, max_vel_theta)
        self._cap(band, cap, "goal")
        self._push(band, *g, dt)
        return band

    # ---- include/teb_local_planner/timed_elastic_band.hpp:46-183
    def _path_timestep(self, site, diff_norm, max_vel_x, max_acc_x):
        timestep_vel = self.div(diff_norm, self.num(max_vel_x))
        if max_acc_x is not None:
            timestep_acc = self.sqrt(self.div(self.num(2.0) * diff_norm, self.num(max_acc_x)))
            if self.cmp("acc", site, timestep_vel, "<=" if self.mut == "acc_le" else "<", timestep_acc):
                return timestep_acc
        return timestep_vel

    def init_path(self, px, py, max_vel_x, max_vel_theta, max_acc_x, start_orientation, goal_orientation, min_samples, guess_backwards_motion,
                  cap=None):
        N = self.num
        n = len(px)
        assert n >= 2
        sx, sy, gx, gy = N(px[0]), N(py[0]), N(px[-1]), N(py[-1])
        backwards = False
        if start_orientation is not None:
            start_orient = N(start_orientation)
            backwards = self._backwards("path", guess_backwards_motion, gx - sx, gy - sy, start_orient)
        else:
            start_orient = self.libm("atan2", gy - sy, gx - sx)
        goal_orient = N(goal_orientation) if goal_orientation is not None else start_orient
        band = ([sx], [sy], [start_orient], [])
        idx = 0
        for k in range(1, n - 1):
            cx, cy = N(px[k]), N(py[k])
            if self.mut == "path_prev_from_band":
                dlx, dly = cx - N(px[k - 1]), cy - N(py[k - 1])
            else:
                dlx, dly = cx - band[0][idx], cy - band[1][idx]
            timestep = self._path_timestep("path", self.norm(dlx, dly), max_vel_x, max_acc_x)
            if self.cmp("ts_le0", "path", timestep, "<" if self.mut == "ts_lt0" else "<=", 0.0):
                timestep = N(0.2)
            yaw = self.libm("atan2", dly, dlx)
            if backwards:
                yaw = self.normalize_theta("path", yaw + PI)
            self._cap(band, cap, "sample")
            self._push(band, cx, cy, yaw, timestep)
            idx += 1
        timestep = self._path_timestep("path", self.norm(gx - band[0][idx], gy - band[1][idx]), max_vel_x, max_acc_x)
        g = (gx, gy, goal_orient)
        if self._fill("path", len(band[0]), min_samples):
            while self._fill("path", len(band[0]), min_samples):
                if self.mut != "halve_after":
                    timestep = self.div(timestep, N(2.0))
                self._cap(band, cap, "insert")
                self._push(band, *self.average("path", (band[0][-1], band[1][-1], band[2][-1]), g), timestep)
                if self.mut == "halve_after":
                    timestep = self.div(timestep, N(2.0))
                self.events["insert:path"] += 1
        self._cap(band, cap, "goal")
        self._push(band, *g, timestep)
        return band

    # ---- src/timed_elastic_band.cpp:555-597
    def prune(self, x, y, th, dt, new_start, new_goal, min_samples):
        """the band after updateAndPruneTEB; only poses [0, n) and time differences [0, n - 1) are read"""
        N = self.num
        X, Y, TH, DT = [N(v) for v in x], [N(v) for v in y], [N(v) for v in th], [N(v) for v in dt[:max(len(x) - 1, 0)]]
        n = len(X)
        if self.mut == "goal_before_prune" and new_goal is not None and n > 0:
            X[-1], Y[-1], TH[-1] = (N(v) for v in new_goal)
        if new_start is not None and n > 0:
            s = [N(v) for v in new_start]
            dist_cache = self.norm(s[0] - X[0], s[1] - Y[0])
            avail = n - 1 if self.mut == "look_no_min_samples" else n - min_samples
            limit = 11 if self.mut == "look_11" else 10
            lookahead = avail if self.int_cmp("look", "prune", avail, limit, avail < limit) else limit
            lookahead = min(lookahead, n - 1)   # (only a mutation can ask beyond the band)
            nearest_idx = 0
            for i in range(1, lookahead + 1):
                dist = self.norm(s[0] - X[i], s[1] - Y[i])
                if self.cmp("near", "prune", dist, "<=" if self.mut == "near_le" else "<", dist_cache):
                    dist_cache, nearest_idx = dist, i
                elif self.mut == "near_no_break":
                    continue
                else:
                    self.events["prune:break"] += 1
                    break
            if lookahead >= 1 and nearest_idx == lookahead:
                self.events["prune:nearest_at_limit"] += 1
            if nearest_idx > 0:
                k = nearest_idx
                del X[1:1 + k], Y[1:1 + k], TH[1:1 + k]
                if self.mut == "shift_dt_off_by_one":
                    del DT[0:k]
                else:
                    del DT[1:1 + k]
                self.events["prune:%s" % ("to_min_samples" if len(X) == min_samples else "some")] += 1
            else:
                self.events["prune:none"] += 1
            X[0], Y[0], TH[0] = s
        if new_goal is not None and len(X) > 0 and self.mut not in ("goal_before_prune", "goal_at_old_index"):
            X[-1], Y[-1], TH[-1] = (N(v) for v in new_goal)
        if new_goal is not None and self.mut == "goal_at_old_index" and len(X) == n > 0:   # (beyond the new count it is lost)
            X[-1], Y[-1], TH[-1] = (N(v) for v in new_goal)
        return X, Y, TH, DT

    # ---- src/optimal_planner.cpp:1097-1133
    def extract_velocity(self, site, max_vel_y, p1, p2, dt):
        N = self.num
        if self.cmp("dt_eq0", site, dt, "==", 0.0):
            return N(0.0), N(0.0), N(0.0)
        dx, dy = p2[0] - p1[0], p2[1] - p1[1]
        holo = abs(max_vel_y) < 1e-9 if self.mut == "holo_eps" else self.cmp("holo", site, max_vel_y, "==", 0.0)
        if holo:
            direction = dx * self.libm("cos", p1[2]) + dy * self.libm("sin", p1[2])
            vx = self.div(self.sign(site, direction) * self.norm(dx, dy), dt)
            vy = N(0.0)
        else:
            cos_theta1, sin_theta1 = self.libm("cos", p1[2]), self.libm("sin", p1[2])
            p1_dx = cos_theta1 * dx + sin_theta1 * dy
            p1_dy = -sin_theta1 * dx + cos_theta1 * dy
            vx, vy = self.div(p1_dx, dt), self.div(p1_dy, dt)
        diff = p2[2] - p1[2]
        orientdiff = diff if self.mut == "omega_unnormalised" else self.normalize_theta(site, diff)
        return vx, vy, self.div(orientdiff, dt)

    def _poses(self, x, y, th):
        return [(self.num(a), self.num(b), self.num(c)) for a, b, c in zip(x, y, th)]

    # ---- src/optimal_planner.cpp:1135-1168
    def velocity_command(self, x, y, th, dt, max_vel_y, dt_ref, look_ahead_poses, prevent):
        """(ok, vx, vy, omega)"""
        N = self.num
        P = self._poses(x, y, th)
        n = len(P)
        zero = (False, N(0.0), N(0.0), N(0.0))
        if n < 2:
            return zero
        lim = n - 1 - (0 if self.mut == "la_prevent_ignored" else prevent)
        la = look_ahead_poses
        if self.int_cmp("la_clamp", "cmd", la, lim, lim < la):
            la = lim
            self.events["la:clamped_above"] += 1
        if self.int_cmp("la_clamp", "cmd", la, 1, la < 1) and self.mut != "la_no_lower_clamp":
            la = 1
            self.events["la:clamped_below"] += 1
        t = N(0.0)
        for counter in range(la):
            t = t + N(dt[counter])
            against = N(dt_ref) * N(float(counter + 1 if self.mut == "la_time_fixed_count" else la))
            if self.cmp("la_time", "cmd", t, ">" if self.mut == "la_time_gt" else ">=", against):
                if counter + 1 < la:
                    self.events["la:cut_by_time"] += 1
                la = counter + 1
                break
        if self.cmp("dt_le0", "cmd", t, "<" if self.mut == "dt_lt0" else "<=", 0.0):
            return zero
        return (True,) + self.extract_velocity("cmd", max_vel_y, P[0], P[la], t)

    # ---- src/optimal_planner.cpp:1170-1196
    def velocity_profile(self, x, y, th, dt, max_vel_y, vel_start, vel_goal):
        """[n + 1] rows (vx, vy, omega)"""
        N = self.num
        P = self._poses(x, y, th)
        n = len(P)
        out = [tuple(N(v) for v in vel_start)]
        for i in range(1, n):
            out.append(self.extract_velocity("profile", max_vel_y, P[i - 1], P[i], N(dt[i - 1])))
        if self.mut != "profile_n":
            out.append(tuple(N(v) for v in vel_goal))
        return out

    # ---- src/optimal_planner.cpp:1198-1247
    def full_trajectory(self, x, y, th, dt, max_vel_y, vel_start, vel_goal):
        """[n] rows (x, y, theta, vx, vy, omega, time_from_start)"""
        N = self.num
        P = self._poses(x, y, th)
        n = len(P)
        if n == 0:
            return []
        if n == 1:
            raise ValueError("getFullTrajectory of one pose reads TimeDiff(0) of an empty sequence")
        half = N(0.5)
        curr_time = N(0.0)
        out = [P[0] + tuple(N(v) for v in vel_start) + (curr_time,)]
        curr_time = curr_time + N(dt[0])
        for i in range(1, n - 1):
            v1 = self.extract_velocity("traj", max_vel_y, P[i - 1], P[i], N(dt[i - 1]))
            v2 = self.extract_velocity("traj", max_vel_y, P[i], P[i + 1], N(dt[i]))
            out.append(P[i] + tuple(half * (a + b) for a, b in zip(v1, v2)) + (curr_time,))
            curr_time = curr_time + N(dt[i])
        vel = tuple(N(v) for v in vel_goal)
        if self.mut == "traj_end_mean":
            v1 = self.extract_velocity("traj", max_vel_y, P[n - 2], P[n - 1], N(dt[n - 2]))
            vel = tuple(half * (a + b) for a, b in zip(v1, vel))
        out.append(P[n - 1] + vel + (curr_time,))
        if self.mut == "time_pairwise":
            out = [row[:6] + (N(math.fsum(float(v) for v in dt[:i])),) for i, row in enumerate(out)]
        return out

    def record_array(self):
        return np.array(self.records, np.float64).reshape(-1, 8)


# ---- numbers out of a run -------------------------------------------------------------------------------------------------------------------
def values(a):
    """fp64 values of a (nested) sequence of numbers as an array"""
    return np.array([[_f(v) for v in row] if isinstance(row, (tuple, list)) else _f(row) for row in a], np.float64)


def exact_mask(a):
    """True where no libm result fed the value (mode "both")"""
    return np.array([[not v.t for v in row] if isinstance(row, (tuple, list)) else not row.t for row in a], bool)


def worst_error(a):
    """(the largest |fp64 - 80 digits| over the values a libm result fed, the largest magnitude of all)"""
    err, mag = 0.0, 0.0
    for row in a:
        for v in (row if isinstance(row, (tuple, list)) else (row,)):
            mag = max(mag, abs(v.f))
            if v.t:
                err = max(err, float(abs(mpf(v.f) - v.m)))
    return err, mag


def summary(rec):
    """[len(KINDS), 8] per kind: comparisons, SEPARATED, EXACT, RUNG, ties in fp64, outcome true, outcome false, the smallest separated
    margin (inf: none)"""
    out = np.zeros((len(KINDS), 8))
    out[:, 7] = np.inf
    for k in range(len(KINDS)):
        r = rec[rec[:, 0] == k]
        sep = r[r[:, 1] == SEPARATED]
        out[k, :7] = [len(r), len(sep), (r[:, 1] == EXACT).sum(), (r[:, 1] == RUNG).sum(), r[:, 4].sum(), (r[:, 3] == 1).sum(), (r[:, 3] == 0).sum()]
        if len(sep):
            out[k, 7] = sep[:, 2].min()
    return out


# ---- the fixture layout: per family one array per field, the cases one after the other -------------------------------------------------------
def pack(records):
    names = list(records)
    fields = sorted({f for n in names for f in records[n]})
    out = {"names": np.array(names)}
    for f in fields:
        parts = [np.ascontiguousarray(records[n].get(f, np.zeros(0))).ravel() for n in names]
        dtype = next((p.dtype for p in parts if len(p)), np.float64)
        out[f] = np.concatenate([p.astype(dtype) for p in parts])
        out[f + "_off"] = np.cumsum([0] + [len(q) for q in parts]).astype(np.int64)
    return out


def unpack(npz):
    """{case name: {field: flat array}}"""
    names = [str(n) for n in npz["names"]]
    fields = [f[:-4] for f in npz.files if f.endswith("_off")]
    return {n: {f: npz[f][npz[f + "_off"][k]:npz[f + "_off"][k + 1]] for f in fields} for k, n in enumerate(names)}
