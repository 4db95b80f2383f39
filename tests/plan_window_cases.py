"""The adapter arithmetic of TebLocalPlannerROS::computeVelocityCommands restated in plain Python floats, and the fixtures of the plan
window tests (tests/test_plan_windows.py holds the restatement to hand-worked answers, tests/test_gpu_plan_windows.py and
tests/test_gpu_fleet_adapter.py hold the device to the restatement).

The reference's adapter needs tf2 and costmap_2d and cannot be compiled here, so the yardstick is this sequential restatement, written
line by line from src/teb_local_planner_ros.cpp: pruneGlobalPlan :657-698, transformGlobalPlan :701-822, updateViaPointsContainer
:627-645, estimateLocalGoalOrientation :827-871, the start replacement :336-340, saturateVelocity :874-919,
convertTransRotVelToSteeringAngle :922-933. The expression order is the kernel contract of include/teb_amd.h: the robot in the plan
frame is R^T (g - t), a pose in the global frame R p + t, products and sums rounded one by one, x * x for pow(x, 2); a yaw is copied
when yaw_tf == 0 and g2o::normalize_theta(yaw + yaw_tf) otherwise. Every loop below is the reference's loop."""
import functools
import math

import numpy as np

from teb_local_planner_amd.config import normalize_theta

DEFAULTS = dict(global_plan_prune_distance=1.0, max_global_plan_lookahead_dist=1.0, global_plan_viapoint_sep=-1.0,
                global_plan_overwrite_orientation=True, moving_average_length=3)   # teb_config.h:261-264


def _to_global(tf, x, y, yaw):
    c, s, tx, ty, yaw_tf = tf
    return (c * x - s * y) + tx, (s * x + c * y) + ty, (yaw if yaw_tf == 0 else normalize_theta(yaw + yaw_tf))


def average_angles(angles):   # misc.h:72-84
    x = y = 0.0
    for a in angles:
        x += math.cos(a)
        y += math.sin(a)
    if x == 0 and y == 0:
        return 0.0
    return math.atan2(y, x)


def plan_window(plan, begin, pose, tf, dist_threshold, **params):
    """One robot's tick up to the call of plan(). plan = (x, y, yaw) lists in the plan frame, begin = what pruneGlobalPlan has erased
    so far, pose = (x, y, theta) in the global frame, tf = (cos, sin, tx, ty, yaw_tf) or None = identity. Returns a dict:
    window (x, y, yaw lists: transformed_plan as plan() gets it), goal_idx, cursor, pruned, vias [(x, y)], goal, global_goal,
    window_count, via_count; and resultant = hypot(sum cos, sum sin) of the moving average when that branch ran, else None."""
    p = dict(DEFAULTS, **params)
    tf = (1.0, 0.0, 0.0, 0.0, 0.0) if tf is None else tuple(float(v) for v in tf)
    c, s, tx, ty, _ = tf
    X = [float(v) for v in plan[0]][begin:]
    Y = [float(v) for v in plan[1]][begin:]
    YAW = [float(v) for v in plan[2]][begin:]
    out = dict(window=([], [], []), goal_idx=0, cursor=begin, pruned=1, vias=[], goal=(0.0, 0.0, 0.0), global_goal=(0.0, 0.0, 0.0),
               window_count=0, via_count=0, resultant=None)
    if not X:                                   # pruneGlobalPlan :659-660 returns true, transformGlobalPlan :713-718 fails with goal_idx 0
        return out
    gx, gy, gth = (float(v) for v in pose)
    ddx, ddy = gx - tx, gy - ty
    rx = c * ddx + s * ddy                      # the robot in the plan frame
    ry = c * ddy - s * ddx
    # pruneGlobalPlan :669-690
    dist_thresh_sq = p["global_plan_prune_distance"] * p["global_plan_prune_distance"]
    erase_end = None
    for it in range(len(X)):
        dx = rx - X[it]
        dy = ry - Y[it]
        if dx * dx + dy * dy < dist_thresh_sq:
            erase_end = it
            break
    if erase_end is None:
        out["pruned"] = 0
    else:
        X, Y, YAW = X[erase_end:], Y[erase_end:], YAW[erase_end:]
        out["cursor"] = begin + erase_end
    n = len(X)
    # transformGlobalPlan :735-757
    i = 0
    sq_dist_threshold = dist_threshold * dist_threshold
    sq_dist = 1e10
    robot_reached = False
    for j in range(n):
        x_diff = rx - X[j]
        y_diff = ry - Y[j]
        new_sq_dist = x_diff * x_diff + y_diff * y_diff
        if robot_reached and new_sq_dist > sq_dist:
            break
        if new_sq_dist < sq_dist:
            sq_dist = new_sq_dist
            i = j
            if sq_dist < 0.05:
                robot_reached = True
    # :761-780
    max_plan_length = p["max_global_plan_lookahead_dist"]
    plan_length = 0.0
    wx, wy, wyaw = [], [], []
    while i < n and sq_dist <= sq_dist_threshold and (max_plan_length <= 0 or plan_length <= max_plan_length):
        x, y, yaw = _to_global(tf, X[i], Y[i], YAW[i])
        wx.append(x); wy.append(y); wyaw.append(yaw)
        x_diff = rx - X[i]
        y_diff = ry - Y[i]
        sq_dist = x_diff * x_diff + y_diff * y_diff
        if i > 0 and max_plan_length > 0:
            ex = X[i] - X[i - 1]
            ey = Y[i] - Y[i - 1]
            plan_length += math.sqrt(ex * ex + ey * ey)
        i += 1
    # :784-797
    if not wx:
        x, y, yaw = _to_global(tf, X[-1], Y[-1], YAW[-1])
        wx.append(x); wy.append(y); wyaw.append(yaw)
        goal_idx = n - 1
    else:
        goal_idx = i - 1
    # updateViaPointsContainer :627-645
    vias = []
    sep = p["global_plan_viapoint_sep"]
    if sep > 0:
        prev = 0
        for k in range(1, len(wx)):
            ex = wx[k] - wx[prev]
            ey = wy[k] - wy[prev]
            if math.sqrt(ex * ex + ey * ey) < sep:
                continue
            vias.append((wx[k], wy[k]))
            prev = k
    # the goal-reached test's global goal :291-292
    global_goal = _to_global(tf, X[-1], Y[-1], YAW[-1])
    # :319-333, estimateLocalGoalOrientation :827-871
    goal_x, goal_y = wx[-1], wy[-1]
    if p["global_plan_overwrite_orientation"]:
        mal = int(p["moving_average_length"])
        if goal_idx > n - mal - 2:
            goal_yaw = wyaw[-1] if goal_idx >= n - 1 else global_goal[2]
        else:
            mal = min(mal, n - goal_idx - 1)
            candidates = []
            kx, ky = goal_x, goal_y
            range_end = goal_idx + mal
            for q in range(goal_idx, range_end):
                nx, ny, _ = _to_global(tf, X[q + 1], Y[q + 1], YAW[q + 1])
                candidates.append(math.atan2(ny - ky, nx - kx))
                if q < range_end - 1:
                    kx, ky = nx, ny
            goal_yaw = average_angles(candidates)
            out["resultant"] = math.hypot(sum(math.cos(a) for a in candidates), sum(math.sin(a) for a in candidates))
        wyaw[-1] = goal_yaw
    else:
        goal_yaw = wyaw[-1]
    # :336-340
    if len(wx) == 1:
        wx.insert(0, 0.0); wy.insert(0, 0.0); wyaw.insert(0, 0.0)
    wx[0], wy[0], wyaw[0] = gx, gy, gth
    out.update(window=(wx, wy, wyaw), goal_idx=goal_idx, vias=vias, goal=(goal_x, goal_y, goal_yaw), global_goal=global_goal,
               window_count=len(wx), via_count=len(vias))
    return out


def saturate_velocity(vx, vy, omega, max_vel_x, max_vel_y, max_vel_trans, max_vel_theta, max_vel_x_backwards,
                      use_proportional_saturation=False):
    """saturateVelocity :874-919 -> (vx, vy, omega)"""
    ratio_x = ratio_omega = ratio_y = 1.0
    if vx > max_vel_x:
        ratio_x = max_vel_x / vx
    if vy > max_vel_y or vy < -max_vel_y:
        ratio_y = abs(max_vel_y / vy)
    if omega > max_vel_theta or omega < -max_vel_theta:
        ratio_omega = abs(max_vel_theta / omega)
    if max_vel_x_backwards <= 0:
        pass                                    # the reference only warns
    elif vx < -max_vel_x_backwards:
        ratio_x = -max_vel_x_backwards / vx
    if use_proportional_saturation:
        ratio = min(min(ratio_x, ratio_y), ratio_omega)
        vx *= ratio
        vy *= ratio
        omega *= ratio
    else:
        vx *= ratio_x
        vy *= ratio_y
        omega *= ratio_omega
    vel_linear = math.hypot(vx, vy)
    if vel_linear > max_vel_trans:
        max_vel_trans_ratio = max_vel_trans / vel_linear
        vx *= max_vel_trans_ratio
        vy *= max_vel_trans_ratio
    return vx, vy, omega


def steering_angle(v, omega, wheelbase, min_turning_radius):
    """convertTransRotVelToSteeringAngle :922-933"""
    if omega == 0 or v == 0:
        return 0.0
    radius = v / omega
    if abs(radius) < min_turning_radius:
        radius = (1.0 if radius > 0 else (-1.0 if radius < 0 else 0.0)) * min_turning_radius   # g2o::sign
    if radius == 0:                             # v / omega underflowed: the reference divides by the signed zero, atan(+-inf)
        return math.copysign(math.pi / 2, wheelbase) * math.copysign(1.0, radius)
    return math.atan(wheelbase / radius)


# ---- fixtures -----------------------------------------------------------------------------------------------------------------------
class Case:
    """name, plan (x, y, yaw arrays), begin, pose, tf (5 doubles or None), thr, params (dict over DEFAULTS)"""

    def __init__(self, name, plan, pose, thr, begin=0, tf=None, **params):
        self.name, self.begin, self.pose, self.tf, self.thr, self.params = name, int(begin), tuple(float(v) for v in pose), tf, float(thr), params
        self.plan = tuple(np.asarray(a, np.float64) for a in plan)

    def restated(self):
        return plan_window(self.plan, self.begin, self.pose, self.tf, self.thr, **self.params)

    def abi_params(self):
        from teb_local_planner_amd import _abi
        return _abi.PlanWindowParams(**dict(DEFAULTS, **self.params))


def line(n, step, y=0.0):
    """n poses along +x, `step` apart (exactly representable), yaw 0.01 k"""
    k = np.arange(n, dtype=np.float64)
    return k * step, np.full(n, float(y)), 0.01 * k


def loop_plan(h):
    """Out along y = h through x = 0 (pose 4), a turn, back along y = -0.1 through x = 0 (pose 14): the robot at the origin meets the
    plan twice, the second time closer."""
    xs = [-1.0 + 0.25 * k for k in range(9)] + [1.25] + [1.0 - 0.25 * k for k in range(9)]
    ys = [h] * 9 + [0.0] + [-0.1] * 9
    return np.array(xs), np.array(ys), np.linspace(0.0, 0.9, 19)


def curve(n):
    """a gentle left turn with 0.25 m chords: headings differ, their resultant stays near its maximum"""
    th = 0.15 * np.arange(n)
    x = np.concatenate([[0.0], np.cumsum(0.25 * np.cos(th[:-1]))])
    y = np.concatenate([[0.0], np.cumsum(0.25 * np.sin(th[:-1]))])
    return x, y, th


def via_plan():
    """130 poses: 120 segments of 0.125, then 9 of 0.03125"""
    k = np.arange(130, dtype=np.float64)
    x = np.where(k <= 120, 0.125 * k, 15.0 + 0.03125 * (k - 120))
    return x, np.zeros(130), np.zeros(130)


def rigid(angle, tx, ty):
    return (math.cos(angle), math.sin(angle), float(tx), float(ty), float(angle))


NO_PRUNE = dict(global_plan_prune_distance=0.01)   # the robot rides 0.0625 beside the line: no pose within 0.01
NO_LENGTH = dict(max_global_plan_lookahead_dist=0.0)
# plans of 63 .. 513 poses; the closest pose T (the scan breaks at T + 1) on the last lane of a wave, of a chunk, the first of the next
CLOSEST = {63: (62,), 64: (62, 63), 65: (62, 63, 64), 255: (62, 254), 256: (254, 255), 257: (254, 255, 256), 513: (255, 256, 511, 512)}
PRUNE_AT = ((513, 63, 0), (513, 255, 0), (513, 256, 0), (513, 300, 0), (513, 258, 3), (257, 256, 0), (65, 64, 1))   # (poses, match, begin)
WINDOW_END = (63, 64, 255, 256, 257)               # the pose of the distance cut, window from pose 0


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    # tiny plans
    out.append(Case("empty", ([], [], []), (0.0, 0.0, 0.0), 1.0))
    out.append(Case("one_pose", line(1, 0.25), (0.0, 0.0625, 0.3), 1.0))
    out.append(Case("two_poses", line(2, 0.25), (0.0, 0.0625, 0.3), 1.0))
    out.append(Case("three_poses", line(3, 0.25), (0.25, 0.0625, 0.3), 1.0))
    out.append(Case("cursor_at_end", line(3, 0.25), (0.25, 0.0625, 0.3), 1.0, begin=3))
    out.append(Case("one_pose_window", line(5, 0.25), (0.5, 0.0625, 0.3), 1.0, max_global_plan_lookahead_dist=0.125, **NO_PRUNE))
    # the goal-yaw branches on 5 poses, moving_average_length 2: goal_idx = n - 1, n - 2, n - mal - 1 (the global goal's yaw), n - mal - 2
    # (the average); the distance cut sets goal_idx: the first pose farther than thr from the robot at pose 0
    for g, thr in ((4, 10.0), (3, 0.625), (2, 0.375), (1, 0.125)):
        out.append(Case("yaw_branch_5_%d" % g, curve(5), (0.0, 0.0, 0.1), thr, moving_average_length=2, **NO_LENGTH))
    out.append(Case("yaw_average_9", curve(9), (0.0, 0.0, 0.1), 0.375, **NO_LENGTH))                     # goal_idx 2 <= 9 - 3 - 2
    out.append(Case("yaw_average_9_edge", curve(9), (0.0, 0.0, 0.1), 0.875, **NO_LENGTH))                # goal_idx 4 = 9 - 3 - 2
    out.append(Case("yaw_global_9", curve(9), (0.0, 0.0, 0.1), 1.125, **NO_LENGTH))                      # goal_idx 5 = 9 - 3 - 1
    out.append(Case("yaw_kept", curve(9), (0.0, 0.0, 0.1), 0.375, global_plan_overwrite_orientation=False, **NO_LENGTH))
    # chunk boundaries
    for n, ts in CLOSEST.items():
        for t in ts:
            out.append(Case("closest_%d_%d" % (n, t), line(n, 0.125), (0.125 * t, 0.0625, 0.3), 0.5, **NO_PRUNE, **NO_LENGTH))
    for n, t, b in PRUNE_AT:
        out.append(Case("prune_%d_%d_%d" % (n, t, b), line(n, 0.125), (0.125 * t, 0.0625, 0.3), 0.5, begin=b,
                        global_plan_prune_distance=0.125, **NO_LENGTH))
    for c in WINDOW_END:
        out.append(Case("window_end_%d" % c, line(513, 0.125), (0.0, 0.0625, 0.3), 0.125 * c - 0.0625, **NO_LENGTH))
    out.append(Case("length_end_257", line(513, 0.25), (0.0, 0.0625, 0.3), 1000.0, max_global_plan_lookahead_dist=64.0))
    # ties, loops, nothing in reach
    out.append(Case("tie_wave_edge", line(130, 0.125, y=1.0), (0.125 * 63.5, 0.0, 0.0), 10.0, **NO_LENGTH))
    out.append(Case("tie_three", ([-0.5, 0.5, 1.5], [0.0, 0.0, 0.0], [0.1, 0.2, 0.3]), (0.0, 0.0, 0.0), 10.0, **NO_LENGTH))
    out.append(Case("loop_first_minimum", loop_plan(0.2), (0.0, 0.0, 0.0), 10.0, **NO_PRUNE, **NO_LENGTH))
    out.append(Case("loop_global_minimum", loop_plan(0.3), (0.0, 0.0, 0.0), 10.0, **NO_PRUNE, **NO_LENGTH))
    out.append(Case("beyond_threshold", line(40, 0.125), (100.0, 100.0, 1.0), 2.0))
    out.append(Case("farther_than_1e5", line(5, 0.25), (2.0e5, 0.0, 0.0), 1.0e6, **NO_LENGTH))
    # max_global_plan_lookahead_dist
    out.append(Case("length_equal_keeps", line(40, 0.25), (0.5, 0.0625, 0.3), 100.0, max_global_plan_lookahead_dist=1.0, **NO_PRUNE))
    out.append(Case("length_equal_from_0", line(40, 0.25), (0.0, 0.0625, 0.3), 100.0, max_global_plan_lookahead_dist=1.0))
    out.append(Case("length_off", line(40, 0.25), (0.5, 0.0625, 0.3), 1.0, max_global_plan_lookahead_dist=-1.0, **NO_PRUNE))
    # via-points
    out.append(Case("via_equal_sep", line(9, 0.25), (0.0, 0.0625, 0.3), 100.0, global_plan_viapoint_sep=0.25, **NO_LENGTH))
    for nv, sep in ((0, 100.0), (1, 15.28125), (40, 0.375)):   # 15.28125: exactly the last pose's distance from the first
        out.append(Case("via_130_%d" % nv, via_plan(), (0.0, 0.0, 0.0), 100.0, global_plan_viapoint_sep=sep, **NO_LENGTH))
    out.append(Case("via_off", line(9, 0.25), (0.0, 0.0625, 0.3), 100.0, global_plan_viapoint_sep=-1.0, **NO_LENGTH))
    # prune
    out.append(Case("prune_none", line(40, 0.125), (1.0, 2.0, 0.0), 10.0, **NO_LENGTH))                  # 2 m beside the line: prune distance 1
    out.append(Case("prune_at_cursor", line(40, 0.125), (0.5, 0.0625, 0.3), 1.0, begin=4, **NO_LENGTH))
    out.append(Case("prune_strict", line(40, 0.25), (0.0, 0.0, 0.0), 100.0, global_plan_prune_distance=0.0, **NO_LENGTH))
    out.append(Case("prune_strict_far", ([-3.0, -2.0, -1.0, -0.5, 0.0], [0.0] * 5, [0.0] * 5), (0.0, 0.0, 0.0), 100.0, **NO_LENGTH))
    # transform: a rotation by 0.7 rad and a translation; the robot's global pose belongs to the plan-frame point (1.0, 0.0625)
    tf = rigid(0.7, 3.5, -2.25)
    gx, gy, _ = _to_global(tf, 1.0, 0.0625, 0.0)
    out.append(Case("transform_rigid", curve(30), (gx, gy, 0.9), 1.0, tf=tf, global_plan_viapoint_sep=0.3,
                    max_global_plan_lookahead_dist=2.0))
    out.append(Case("transform_wraps_yaw", line(12, 0.25), _to_global(rigid(3.1, 1.0, 1.0), 0.5, 0.0, 0.0), 0.75, tf=rigid(3.1, 1.0, 1.0),
                    **NO_LENGTH))
    return tuple(out)


def case(name):
    return next(c for c in cases() if c.name == name)


def fleet_plans():
    """plans of 5 / 257 / 64 poses with poses, thresholds and one parameter set: three robots of one call"""
    tf = rigid(0.7, 3.5, -2.25)
    plans = [curve(5), line(257, 0.125), line(64, 0.125)]
    at = [(0.25, 0.0625), (0.125 * 255, 0.0625), (0.125 * 63, 0.0625)]
    poses = [_to_global(tf, x, y, 0.0)[:2] + (0.2 * r,) for r, (x, y) in enumerate(at)]
    tfs = [tf, tf, tf]
    thr = [1.0, 0.5, 0.75]
    params = dict(global_plan_viapoint_sep=0.25, max_global_plan_lookahead_dist=3.0)
    return plans, poses, tfs, thr, params
