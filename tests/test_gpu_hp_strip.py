"""The band producers and read-outs of the device (init_line / init_plan / prune / consumers kernels of csrc/teb_strip.hpp, init_path_band
of csrc/teb_graph.hpp) against the fixtures of tests/golden/make_hp_strip.py: the op-by-op fp64 restatement of the reference's
initTrajectoryToGoal x3, updateAndPruneTEB, getVelocityCommand / getVelocityProfile / getFullTrajectory, checked at 80 digits, against
the reference planner's own functions and against the CPU oracle, on cases built ON the thresholds of every decision
(tests/strip_threshold_cases.py; what the cases cover is asserted on the CPU in tests/test_hp_strip.py).

This file reads only the fixtures. Per case: the pose count, the refusal with its error code (and pose count 0 where the kernel refuses),
the ok flag and every output that no libm result feeds are bit-equal; every other output is within 1e-12 (the restatement is within
1e-13 of its 80-digit value on these). Of a pruned band only poses [0, n) and time differences [0, n - 1) are compared. The fleets run
through update_and_prune(b = -1), update_and_prune_per_scene, update_and_prune_per_class and velocity_commands beside single-scene
handles, and must give what those give bit for bit.

Two inputs never reach a kernel and are asserted as such: a band of ONE pose cannot be uploaded (TEB_AMD_ERR_INVALID_ARG: a band needs
two poses; a producer never builds fewer), and a plan or path of more than max_poses + 1 points is refused before the launch. Bands with
time differences of 0 or below ARE uploaded and read out.

Observed on an MI355X: 194 tests in 1.9 s; the slowest case (0.34 s) is the first, which creates the first handle; the MAX_POSES
read-out, the largest launch, takes 0.02 s.
"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import hp_strip as HS  # noqa: E402  (unpack: no mpmath needed)

from teb_local_planner_amd import _abi, planner  # noqa: E402
from teb_local_planner_amd.config import TebConfig  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1e-12
FILES = ["line", "plan", "path", "prune", "cons", "lanes_build", "lanes_prune", "lanes_readout", "fleet"]
LINE, PLAN, PATH, PRUNE, CONS = range(5)
_FIX, _RAW, _SOLVERS = {}, {}, {}


def _file(stem):
    if stem not in _FIX:
        _RAW[stem] = np.load(os.path.join(HERE, "golden", "hp_strip_%s.npz" % stem))
        _FIX[stem] = HS.unpack(_RAW[stem])
    return _FIX[stem]


def _names():
    return [(stem, n) for stem in FILES for n in _file(stem)]


@pytest.fixture(scope="module", autouse=True)
def _close_the_handles():
    yield
    for s in _SOLVERS.values():
        s.close()
    _SOLVERS.clear()


def _config(max_vel_y=0.0, dt_ref=0.3, min_samples=3):
    cfg = TebConfig()
    cfg.robot.max_vel_y, cfg.trajectory.dt_ref, cfg.trajectory.min_samples = float(max_vel_y), float(dt_ref), int(min_samples)
    return cfg


def _solver(cap, max_vel_y=0.0, dt_ref=0.3):
    """one single-band handle per capacity and configuration, shared by the cases"""
    key = (int(cap), float(max_vel_y), float(dt_ref))
    if key not in _SOLVERS:
        _SOLVERS[key] = planner.TebBatchSolver(_config(max_vel_y, dt_ref), 1, int(cap), 1, 1, 1)
    return _SOLVERS[key]


def _opt(v):
    return None if np.isnan(v).any() else (float(v) if np.ndim(v) == 0 else [float(a) for a in v])


def _host(fxs, cap):
    batch = _abi.TebBatchHost(len(fxs), int(cap))
    for k, fx in enumerate(fxs):
        batch.set_teb(k, fx["in_x"], fx["in_y"], fx["in_th"], fx["in_dt"])
        if int(fx["op"][0]) == CONS:
            batch.vel_start[k], batch.vel_goal[k] = fx["fargs"][2:5], fx["fargs"][5:8]
    return batch


def _band(s, b, cap):
    out = _abi.TebBatchHost(s.count, int(cap))
    s.download(out)
    return dict(zip(("out_x", "out_y", "out_th", "out_dt"), out.get_teb(b)))


def _same(name, fx, got):
    """bit-equal where the fixture says exact, TOL elsewhere"""
    for key, g in got.items():
        want, ex = fx[key], fx["ex_" + key.replace("out_", "")]
        g = np.asarray(g, np.float64).ravel()
        assert g.shape == want.shape, (name, key, g.shape, want.shape)
        np.testing.assert_array_equal(g[ex], want[ex], err_msg="%s %s (exact entries)" % (name, key))
        worst = np.abs(g[~ex] - want[~ex]).max(initial=0.0)
        assert worst <= TOL, (name, key, worst)


def _refused(call, code):
    with pytest.raises(planner.TebAmdError) as e:
        call()
    assert e.value.code == code


def _produce(s, fx):
    op, f, i = int(fx["op"][0]), fx["fargs"], [int(v) for v in fx["iargs"]]
    if op == LINE:
        s.init_trajectory_line(0, f[0:3], f[3:6], float(f[6]), float(f[7]), i[0], bool(i[1]))
    elif op == PLAN:
        s.init_trajectory_plan(0, fx["in_x"], fx["in_y"], fx["in_th"], float(f[0]), float(f[1]), bool(i[0]), i[1], bool(i[2]))
    else:
        s.init_trajectory_path(0, fx["in_x"], fx["in_y"], float(f[0]), float(f[1]), _opt(f[2]), _opt(f[3]), _opt(f[4]), i[0], bool(i[1]))


def _readout(s, fx):
    look, prevent = (int(v) for v in fx["iargs"])
    ok, cmd = s.velocity_command(0, look, prevent)
    return ok, {"cmd": cmd, "profile": s.velocity_profile(0), "traj": s.full_trajectory(0)}


def _run_single(name, fx):
    """the case on its single-scene handle: asserts it against the fixture, returns what the device gave"""
    op, cap, status, n = int(fx["op"][0]), int(fx["cap"][0]), int(fx["status"][0]), int(fx["n"][0])
    if op in (LINE, PLAN, PATH):
        s = _solver(cap)
        if status != 0:
            _refused(lambda: _produce(s, fx), _abi.ERR_CAPACITY)
            if status == 1:   # the kernel refused: the band is gone
                assert s.pose_counts()[0] == 0, name
            return None
        _produce(s, fx)
        assert s.pose_counts()[0] == n, (name, s.pose_counts()[0], n)
        got = _band(s, 0, cap)
        _same(name, fx, got)
        return got
    if op == PRUNE:
        s = _solver(cap)
        ns, ng, ms = _opt(fx["fargs"][0:3]), _opt(fx["fargs"][3:6]), int(fx["iargs"][0])
        if len(fx["in_x"]) == 0:   # pose count 0 is what a refused producer leaves: the band stays as it is
            _refused(lambda: s.init_trajectory_line(0, [0.0, 0.0, 0.0], [10.125, 0.0, 0.0], 0.25, 0.5, 3, False), _abi.ERR_CAPACITY)
            assert cap == 16 and s.pose_counts()[0] == 0
            s.update_and_prune(ns, ng, ms, b=0)
            assert s.pose_counts()[0] == 0 == n, name
            return None
        s.upload(_host([fx], cap))
        s.update_and_prune(ns, ng, ms, b=0)
        assert s.pose_counts()[0] == n, (name, s.pose_counts()[0], n)
        got = _band(s, 0, cap)
        assert all(fx["ex_" + k].all() for k in ("x", "y", "th", "dt")), name      # pruning copies: nothing but bit-equal will do
        _same(name, fx, got)
        return got
    s = _solver(cap, fx["fargs"][0], fx["fargs"][1])
    if len(fx["in_x"]) < 2:
        _refused(lambda: s.upload(_host([fx], cap)), _abi.ERR_INVALID_ARG)
        return None
    s.upload(_host([fx], cap))
    ok, got = _readout(s, fx)
    assert ok == bool(fx["cmd"][3]), (name, ok)
    assert len(got["profile"]) == n + 1 and len(got["traj"]) == n, name
    _same(name, dict(fx, cmd=fx["cmd"][:3]), got)
    got["cmd"] = np.append(got["cmd"], float(ok))
    return got


@pytest.mark.parametrize("stem,name", _names())
def test_every_case_on_its_single_scene_handle(stem, name):
    _run_single(name, _file(stem)[name])


# ---- fleets --------------------------------------------------------------------------------------------------------------------------------------
def _fleet(fleet):
    fix = _file("fleet")
    raw = _RAW["fleet"]
    members = [str(m) for m in raw["fleet_" + fleet]]
    shared = {k[len("fleet_%s_" % fleet):]: raw[k] for k in raw.files if k.startswith("fleet_%s_" % fleet)}
    return members, [fix[m] for m in members], shared


def _fleet_solver(fxs, cfg, cfgs=None, class_of=None, scenes=True):
    cap = int(fxs[0]["cap"][0])
    s = planner.TebBatchSolver(cfg, len(fxs), cap, 4, 4, 4)
    if scenes:
        s.set_scenes([_abi.ObstacleTable() for _ in fxs])
        if cfgs is not None:
            s.set_scene_configs(cfgs, [int(c) for c in class_of])
        s.set_band_scenes(np.arange(len(fxs), dtype=np.int32))
    s.upload(_host(fxs, cap))
    return s, cap


def _pruned_like_the_members(s, cap, members, fxs):
    counts = s.pose_counts()
    for k, (name, fx) in enumerate(zip(members, fxs)):
        assert counts[k] == int(fx["n"][0]), (name, counts[k])
        got = _band(s, k, cap)
        _same(name, fx, got)
        one = _run_single(name, fx)
        for key in got:
            np.testing.assert_array_equal(got[key], one[key], err_msg="%s %s against the single-scene handle" % (name, key))


@pytest.mark.parametrize("fleet", ["all_bands", "per_scene", "per_class"])
def test_fleet_pruning_equals_the_fixture_and_the_single_scene_handles(fleet):
    members, fxs, shared = _fleet(fleet)
    starts = np.array([fx["fargs"][0:3] for fx in fxs])
    goals = np.array([fx["fargs"][3:6] for fx in fxs])
    if fleet == "all_bands":      # HomotopyClassPlanner::updateAllTEBs: one start and goal for every band of the handle
        assert (starts == starts[0]).all() and (goals == goals[0]).all() and len({int(fx["n"][0]) for fx in fxs}) > 1
        s, cap = _fleet_solver(fxs, _config(), scenes=False)
        s.update_and_prune(list(starts[0]), list(goals[0]), int(shared["min_samples"]))
    elif fleet == "per_scene":
        assert len({tuple(r) for r in starts}) == len(fxs)
        s, cap = _fleet_solver(fxs, _config())
        s.update_and_prune_per_scene(starts, goals, int(shared["min_samples"]))
    else:
        ms, of = [int(v) for v in shared["class_min_samples"]], [int(v) for v in shared["class_of_scene"]]
        assert [int(fx["iargs"][0]) for fx in fxs] == [ms[c] for c in of] and len(set(ms)) == 2
        s, cap = _fleet_solver(fxs, _config(min_samples=7), [_config(min_samples=m) for m in ms], of)
        s.update_and_prune_per_class(starts, goals)
    try:
        _pruned_like_the_members(s, cap, members, fxs)
    finally:
        s.close()


def test_fleet_commands_of_two_classes_in_one_launch():
    members, fxs, shared = _fleet("commands")
    vy, ref, of = shared["class_max_vel_y"], shared["class_dt_ref"], [int(v) for v in shared["class_of_scene"]]
    assert vy[0] == 0.0 and vy[1] != 0.0 and ref[0] != ref[1]
    for fx, c in zip(fxs, of):
        assert fx["fargs"][0] == vy[c] and fx["fargs"][1] == ref[c]
    look, prevent = int(shared["look"]), int(shared["prevent"])
    s, _ = _fleet_solver(fxs, _config(0.1, 1.0), [_config(a, b) for a, b in zip(vy, ref)], of)
    try:
        ok, cmd = s.velocity_commands(np.arange(len(fxs)), look, prevent)
    finally:
        s.close()
    for k, (name, fx) in enumerate(zip(members, fxs)):
        assert [int(v) for v in fx["iargs"]] == [look, prevent]
        assert bool(ok[k]) == bool(fx["cmd"][3]), name
        _same(name, dict(fx, cmd=fx["cmd"][:3]), {"cmd": cmd[k]})
        one = _run_single(name, fx)
        np.testing.assert_array_equal(np.append(cmd[k], float(ok[k])), one["cmd"], err_msg=name + " against the single-scene handle")
