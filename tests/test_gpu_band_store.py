"""The band store of a handle on the MI355X (csrc/teb_band_store.hpp: BandStrips, DevBandStore, BandAttrs, the packed messages).

(a) The same 18 bands of 12 poses through both upload paths - the packed message of small batches (max_poses 64) and the strided
    copies (max_poses = TEB_AMD_MAX_POSES: 18 x (11 + 4 x 944) doubles exceed the message buffer) - with every optional attribute array
    given for one upload and omitted for the next: pose counts, band flags, optimized flags and the downloaded bands of both handles
    equal the input, bit for bit, and so each other.
(b) One small handle (5 band slots, 12 poses, 4 obstacles) through upload, snapshot, a line band into slot 3 (slot 2 becomes the skipped
    band), a compaction that permutes and drops that band, an exploration, one optimise iteration and restore. After every step the counts, flags
    and bands and, once they exist, the results are compared bit for bit with tests/golden/band_store_sequence.npz: the same sequence
    recorded on the library of the commit before the band store existed (python tests/test_gpu_band_store.py --record FILE, with
    TEB_AMD_LIB naming that library). The test passes on either library.
No step provokes an error on the device."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

from teb_local_planner_amd import _abi, planner, scenes  # noqa: E402
from teb_local_planner_amd.config import TebConfig  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(HERE, "golden", "band_store_sequence.npz")
OPTIONAL = ("has_vel_start", "vel_start", "has_vel_goal", "vel_goal", "prefer_rotdir", "via_points_enabled")
MAX_POSES = 944   # TEB_AMD_MAX_POSES
PACK_DOUBLES = 65536


def _bands(count, poses, stride, seed):
    """`count` sine bands of `poses` poses with attributes off the defaults; the padding of the rows is marked"""
    rng = np.random.default_rng(seed)
    cfg = TebConfig()
    b = _abi.TebBatchHost(count, stride)
    for a in (b.x, b.y, b.theta, b.dt):
        a[:] = -99.0
    for k in range(count):
        b.set_teb(k, *scenes.sine_band(poses, 0.1 * (poses - 1), rng.uniform(-0.3, 0.3), float(rng.integers(1, 4)), cfg.robot.max_vel_x))
    b.has_vel_start[:] = rng.integers(0, 2, count); b.has_vel_goal[:] = rng.integers(0, 2, count)
    b.prefer_rotdir[:] = rng.integers(0, 3, count); b.via_points_enabled[:] = rng.integers(0, 2, count)
    b.vel_start[:] = rng.uniform(-0.3, 0.3, (count, 3)); b.vel_goal[:] = rng.uniform(-0.3, 0.3, (count, 3))
    return cfg, b


def _upload_without(s, batch, omitted):
    """teb_amd_upload_tebs with the optional arrays `omitted` passed as NULL"""
    bs = batch.c_struct()
    for name in omitted:
        setattr(bs, name, None)
    rc = planner.lib().teb_amd_upload_tebs(s._h, C.byref(bs))
    assert rc == 0, planner.lib().teb_amd_last_error()
    s.count = batch.count


def _same_bits(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), what


def test_packed_and_strided_upload_agree_with_the_input():
    B, n = 18, 12
    cfg, small_in = _bands(B, n, 64, seed=5)
    large_in = _abi.TebBatchHost(B, MAX_POSES)   # the same bands in rows of 944
    for k in ("x", "y", "theta", "dt"):
        getattr(large_in, k)[:] = -99.0
        getattr(large_in, k)[:, :64] = getattr(small_in, k)
    for k in ("n",) + OPTIONAL:
        getattr(large_in, k)[:] = getattr(small_in, k)
    assert 11 * B + 4 * B * 64 <= PACK_DOUBLES < 11 * B + 4 * B * MAX_POSES   # the packed path, the strided path
    small = planner.TebBatchSolver(cfg, B, 64, 4, 1, 1)
    large = planner.TebBatchSolver(cfg, B, MAX_POSES, 4, 1, 1)
    for omitted in [()] + [(name,) for name in OPTIONAL] + [OPTIONAL]:
        via = np.ones(B, np.int32) if "via_points_enabled" in omitted else small_in.via_points_enabled
        hvs = np.ones(B, np.int32) if "has_vel_start" in omitted else small_in.has_vel_start
        hvg = np.ones(B, np.int32) if "has_vel_goal" in omitted else small_in.has_vel_goal
        got = []
        for s, src in ((small, small_in), (large, large_in)):
            if s.count:
                s.set_optimized_flags(np.ones(B, np.int32))   # an upload resets them
            _upload_without(s, src, omitted)
            out = _abi.TebBatchHost(B, src.stride)
            s.download(out)
            got.append((s.pose_counts(), s.band_flags(), s.optimized_flags(), out))
            _same_bits(got[-1][0], src.n, "pose counts")
            for u, v, name in zip(got[-1][1], (via, hvs, hvg), ("via_points_enabled", "has_vel_start", "has_vel_goal")):
                _same_bits(u, v.astype(np.int32), name + " with %s omitted" % (omitted,))
            _same_bits(got[-1][2], np.zeros(B, np.int32), "optimized flags")
            _same_bits(out.n, src.n, "downloaded pose counts")
            for k in ("x", "y", "theta", "dt"):   # whole rows travel, padding included
                _same_bits(getattr(out, k), getattr(src, k), k)
        for k in range(B):   # ... and so the two handles agree
            for u, v in zip(got[0][3].get_teb(k), got[1][3].get_teb(k)):
                _same_bits(u, v, "band %d" % k)
    small.close()
    large.close()


# ---- (b) ------------------------------------------------------------------------------------------------------------------------------
def _state(s, results):
    """counts, flags, the poses of every band (never the padding of a row: it is whatever the allocation held) and, if asked for, results"""
    out = dict(n=s.pose_counts(), optimized=s.optimized_flags())
    out["via_en"], out["has_vs"], out["has_vg"] = s.band_flags()
    b = _abi.TebBatchHost(max(s.count, 1), 12)
    if s.count:
        s.download(b)
    out["bands"] = np.concatenate([np.concatenate(b.get_teb(k)) for k in range(s.count)]) if s.count else np.zeros(0)
    if results:
        r = s.results()
        out.update(status=r.status, lm_iterations=r.lm_iterations, lm_trials=r.lm_trials, chi2=r.chi2, cost=r.cost, lambda_=r.lambda_)
    return {k: np.ascontiguousarray(v).copy() for k, v in out.items()}


def run_sequence():
    """{step name: state}; the steps in order"""
    cfg, two = _bands(2, 8, 12, seed=11)
    two.has_vel_start[:] = 1; two.prefer_rotdir[:] = _abi.ROT_NONE   # (a free start velocity is an extension the optimiser never sees in a tick)
    cfg.hcp.simple_exploration = True
    t = _abi.ObstacleTable()
    t.add_point(0.3, 0.12); t.add_point(0.55, -0.1); t.add_point(-0.6, 0.4); t.add_point(1.6, -0.3, vel=(0.05, 0.0))
    s = planner.TebBatchSolver(cfg, 5, 12, 4, 1, 1)
    s.set_obstacles(t)
    start, goal = (0.0, 0.0, 0.0), (0.8, 0.0, 0.0)
    steps = {}
    s.upload(_bands(5, 8, 12, seed=12)[1])   # every slot written once: what the snapshot below holds beyond its two bands is defined
    s.upload(two)
    steps["1_upload"] = _state(s, False)
    s.snapshot()
    steps["2_snapshot"] = _state(s, False)
    s.init_trajectory_line(3, start, goal, 0.0, cfg.robot.max_vel_x, cfg.trajectory.min_samples)
    assert s.count == 4
    steps["3_line"] = _state(s, False)
    n_kept, new_best = s.compact_bands(np.array([1, 1, 0, 1], np.int32), 3)   # band 3 first, the skipped band leaves: 3, 0, 1
    assert (n_kept, new_best) == (3, 0)
    steps["4_compact"] = _state(s, False)
    r = s.explore_candidates(start, goal, dist_to_obst=0.2, start_vel=(0.1, 0.0, 0.02), free_goal_vel=True, best=0)
    assert 3 <= r["n_total"] <= 5
    steps["5_explore"] = _state(s, False)
    steps["5_explore"]["explored"] = np.array([r["n_total"], r["n_vertices"], r["n_paths"], r["initial_plan_teb"]], np.int32)
    s.optimize(1, 1)
    s.synchronize()
    steps["6_optimize"] = _state(s, True)
    s.restore()
    steps["7_restore"] = _state(s, True)   # (the strips of ALL slots come back: two bands of step 1, the others of the upload before it)
    s.close()
    return steps


def test_a_handle_through_every_band_set_matches_the_recorded_sequence():
    want = np.load(GOLDEN)
    steps = run_sequence()
    assert sorted("%s/%s" % (st, k) for st, d in steps.items() for k in d) == sorted(want.files)
    for st in sorted(steps):
        for k, v in steps[st].items():
            _same_bits(v, want["%s/%s" % (st, k)], "%s: %s" % (st, k))


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--record":
        np.savez(sys.argv[2], **{"%s/%s" % (st, k): v for st, d in run_sequence().items() for k, v in d.items()})
        print("recorded with library", planner.TebBatchSolver.build_info()[1])
    else:
        sys.exit("usage: test_gpu_band_store.py --record FILE.npz")
