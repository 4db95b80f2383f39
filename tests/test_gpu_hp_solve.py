"""The product kernel's own LM step against the 60-digit reference of the damped solve (tests/test_hp_solve.py is the CPU side and
describes the reference, the metric, the bounds and the cases; tests/hp_solve.py, tests/hp_solve_cases.py).

No kernel and no entry point of its own: for every case (one band, one launch, one LM iteration, teb_autosize off)
  1. make_solver uploads the band with the layout pinned (and band_ldlt / speculative_trials where the case says so);
  2. debug_linearize(0, n, 1.0): the device's own H and b at that state (the generic instantiation in the same layout; the bit
     fingerprints hold every other instantiation to its bits) - last_instantiation() confirms the layout;
  3. set_iteration_log(True), upload again, optimize(inner = 1, outer = 1) - last_instantiation() again;
  4. the log row: damping trials k of the iteration, lambda after it;
  5. download: step = after - before exactly, +- ulp(after) / 2.
Asserted per case: the layout that ran, 1 <= k (>= 2 where the case is there for a rejected first trial: in the blocks layout the H
restore from the backup has run; with solver helpers the accepted step came from cr_solve_blocks_helper / cr_solve_hybrid_helper),
lambda after the iteration in [1/3, 2/3] lambda_k (an accepted trial, and the lambda_k reconstruction), max_i omega_i <= max(256 eps,
16 omega_cpu), forward error <= max(256 eps kappa, 16 fwd_cpu), omega_cpu / fwd_cpu from numpy.linalg.solve on the device's A and b.
No case is skipped. Solver helpers: last_launch_info() must report the helpers of the launch; whether each retry's step arrived from
its helper in time is the kernel's own decision (a late one is solved by the band's workgroup: same routine, same system), so a case
whose helpers were not used asserts what the one-CU path gives and says so in its output.

The matrix-core build (libteb_amd_mfma.so) runs the cr and band cases at n = 33 and 129 in a child interpreter, as
tests/test_gpu_mfma_build.py reaches it.

Largest observed on an MI355X, in eps (omega / forward error), per layout: blocks in LDS 2.3 / 3.6e3, hybrid 9.1 / 3.5e3, sequential
LDL^T 0.4 / 7.1e2, band in HBM 0.9 / 2.0e3, solver helpers (k = 4, both LDS layouts) 0.3 / 1.0e2, the matrix-core cases inside the
figures of their layouts; at most 0.036 of the omega bound (256 .. 2490 eps) and 2e-4 of the forward bound (kappa 7e2 .. 5.8e5). k was
1, 2, 3 and 5 as with the oracle, the noise share <= 43 eps, all helpers arrived. The whole file takes 6.4 s (2 s of it the child).
"""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import hp_solve_cases as SC  # noqa: E402
from test_hp_solve import run_check, assert_bounds, NOISE_SHARE, EPS  # noqa: E402

from teb_local_planner_amd import planner  # noqa: E402

pytestmark = pytest.mark.gpu

EXPECT_VARIANT = os.environ.get("TEB_HP_SOLVE_EXPECT_VARIANT")   # set by the matrix-build test below for its child


@pytest.mark.parametrize("name", list(SC.CASES))
def test_lm_step_against_the_reference(name):
    c = SC.build(name)
    cfg, obst, via, batch, n = c["cfg"], c["obst"], c["via"], c["batch"], c["n"]
    if EXPECT_VARIANT:
        assert EXPECT_VARIANT in planner.TebBatchSolver.build_info()[2]
    s = planner.make_solver(cfg, obst, via, batch, options=c["options"])
    G = s.debug_linearize(0, n, 1.0)
    assert s.last_instantiation()[0] == SC.LAYOUT_INDEX[c["layout"]], (c["layout"], s.last_instantiation())
    s.set_iteration_log(True)
    s.upload(batch)
    s.optimize(1, 1)
    ran, info = s.last_instantiation(), s.last_launch_info()
    log = s.iteration_log(0)
    after = s.download(batch.copy())
    s.close()
    assert ran[0] == SC.LAYOUT_INDEX[c["layout"]], (c["layout"], ran)
    assert len(log) == 1 and after.n[0] == n
    assert info[1] == c["helpers"], info
    if c["helpers"]:
        print("%s: %d solver helpers per band, launch repeated on one CU: %s" % (name, info[1], info[2]))
        if info[2]:
            print("%s: the helpers did not arrive in time - the step below is the one-CU path's" % name)
    F = run_check(name, c, G["H"], G["b"], log[0], after)
    if F["noise_share"] > NOISE_SHARE:   # a condition on the inputs, asserted on the CPU; here it only explains a miss
        print("%s: noise share %.1f eps" % (name, F["noise_share"] / EPS))
    assert_bounds(F)


MFMA_LIB = os.path.join(ROOT, "teb_local_planner_amd", "libteb_amd_mfma.so")
MFMA_CASES = ("cr_n33", "cr_n129", "band_n33", "band_n129")


def test_lm_step_of_the_matrix_core_build():
    assert os.path.exists(MFMA_LIB), "teb_local_planner_amd/libteb_amd_mfma.so is missing: __graft_entry__.build() builds it"
    env = dict(os.environ, TEB_AMD_LIB=MFMA_LIB, TEB_HP_SOLVE_EXPECT_VARIANT="TEB_AMD_MFMA_SCHUR",
               PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    ids = ["%s::test_lm_step_against_the_reference[%s]" % (os.path.abspath(__file__), name) for name in MFMA_CASES]
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-rP", "-m", "gpu"] + ids, env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    print(r.stdout[-4000:], r.stderr[-1000:])
    assert r.returncode == 0 and "%d passed" % len(MFMA_CASES) in r.stdout, r.stdout[-3000:]
