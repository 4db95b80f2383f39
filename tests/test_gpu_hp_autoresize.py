"""The device's autoResize - autoresize_script_lane0, autoresize_chains, the script application (csrc/teb_kernel.hpp,
csrc/teb_autoresize_chain.hpp) - against the plain restatement of the reference's loop, sweep by sweep
(tests/test_hp_autoresize.py is the CPU side and describes the reference, the case families and the coverage conditions).

For every case of tests/autoresize_cases.py, in the host's own layout pick (default options) and with every layout pinned that holds the case's pose
capacity (last_instantiation() confirms it), the ladder cases through the defaults kernel (last_config_profile() == 1) and through
generic_config_path (== 0) as well: the band is uploaded with an empty obstacle table, weight_obstacle as in the defaults,
compute_cost off, and optimize(0, 1) is called - autoResize and the graph side data run, the LM loop is left at once (g2o's
optimize(0)), the strip is stored. In fast mode once per recorded sweep on the resident band, in full mode once. After each call:
  status TEB_FAILED (the band with the NaN time difference: TEB_NONFINITE), 0 LM iterations, overflow flags clear - or, where the sweep
  would leave more poses than the handle holds, bit 2 set and the band as it was before the sweep;
  n equal; dt, x, y BIT-equal; start and goal untouched; every heading of an input pose bit-equal; every new heading within
  max(256 eps, 16 x err_ref) rad of the 80-digit value of the fixture (256 eps: the project's floor for device arithmetic through libm,
  BOUND of tests/test_hp_linearize.py; 16 x the fp64 restatement's own error: two sincos and one atan2 per level of the split tree).
No mpmath and no oracle is needed here. No case and no pose is skipped.

Found with it on an MI355X: nothing - in every case, variant and call the device holds the restatement's band: n, dt, x, y and the input
headings bit for bit, status and overflow flags as named. Largest heading error of a new pose per family, in eps (bound 256): ladder
1.5, guards 3.0, chain limits 3.25, sizes 2.0, capacity 4.2, batch 2.75. The whole file (176 tests) takes 4.3 s; the slowest case 0.33 s
(the first launch of the process).
"""
import os
import sys
import time

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import hp_autoresize as HA  # noqa: E402
import autoresize_cases as AC  # noqa: E402
import make_hp_autoresize as MK  # noqa: E402

from teb_local_planner_amd import planner, scenes, _abi  # noqa: E402

pytestmark = pytest.mark.gpu

WORST = {}   # family -> largest heading error of a new pose seen so far (rad), printed by every case


def _config(c):
    cfg = scenes.TebConfig()
    t = cfg.trajectory
    t.teb_autosize, t.dt_ref, t.dt_hysteresis, t.min_samples, t.max_samples = True, c["dt_ref"], c["hyst"], c["min_samples"], c["max_samples"]
    cfg.obstacles.include_dynamic_obstacles = not c["fast"]   # TebOptimalPlanner::optimizeTEB: fast_mode = !include_dynamic_obstacles
    return cfg


def _batch(c):
    b = _abi.TebBatchHost(len(c["members"]), c["cap"])
    for j, m in enumerate(c["members"]):
        b.set_teb(j, m["x"], m["y"], m["theta"], m["dt"])
    return b


@pytest.mark.parametrize("name", AC.CASES)
def test_device_autoresize_against_the_restatement(name):
    c = AC.build(name)
    fx = MK.load(name)
    assert str(fx[name + "/hash"]) == MK.case_hash(c)
    cfg, batch = _config(c), _batch(c)
    own = AC.own_layout(c["cap"])
    faster = [L for L, _ in AC.LAYOUT_LIMITS][:[L for L, _ in AC.LAYOUT_LIMITS].index(own) + 1]
    worst, t0 = 0.0, time.perf_counter()
    for layout, generic, fixed in c["variants"]:
        # the host's own pick runs with the default options (helper workgroups where the host decides for them); a pinned layout runs one
        # workgroup per band, as in the other pins: what is compared is the layout's instantiation, not the helpers' protocol
        opt = (_abi.Options(generic_config_path=generic, fixed_layout=fixed) if layout == "auto" else
               _abi.Options(layout=layout, generic_config_path=generic, multi_cu=-1, speculative_trials=-1))
        s = planner.make_solver(cfg, _abi.ObstacleTable(), [], batch, options=opt)
        try:
            for call in range(c["calls"]):
                s.optimize(0, 1, compute_cost=False)
                res, got, flags = s.results(), s.download(batch.copy()), s.debug_overflow_flags()
                what = (name, layout, "generic" if generic else "defaults", "fixed" if fixed else "", "call %d" % call)
                ran = s.last_instantiation()
                if layout != "auto" or fixed:
                    assert ran[0] == AC.LAYOUT_INDEX[own if layout == "auto" else layout], (what, ran)
                else:
                    assert ran[0] in [AC.LAYOUT_INDEX[L] for L in faster], (what, ran)
                if name.startswith("capacity_outgrow") and call == 0:
                    assert ran[0] == AC.LAYOUT_INDEX[own], (what, ran)   # the optimistic launch was repeated in the handle's own layout
                if c["family"] == "ladder":
                    assert s.last_config_profile() == (0 if generic else 1), (what, s.last_config_profile())
                for j, m in enumerate(c["members"]):
                    want, over = MK.expected(fx, c, j, call)
                    assert res.status[j] == (_abi.TEB_NONFINITE if j == c["nan_member"] else _abi.TEB_FAILED), (what, j, res.status)
                    assert res.lm_iterations[j] == 0 and res.lm_trials[j] == 0, (what, j)
                    assert (flags[j] & 2) == (2 if over else 0) and (flags[j] & ~2) == 0, (what, j, flags)
                    n = int(got.n[j])
                    assert n <= c["cap"]
                    band = (got.x[j, :n], got.y[j, :n], got.theta[j, :n], got.dt[j, :max(n - 1, 0)])
                    bad, e = HA.check_band(band, want, ((m["x"][0], m["y"][0], m["theta"][0]), (m["x"][-1], m["y"][-1], m["theta"][-1])))
                    assert not bad, (what, j, bad)
                    worst = max(worst, e)
        finally:
            s.close()
    WORST[c["family"]] = max(WORST.get(c["family"], 0.0), worst)
    print("%s: %d variants, largest heading error of a new pose %.2f eps (family %s so far: %.2f eps), %.3f s" %
          (name, len(c["variants"]), worst / HA.EPS, c["family"], WORST[c["family"]] / HA.EPS, time.perf_counter() - t0))
