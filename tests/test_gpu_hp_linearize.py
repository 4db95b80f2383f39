"""Every cost term's closed-form linearisation on the device against the high-precision reference (tests/test_hp_linearize.py is the
CPU side and describes the reference, the cases and the metric).

For every case of tests/hp_linearize_cases.py: planner.make_solver(...).debug_linearize(0, n, wm) in analytic mode with wm in {1, 2},
H, b and chi^2 against the fixture under tests/golden/ (no mpmath and no oracle needed here). Short cases run in the host's own layout
pick and with each of the three layouts pinned, long cases in their named layout (n = 300 band in LDS: the leftover pass with several
lanes per pose beyond 256; n = 238 blocks in LDS; n = 600 band in HBM); teb_amd_debug_last_instantiation confirms the layout that ran.
Bound per case: max(256 eps, 16 x the CPU oracle's error on that case) on H and b - the oracle's error is the fp64 noise floor of the
same closed forms, the factor 16 allows for the fused accumulation of Accum::row, the scatter order and a few ulp in the device's
sin / cos / sqrt; chi^2 per category relative (rows + 16) eps. No case and no entry is skipped.

Largest observed device error per family on an MI355X, in eps (H / b), over every layout and both multipliers: velocity 2.8 / 1.5,
acceleration 3.0 / 1.2, diff-drive 23 / 3.8, car-like 2.1 / 1.1, time-optimal 0 / 0, shortest path 1.3 / 0.1, prefer-rotdir 0 / 0.5,
via-points 1.5 / 0, static obstacles 194 / 13 (polygon footprint 215 / 53, bound 3435 / 840 there), dynamic obstacles 56 / 3.4,
velocity-obstacle ratio 2.2 / 1.1, legacy association 4.6 / 1.6, next to a kink 215 / 21, long bands: LDS band 48 / 1.1, blocks
14 / 0.8, HBM band 19 / 1.5. The whole file takes 4 s.
"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import hp_linearize as hp  # noqa: E402
import hp_linearize_cases as HC  # noqa: E402
import make_hp_linearize as MK  # noqa: E402
from test_hp_linearize import check_chi2, BOUND, EPS  # noqa: E402

from teb_local_planner_amd import planner, _abi  # noqa: E402

pytestmark = pytest.mark.gpu

@pytest.mark.parametrize("name", list(HC.CASES))
def test_device_closed_forms_against_the_reference(name):
    fx = MK.load(name)
    state = fx[name + "/state"]
    n = state.shape[1]
    c = HC.build(name, state=(state[0], state[1], state[2], state[3][:n - 1])) if HC.is_near(name) else HC.build(name)
    cfg, obst, via, batch = c["cfg"], c["obst"], c["via"], c["batch"]
    cfg.jacobian_mode = _abi.JACOBIAN_ANALYTIC
    assert int(batch.n[0]) == n
    for wm in c["wms"]:
        assert str(fx["%s/wm%g/scene" % (name, wm)]) == hp.input_hash(cfg, obst, via, batch, 0)
    for layout in c["layouts"]:
        s = planner.make_solver(cfg, obst, via, batch, options=None if layout == "auto" else _abi.Options(layout=layout))
        for wm in (1.0, 2.0):
            p = "%s/wm%g/" % (name, wm if wm in c["wms"] else 1.0)
            G = s.debug_linearize(0, n, wm)
            ran = s.last_instantiation()
            assert ran[1] == _abi.JACOBIAN_ANALYTIC
            if layout != "auto":
                assert ran[0] == HC.LAYOUT_INDEX[layout], (layout, ran)
            eH, eb = hp.errors(hp.band_of_dense(G["H"]), G["b"], fx[p + "Hband"], fx[p + "b"], fx[p + "chi2"])
            bound_H, bound_b = np.maximum(BOUND, 16 * fx[p + "oracle_err"])
            print("%s %s wm %g: H error %.1f eps (bound %.0f), b error %.1f eps (bound %.0f)" % (name, layout, wm, eH / EPS, bound_H / EPS, eb / EPS, bound_b / EPS))
            assert eH <= bound_H and eb <= bound_b, (layout, wm, eH / EPS, eb / EPS)
            check_chi2(G["chi2"], fx[p + "chi2"], fx[p + "rows"])
        s.close()
