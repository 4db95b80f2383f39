"""The net under the pre-built instantiations of the optimise kernel (tests/test_gpu_every_instantiation.py) against the build
(teb_local_planner_amd/build.py), on the CPU: the tool's EXPECTED is what the product builds, every case on a specialised kind has a generic
twin, and every unit built with the cheap call of the solve (no -DTEB_AMD_SOLVE_CSR in UNIT_FLAGS) is the expected instantiation of a case
with a twin - so a new kind, or a unit moved off the plain convention, cannot get past the GPU test unseen."""
import importlib.util
import os
import re

import pytest

from teb_local_planner_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "launch_every_instantiation.py")


@pytest.fixture(scope="module")
def tool():
    spec = importlib.util.spec_from_file_location("launch_every_instantiation", TOOL)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _product_units():
    """{(layout, Jacobian mode, kind): object name} of the product's optimise-kernel units"""
    units = {}
    for obj, src, defs in build._units("product"):
        m = re.fullmatch(r"opt_(\d+)_(\d+)_(\d+)\.o", obj)
        if m:
            assert src == "teb_opt_inst.hip" and not any(d == "-DTEB_INST_STUB" for d in defs), (obj, defs)
            units[tuple(int(g) for g in m.groups())] = obj
    return units


def test_expected_is_what_the_product_builds(tool):
    units = _product_units()
    assert set(units) == tool.EXPECTED, ("built, not expected: %s" % sorted(set(units) - tool.EXPECTED),
                                         "expected, not built: %s" % sorted(tool.EXPECTED - set(units)))


@pytest.mark.parametrize("layout", ["band", "blocks", "bandg"])
def test_cases_of_the_layout_are_well_formed(tool, layout):
    """Labels unique; twins exactly on the specialised kinds; a helper pair is the same scene without helpers on the full-batch kind of
    its size class; distance helpers only on single-band scenes (the multi-band defect of the distance helpers)."""
    cases = tool.cases(layout)
    labels = [c.label for c in cases]
    assert len(set(labels)) == len(labels)
    by_label = dict(zip(labels, cases))
    for c in cases:
        jm, kind = c.expected
        assert (tool.LAYOUTS[layout], jm, kind) in tool.EXPECTED, c.label
        assert c.twin == (kind >= 4), "%s: kind %d, twin %s" % (c.label, kind, c.twin)
        assert not c.opts.get("generic_config_path") or kind < 4, c.label
        if c.opts.get("multi_cu", 0) > 0:
            assert c.batch.count == 1, "%s: distance helpers on %d bands" % (c.label, c.batch.count)
        if c.pair is not None:
            p = by_label[c.pair]
            assert p.pair is None and p.opts["multi_cu"] == -1 and p.opts["speculative_trials"] == -1, c.label
            assert {k: v for k, v in c.opts.items() if k not in ("multi_cu", "speculative_trials")} == \
                   {k: v for k, v in p.opts.items() if k not in ("multi_cu", "speculative_trials")}, c.label
            assert bytes(c.cfg.to_c()) == bytes(p.cfg.to_c()), c.label
            assert c.via == p.via and c.batch.count == p.batch.count and c.batch.stride == p.batch.stride, c.label
            for f in ("n", "x", "y", "theta", "dt", "via_points_enabled"):
                assert (getattr(c.batch, f) == getattr(p.batch, f)).all(), (c.label, f)
            assert p.expected == (jm, {2: 0, 3: 1, 5: 4, 7: 6, 9: 8, 11: 10}[kind]), (c.label, p.expected)


def test_every_unit_on_the_cheap_call_is_compared_with_its_generic_twin(tool):
    units = _product_units()
    cheap = sorted(k for k, obj in units.items() if "-DTEB_AMD_SOLVE_CSR" not in build.UNIT_FLAGS.get(obj, []))
    assert cheap, "no unit on the no-callee-saved call: the premise of this test is gone"
    twinned = set()
    for layout, lay in tool.LAYOUTS.items():
        twinned |= {(lay,) + tuple(c.expected) for c in tool.cases(layout) if c.twin}
    for k in cheap:
        assert k[2] in tool.TWIN_KIND, "%s (%s) is on the cheap call but no specialised kind" % (k, units[k])
        # the twin's unit is on the plain convention (what the oracle parity of the generic kinds vouches for)
        twin_obj = units[(k[0], k[1], tool.TWIN_KIND[k[2]])]
        assert "-DTEB_AMD_SOLVE_CSR" in build.UNIT_FLAGS.get(twin_obj, []), (k, twin_obj)
    assert not [k for k in cheap if k not in twinned], "units on the cheap call no case compares with a generic twin: %s" % \
        [units[k] for k in cheap if k not in twinned]
