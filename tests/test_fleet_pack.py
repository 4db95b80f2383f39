"""Fleet batches on the CPU: what teb_amd_set_scenes is handed (_abi.pack_scenes round trip and its host-side errors), the ctypes
signatures of the five fleet calls, the six fleet units in the product build (csrc/teb_fleet_inst.hip, plain calling convention
of the solve, outside the opt_* table), and the conditioning of the fleets that tests/test_gpu_fleet.py compares with the CPU oracle."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import fleet_cases  # noqa: E402
import sensitivity  # noqa: E402

from teb_local_planner_amd import _abi, build, planner  # noqa: E402

THREADS = min(os.cpu_count() or 1, 16)


@pytest.mark.parametrize("make", [lambda: fleet_cases.point_fleet(11), lambda: fleet_cases.mixed_fleet(12)], ids=["points", "mixed"])
def test_pack_scenes_round_trip(make):
    f = make()
    p = _abi.pack_scenes(f.tables, f.vias)
    assert p.n == f.n_scenes and len(p.obstacles) == f.n_scenes
    assert p.rows == sum(len(t) for t in f.tables) and p.vertices == sum(len(t.vert_x) for t in f.tables)
    assert p.via_count.dtype == np.int32 and p.via_count.tolist() == [len(v) for v in f.vias]
    off = np.concatenate([[0], np.cumsum(p.via_count)])
    for s, (t, v) in enumerate(zip(f.tables, f.vias)):
        o = p.obstacles[s]
        assert o.count == len(t)
        for k in ("type", "dynamic"):
            assert [getattr(o, k)[i] for i in range(len(t))] == list(getattr(t, k))
        for k in ("ax", "ay", "bx", "by", "radius", "vx", "vy"):
            assert [getattr(o, k)[i] for i in range(len(t))] == list(getattr(t, k)), k
        assert [o.vert_offset[i] for i in range(len(t) + 1)] == list(t.vert_offset)
        assert [o.vert_x[i] for i in range(len(t.vert_x))] == list(t.vert_x)
        assert [o.vert_y[i] for i in range(len(t.vert_y))] == list(t.vert_y)
        assert list(zip(p.via_x[off[s]:off[s + 1]], p.via_y[off[s]:off[s + 1]])) == [tuple(map(float, q)) for q in v]
    assert p.via_points == sum(len(v) for v in f.vias)


def test_fleets_differ_and_interleave():
    for f in (fleet_cases.point_fleet(11), fleet_cases.mixed_fleet(12)):
        counts = [len(f.bands_of(s)) for s in range(f.n_scenes)]
        assert all(1 <= c <= 5 for c in counts) and sum(counts) == f.batch.count
        assert len({len(t) for t in f.tables}) > 1                       # the scenes differ
        assert (np.diff(f.scene_of) != 0).sum() > f.n_scenes - 1          # not grouped by scene
    f = fleet_cases.mixed_fleet(12)
    assert sum(len(t) == 0 for t in f.tables) == 1


def test_oracle_fleets_are_the_stated_sizes():
    f = fleet_cases.oracle_point_fleet()
    assert f.n_scenes == 64 and f.batch.count == 256 and all(len(t) == 60 for t in f.tables) and (f.batch.n == 100).all()
    assert all(len(f.bands_of(s)) == 4 for s in range(64)) and any(any(t.dynamic) for t in f.tables)
    g = fleet_cases.oracle_mixed_fleet()
    assert g.n_scenes == 6 and sum(len(t) == 0 for t in g.tables) == 1 and any(g.vias)
    types = {ty for t in g.tables for ty in t.type}
    assert types == {_abi.OBST_POINT, _abi.OBST_CIRCULAR, _abi.OBST_LINE, _abi.OBST_PILL, _abi.OBST_POLYGON}


@pytest.mark.parametrize("make", [fleet_cases.oracle_point_fleet, fleet_cases.oracle_mixed_fleet], ids=["points", "mixed"])
def test_no_band_of_the_oracle_fleets_is_ill_conditioned(oracle, make):
    """The oracle-parity tests of tests/test_gpu_fleet.py compare EVERY band (tols=None, skipped == 0), so every band has to be one on
    which the oracle's own two Jacobian modes agree: sensitivity.band_tolerances marks none with None (different pose counts or status)
    and none above WELL_CONDITIONED_TOL. Neither mode involves the GPU; a change of a seed or of fleet_cases.*_ORACLE_REPLACED that
    brings in an ill-conditioned band fails here, before a GPU sees it."""
    f = make()
    marked = []
    for sc in range(f.n_scenes):
        sub, idx = f.scene_batch(sc)
        if not idx:
            continue
        tols = sensitivity.band_tolerances(oracle, f.cfg, f.tables[sc], f.vias[sc], sub, threads=THREADS)
        marked += [(sc, b, t) for b, t in zip(idx, tols) if t is None or t > sensitivity.WELL_CONDITIONED_TOL]
    assert not marked, "(scene, band, tolerance) of the ill-conditioned bands: %s" % marked


def test_pack_scenes_shape_errors():
    t = _abi.ObstacleTable()
    t.add_point(1.0, 2.0)
    with pytest.raises(ValueError, match="at least one scene"):
        _abi.pack_scenes([])
    with pytest.raises(ValueError, match="via-point lists"):
        _abi.pack_scenes([t, t], [[]])
    with pytest.raises(ValueError, match="pair"):
        _abi.pack_scenes([t], [[(1.0, 2.0, 3.0)]])
    with pytest.raises(ValueError, match="ObstacleTable"):
        _abi.pack_scenes([t, None])
    p = _abi.pack_scenes([t, t], None)   # None: no via-points anywhere
    assert p.via_count.tolist() == [0, 0] and p.via_points == 0


def test_pack_scenes_capacity_errors():
    f = fleet_cases.mixed_fleet(12)
    rows, verts, vias = (sum(len(t) for t in f.tables), sum(len(t.vert_x) for t in f.tables), sum(len(v) for v in f.vias))
    assert rows > 0 and verts > 0 and vias > 0
    _abi.pack_scenes(f.tables, f.vias, max_tebs=f.n_scenes, max_obstacles=rows, max_obstacle_vertices=verts, max_via_points=vias)
    for kw, what in ((dict(max_tebs=f.n_scenes - 1), "scenes"), (dict(max_obstacles=rows - 1), "obstacle rows"),
                     (dict(max_obstacle_vertices=verts - 1), "polygon vertices"), (dict(max_via_points=vias - 1), "via-points")):
        with pytest.raises(ValueError, match=what):
            _abi.pack_scenes(f.tables, f.vias, **kw)


def test_ctypes_signatures_of_the_fleet_calls():
    L = planner.lib()
    vp, i32 = C.c_void_p, C.c_int32
    assert L.teb_amd_set_scenes.argtypes == [vp, i32, C.POINTER(_abi.Obstacles), _abi.p_i32, _abi.p_f64, _abi.p_f64]
    assert L.teb_amd_set_band_scenes.argtypes == [vp, _abi.p_i32, i32]
    assert L.teb_amd_clear_scenes.argtypes == [vp]
    assert L.teb_amd_get_scene_count.argtypes == [vp, _abi.p_i32]
    assert L.teb_amd_select_best_per_scene.argtypes == [vp, _abi.p_i32, _abi.p_i32, _abi.p_i32, _abi.p_f64]
    for m in ("set_scenes", "set_band_scenes", "clear_scenes", "scene_count", "select_best_per_scene"):
        assert callable(getattr(planner.TebBatchSolver, m))
    assert callable(planner.TebFleetPlanner.plan) and callable(planner.TebFleetPlanner.getVelocityCommands)
    # no handle: every fleet call refuses a null handle instead of touching it (no GPU needed for that)
    n = i32(7)
    assert L.teb_amd_get_scene_count(None, C.byref(n)) == _abi.ERR_INVALID_ARG
    assert L.teb_amd_clear_scenes(None) == _abi.ERR_INVALID_ARG
    assert L.teb_amd_set_band_scenes(None, None, 0) == _abi.ERR_INVALID_ARG
    assert L.teb_amd_set_scenes(None, 0, None, None, None, None) == _abi.ERR_INVALID_ARG
    assert L.teb_amd_select_best_per_scene(None, None, None, None, None) == _abi.ERR_INVALID_ARG


def test_the_six_fleet_units_of_the_product():
    units = {obj: (src, defs) for obj, src, defs in build._units("product")}
    fleet = sorted(o for o in units if o.startswith("fleet_"))
    assert fleet == sorted("fleet_%d_0_%d.o" % (sv, sk) for sv in (0, 1, 2) for sk in (0, 1))
    for o in fleet:
        src, defs = units[o]
        m = re.fullmatch(r"fleet_(\d)_0_(\d)\.o", o)
        assert src == "teb_fleet_inst.hip"
        assert "-DTEB_AMD_FLEET" in defs and "-DTEB_AMD_SOLVE_CSR" in defs, (o, defs)
        assert "-DTEB_INST_SOLVER=%s" % m.group(1) in defs and "-DTEB_INST_SCENE=%s" % m.group(2) in defs
        assert o not in build.UNIT_FLAGS and not re.fullmatch(r"opt_\d+_\d+_\d+\.o", o)
        assert build.FLEET_UNIT_FLAGS[o] == ["-DTEB_AMD_FLEET", "-DTEB_AMD_SOLVE_CSR"]
    for variant in ("mfma", "analytic", "exp"):   # product only
        assert not [o for o, _, _ in build._units(variant) if o.startswith("fleet_")]


def test_the_guarded_edit_leaves_the_single_scene_kernel_text_alone():
    """teb_kernel.hpp names FleetDev / fl only under TEB_AMD_FLEET: with the guarded regions taken out, no fleet word is left."""
    src = open(os.path.join(build.CSRC, "teb_kernel.hpp")).read()
    assert src.count("#ifdef TEB_AMD_FLEET") == 2 and src.count("#ifndef TEB_AMD_FLEET") == 1
    out, stack = [], []
    for line in src.splitlines():
        t = line.strip()
        if t.startswith("#if"):
            stack.append("fleet" if t.startswith("#ifdef TEB_AMD_FLEET") else ("nofleet" if t.startswith("#ifndef TEB_AMD_FLEET") else "other"))
            if stack[-1] != "other":
                continue
        elif t.startswith("#else") and stack and stack[-1] in ("fleet", "nofleet"):
            stack[-1] = "nofleet" if stack[-1] == "fleet" else "fleet"
            continue
        elif t.startswith("#endif") and stack:
            if stack.pop() != "other":
                continue
        if "fleet" not in stack:
            out.append(line)
    text = "\n".join(out)
    assert "FleetDev" not in text and "TEB_AMD_FLEET" not in text and not re.search(r"\bfl\.", text)
    assert "teb_optimize_kernel(const teb_amd_config_t c, const SceneDev sc, const BatchDev bt, const OptArgs args," in text
