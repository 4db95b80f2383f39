"""TimedElasticBand::autoResize (reference src/timed_elastic_band.cpp:227-286) pinned sweep by sweep - the CPU side.

The reference of this pin is tests/hp_autoresize.py: the reference's loop restated on Python lists (list.insert / del, `i -= 1`), whose
n, dt, x, y are exact expectations and whose headings are evaluated at 80 digits through the whole split tree. The cases are those of
tests/autoresize_cases.py (threshold ladders, guards, the limits of the chain machine, sizes on every wave / slot / layout boundary,
capacity, a batch with a NaN). The fixtures under tests/golden/hp_autoresize_*.npz hold what the restatement gives
(tests/golden/make_hp_autoresize.py); tests/test_gpu_hp_autoresize.py compares the device with them. Here:

  * the fixtures are what the restatement gives today (bit for bit), for every case, none skipped;
  * the CPU oracle (oracle/teb_oracle.cpp, an edit-free C++ loop of its own) equals the restatement on every case and sweep: n, dt, x, y
    bit-equal, headings within max(256 eps, 16 x err_ref) of the 80-digit value;
  * the coverage conditions hold on the reference alone: every threshold x {=, +1 ulp, -1 ulp} x provenance combination occurs for
    both parameter pairs (dt_ref - hyst x halved cannot - a half exceeds dt_ref - and is asserted never to occur); no case outside
    the ladders compares anything within 1 ulp of a threshold; both guards are met at the last count that passes and at the first that
    binds, in fast and in full mode; every sweep class (chains, chains gave up, guard, nothing fires) occurs among the cases of every
    layout and among the bands that need that layout; every size pattern from T = 63 up also runs on the sequential machine; every average is well conditioned (|e^ia + e^ib| >= 1) and no case touches the reference's undefined behaviour;
  * the checker (hp_autoresize.check_band) rejects each of nine mutations of the restatement on at least one case.
"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import hp_autoresize as HA  # noqa: E402
import autoresize_cases as AC  # noqa: E402
import make_hp_autoresize as MK  # noqa: E402

from oracle import oracle_py  # noqa: E402

_REF = {}


def ref(name):
    """(case, fixture entries recomputed) - once per case, shared by the tests below"""
    if name not in _REF:
        _REF[name] = MK.reference_record(name)
    return _REF[name]


def test_every_case_has_its_fixture_and_no_other():
    want = {}
    for name in AC.CASES:
        want.setdefault(AC.group_of(name), set()).add(name)
    have = {f[:-4] for f in os.listdir(os.path.join(HERE, "golden")) if f.startswith("hp_autoresize_") and f.endswith(".npz")}
    assert have == set(want)
    for g, names in want.items():
        fx = np.load(os.path.join(HERE, "golden", g + ".npz"))
        assert {k.split("/")[0] for k in fx.files} == names
        assert os.path.getsize(os.path.join(HERE, "golden", g + ".npz")) < MK.MAX_FILE_BYTES == 500 * 1000, g
    assert {AC.build(n)["family"] for n in AC.CASES} == set(AC.FAMILIES)


@pytest.mark.parametrize("name", AC.CASES)
def test_fixture_is_the_restatement(name):
    c, rec = ref(name)
    fx = MK.load(name)
    assert str(fx[name + "/hash"]) == MK.case_hash(c)
    mine = {k for k in fx.files if k.startswith(name + "/")}
    assert mine == set(rec)
    for k in mine:
        a, b = np.asarray(fx[k]), np.asarray(rec[k])
        assert a.shape == b.shape and a.dtype == b.dtype, k
        assert a.tobytes() == b.tobytes(), k
    for j in range(len(c["members"])):   # conditioning, and the reference's undefined behaviour was not met (reference() would have raised)
        assert float(rec["%s/m%d/conditioning" % (name, j)]) >= 1.0   # (inf where the case takes no average)


@pytest.mark.parametrize("name", AC.CASES)
def test_oracle_equals_the_restatement(name):
    c, rec = ref(name)
    fx = MK.load(name)
    args = (c["dt_ref"], c["hyst"], c["min_samples"], c["max_samples"])
    worst = 0.0
    for j, m in enumerate(c["members"]):
        k = "%s/m%d/" % (name, j)
        sg = ((m["x"][0], m["y"][0], m["theta"][0]), (m["x"][-1], m["y"][-1], m["theta"][-1]))
        if not c["fast"]:
            want, over = MK.expected(fx, c, j, 0)
            assert not over
            got = oracle_py.autoresize(m["x"], m["y"], m["theta"], m["dt"], *args, False, cap=2048)
            bad, e = HA.check_band(got, want, sg)
            assert not bad, (name, j, bad)
            worst = max(worst, e)
            continue
        x, y, th, dt = m["x"], m["y"], m["theta"], m["dt"]
        for call in range(c["calls"]):
            want, over = MK.expected(fx, c, j, call)
            got = oracle_py.autoresize(x, y, th, dt, *args, True, cap=2048)
            if over:   # the sweep the handle cannot hold leaves exactly one pose too many where the case says so
                assert len(got[0]) > c["cap"]
                if c["name"].endswith("_over"):
                    assert len(got[0]) == c["cap"] + 1
                break
            bad, e = HA.check_band(got, want, sg)
            assert not bad, (name, j, call, bad)
            worst = max(worst, e)
            x, y, th, dt = got   # (the oracle's own headings go into its next sweep, as the device's do)
    print("%s: oracle heading error %.1f eps" % (name, worst / HA.EPS))


def _records(name):
    c, rec = ref(name)
    return c, [(j, rec["%s/m%d/records" % (name, j)], rec["%s/m%d/classes" % (name, j)]) for j in range(len(c["members"]))]


def test_every_rung_occurs_and_only_in_the_ladders():
    seen = {AC.DEFAULTS: np.zeros((3, 4, 3), np.int64), AC.DYADIC: np.zeros((3, 4, 3), np.int64)}
    for name in AC.CASES:
        c, per_member = _records(name)
        for j, r, _ in per_member:
            rungs = r[:, :3, :, :3].sum(axis=0)
            assert rungs[HA.THR_LO, HA.P_HALVED].sum() == 0, name   # a half exceeds dt_ref
            if c["ladder"] and j == 0:
                assert rungs.sum() > 0, name
                if c["family"] == "ladder":
                    seen[(c["dt_ref"], c["hyst"])] += rungs
            else:
                assert rungs.sum() == 0, (name, j, "a comparison within 1 ulp of a threshold outside the ladders")
    for pair, s in seen.items():
        for t in range(3):
            for p in range(4):
                for r in range(3):
                    if (t, p) != (HA.THR_LO, HA.P_HALVED):
                        assert s[t, p, r] > 0, (pair, HA.THR_NAMES[t], HA.PROV_NAMES[p], ("=", "+1 ulp", "-1 ulp")[r])


def test_the_point_two_of_the_defaults_is_kept():
    c, rec = ref("ladder_def_input_fast")
    assert 0.2 in c["members"][0]["dt"] and 0.3 - 0.1 < 0.2
    assert 0.2 in rec["ladder_def_input_fast/m0/b0/dt"]


def test_guards_are_met_either_side():
    for mode in ("fast", "full"):
        g = np.zeros((2, 4), np.int64)
        later = np.zeros((2, 4), np.int64)
        for name in AC.CASES:
            c, per_member = _records(name)
            if c["family"] == "guards" and name.endswith(mode):
                for _, r, _ in per_member:
                    g += r[:, HA.THR_MAX:].sum(axis=(0, 2))
                    later += r[1:, HA.THR_MAX:].sum(axis=(0, 2))
        assert g[0, HA.R_EQ] and g[0, HA.R_DOWN], (mode, "max_samples: first count that binds, last that passes")
        assert g[1, HA.R_EQ] and g[1, HA.R_UP], (mode, "min_samples: first count that binds, last that passes")
        assert later[0].sum() > 0, (mode, "a max_samples comparison in a sweep after the first")


def test_every_sweep_class_in_every_layout():
    """.. among the cases pinned to the layout, and among the bands that NEED the layout (more poses than the faster layout holds)"""
    seen = {L: set() for L, _ in AC.LAYOUT_LIMITS}
    needs = {L: set() for L, _ in AC.LAYOUT_LIMITS}
    below = {"cr": 0, "band": 238, "bandg": 337}
    longest = {}
    for name in AC.CASES:
        c, per_member = _records(name)
        for j, _, cl in per_member:
            for L in {v[0] for v in c["variants"]} - {"auto"}:
                seen[L] |= set(cl[:, 0].tolist())
            own = AC.own_layout(c["cap"])
            if len(c["members"][j]["x"]) > below[own]:
                needs[own] |= set(cl[:, 0].tolist())
            for k, steps in cl.tolist():
                longest[k] = max(longest.get(k, 0), steps)
        if name.endswith("_seq"):   # the size patterns on the sequential machine
            assert per_member[0][2][0, 0] in (AC.CLASS_GUARD, AC.CLASS_GAVE_UP), name
            assert int(ref(name)[1][name + "/m0/modified"][0]) == 1, name   # .. and the rules did fire
        elif c["family"] == "sizes" and per_member[0][2][0, 0] != AC.CLASS_NOTHING:
            assert per_member[0][2][0, 0] == AC.CLASS_CHAINS or c["min_samples"] == 1, name
    everything = {AC.CLASS_CHAINS, AC.CLASS_GAVE_UP, AC.CLASS_GUARD, AC.CLASS_NOTHING}
    for L in seen:
        assert seen[L] == everything, (L, seen[L])
        assert needs[L] == everything, (L, needs[L])
    for group, Ts in AC.SIZES.items():
        for T in Ts:
            for pat in ("taillast", "trigfirst", "mix"):
                assert (("sizes_%s_T%d_%s_seq" % (group, T, pat)) in AC.CASES) == (T >= 63)
    assert longest[AC.CLASS_CHAINS] == 64   # a member chain that takes every evaluation the chain machine allows
    for length, cls in ((63, AC.CLASS_CHAINS), (64, AC.CLASS_CHAINS), (65, AC.CLASS_GAVE_UP)):
        for n in (100, 330, 600):
            assert _records("chain_creep%d_n%d" % (length, n))[1][0][2][0].tolist() == [cls, min(length, 64)]
    for n in (60, 280, 540):
        assert _records("chain_split16_n%d" % n)[1][0][2][0, 0] == AC.CLASS_CHAINS
        assert _records("chain_split32_n%d" % n)[1][0][2][0, 0] == AC.CLASS_GAVE_UP


def test_capacity_cases_stop_where_they_say():
    for name in AC.CASES:
        c, rec = ref(name)
        stopped = [int(rec["%s/m%d/stopped" % (name, j)]) for j in range(len(c["members"]))]
        assert any(stopped) == name.endswith("_over"), name
        if name.endswith("_fit"):
            assert len(rec[name + "/m0/b0/x"]) == c["cap"]
    assert len(ref("capacity_outgrow_band")[1]["capacity_outgrow_band/m0/b0/x"]) > 238   # more than the blocks layout holds


@pytest.mark.parametrize("mutation", HA.MUTATIONS)
def test_checker_rejects_mutation(mutation):
    rejected = []
    for name in AC.CASES:
        c, rec = ref(name)
        fx = MK.load(name)
        for j, m in enumerate(c["members"]):
            try:
                r = AC.reference(c, j, mutation=mutation, high_precision=False)
            except (HA.Undefined, IndexError):
                continue   # (a mutant that leaves the defined behaviour on this band proves nothing here)
            bands = r["sweeps"] if c["fast"] else [r["final"]]
            for call, b in enumerate(bands):
                want, over = MK.expected(fx, c, j, call)
                if over:
                    break
                bad, _ = HA.check_band((b["x"], b["y"], b["theta"], b["dt"]), want,
                                       ((m["x"][0], m["y"][0], m["theta"][0]), (m["x"][-1], m["y"][-1], m["theta"][-1])))
                if bad:
                    rejected.append((name, call, bad[0]))
                    break
        if len(rejected) >= 2:
            break
    assert rejected, mutation
    print(mutation, "rejected on", rejected)
