"""Cases of tests/test_hp_autoresize.py and tests/test_gpu_hp_autoresize.py. NOT a test file.

A case is one launch configuration (dt_ref, dt_hysteresis, min_samples, max_samples, fast or full mode, pose capacity of the handle) and
one band - the batch case: eight - on which TimedElasticBand::autoResize (reference src/timed_elastic_band.cpp:227-286) runs alone:
optimize(0, 1) leaves after autoResize and the graph side data (g2o's optimize(0)), so the downloaded band is the output of one
autoResize() call; in fast mode (include_dynamic_obstacles = false) that is one sweep, and `calls` calls in a row show the sweeps one
after the other. build(name) returns dict(members=[dict(x, y, theta, dt)], dt_ref, hyst, min_samples, max_samples, fast, calls, cap,
variants=[(layout, generic_config_path, fixed_layout)], ladder, family, nan_member).

Bands: irregular x, y (a pose built from the wrong parent, or shifted by one, changes bits), headings that walk by at most 0.25 rad from
pose to pose and wrap at +- pi (atan2 either side of the branch cut); the restatement asserts |e^ia + e^ib| >= 1 for every average it
takes (tests/test_hp_autoresize.py), i.e. parents at most 2 pi / 3 apart - also after merges have removed poses between them.

Families
  ladder    a time difference AT each of the three thresholds (dt_ref + hyst, 2 dt_ref, dt_ref - hyst, formed in fp64 as the reference
            forms them) and on its two fp64 neighbours, reached four ways: as an input interval, after an excess was pushed onto it
            (the builder picks the neighbour so that the fp64 sum lands on the rung), after a merge, after a halving (2 hi halves to
            exactly hi and is kept, 2 nextafter(hi) halves to a push). Defaults (0.3 / 0.1; 0.3 - 0.1 = 0.19999999999999998, so the band
            also holds dt = 0.2, which is NOT too short) and a dyadic pair (0.25 / 0.0625). Each also through generic_config_path.
            dt_ref - hyst x halved cannot occur: only an interval above 2 dt_ref is halved, its halves exceed dt_ref.
  guards    max_samples in {T, T + 1, T + 2, T + 3} against six intervals that want a split and four that want a push (none, one, two,
            three splits; everything after that is neither split nor pushed, :239), min_samples in {T, T - 1, T - 2, T - 3} against six
            short intervals and a short last one, `flip`: the max_samples guard binds, is released by merges and binds again within
            one sweep, `release`: it binds early in sweep 1, merges behind it release it, and the intervals it held back are pushed and
            split in sweep 2;
            fast and full mode; one 1000 s interval under max_samples = n + 28 and 500: a lopsided tree of 11 levels whose waiting
            halves spill the sequential machine's stack registers.
            (A guard cannot bind FIRST in sweep 2: the output of a sweep in which no guard bound has every interval inside
            [dt_ref - hyst, dt_ref + hyst] except the one the last-interval rule added to, which is below 2 dt_ref and is met at
            sizeTimeDiffs() <= max_samples - 1. What a later sweep can see is a guard that bound in sweep 1 and does no longer:
            `release`.)
  chain     the limits of the chain machine (csrc/teb_autoresize_chain.hpp: kArChainSteps = 64 evaluations, kArChainStack = 4 waiting
            halves): an excess handed on over 63, 64, 65 intervals (dt = 0.41, then 0.3, an absorbing 0.25), placed at the start of a
            band and across interval 256 and 512 (the second and third slot of a lane); splits of 16 dt_ref (1 + 2^-20) - four halves
            wait - and 32 dt_ref (1 + 2^-20) - five: the chains give up.
  sizes     T = n - 1 on either side of every wave, workgroup, slot and layout boundary, three patterns each: `taillast` (dead band
            everywhere, a too short LAST interval: T member chains of one evaluation, the tail applied to the previous chain's interval;
            sequential machine: one run record over the band plus the tail), `trigfirst` (the same with the short interval first),
            `mix` (triggers of every kind on both sides of every multiple of 64, and some more). With min_samples = 3 every one of
            these sweeps belongs to the chains; for T >= 63 each pattern runs again as `_seq` with min_samples = T - (merges of the
            sweep): the chains hand the sweep over (a guard may bind) and every rule still fires, so the sequential machine meets
            the same boundaries - run records and ballot masks up to interval 942, one run over a whole band plus the tail.
  capacity  a sweep whose output has exactly `cap` poses (fits) and cap + 1 (TEB_FAILED, bit 2 of the overflow flags, band as before the
            sweep), by the chains and by the sequential machine; handles much larger than the band, where the host launches an
            optimistic layout that the band outgrows and repeats the launch - against fixed_layout.
  batch     eight bands of different families and lengths in one launch, one with a NaN time difference mid-band (every comparison
            with it is false: the interval passes through; status TEB_NONFINITE), the seven others untouched by it.

Which machine runs a sweep on the device is not observable; sweep_class() decides it on the inputs with the host build of the chain
header (tests/host/autoresize_chains_host.cpp, info[5]) - a condition on the inputs, not a claim about the device.

Out of scope: infinite time differences (the reference splits until max_samples, the device reports overflow when 64 halves wait), and
the reference's own undefined behaviour - the last-interval rule at i = 0 reads TimeDiff(-1) - which min_samples >= 1 and the
restatement's refusal (hp_autoresize.Undefined) keep out: asserted below and in tests/test_hp_autoresize.py.
"""
import ctypes as C
import math
import os
import subprocess
import tempfile
import zlib

import numpy as np

import hp_autoresize as HA

HERE = os.path.dirname(os.path.abspath(__file__))
LAYOUT_LIMITS = (("cr", 238), ("band", 337), ("bandg", 944))   # pose capacity of the three layouts of the normal matrix
LAYOUT_INDEX = {"band": 0, "cr": 1, "bandg": 2}                 # teb_amd_debug_last_instantiation's numbering
CLASS_CHAINS, CLASS_GAVE_UP, CLASS_GUARD, CLASS_NOTHING = range(4)   # sweep_class(); NOTHING: no rule fires, neither machine runs
CLASS_NAMES = ("chains", "chains gave up", "guard may bind", "nothing fires")
DEFAULTS, DYADIC = (0.3, 0.1), (0.25, 0.0625)
SIZES = {"blocks": (1, 2, 63, 64, 65, 127, 128, 129, 237), "lds": (255, 256, 257, 336), "hbm": (511, 512, 513, 767, 768, 769, 943)}
SIZE_CAP = {"blocks": 238, "lds": 337, "hbm": 944}
up = lambda v: math.nextafter(v, math.inf)
down = lambda v: math.nextafter(v, -math.inf)


def own_layout(cap):
    return next(name for name, most in LAYOUT_LIMITS if cap <= most)


def layouts_for(cap):
    return [name for name, most in LAYOUT_LIMITS if cap <= most]


def poses(rng, n):
    x = np.cumsum(rng.uniform(0.05, 0.3, n)); y = np.cumsum(rng.normal(0, 0.05, n))
    th = np.cumsum(rng.uniform(-0.25, 0.25, n)) + rng.uniform(-3, 3)
    return x, y, (th + math.pi) % (2 * math.pi) - math.pi


def dead(rng, T, dt_ref=0.3):
    """time differences well inside the dead band"""
    return rng.uniform(dt_ref * 0.87, dt_ref * 1.13, T)


def _landing(target, first, addend_of=lambda a: a):
    """(a, b) with fl(b + addend_of(a)) == target: a = `first` or one of its upper fp64 neighbours, b next to target - addend"""
    a = first
    for _ in range(64):
        addend = addend_of(a)
        b = target - addend
        for _ in range(8):
            s = b + addend
            if s == target:
                return [a, b]
            b = up(b) if s < target else down(b)
        a = up(a)
    raise AssertionError("no fp64 pair lands on the rung")


def absorb(rng, dt_ref):
    """five intervals low in the dead band: whatever excess the rung before them hands on (at most dt_ref) has died out behind them, so
    that the next rung is met as it was built"""
    return rng.uniform(0.76 * dt_ref, 0.80 * dt_ref, 5)


def ladder_dt(rng, pair, provenance):
    dt_ref, hyst = pair
    hi, big, lo = HA.thresholds(dt_ref, hyst)
    out = []
    for thr in (hi, big, lo):
        for rung in (thr, up(thr), down(thr)):
            out += list(absorb(rng, dt_ref))
            if provenance == "input":
                out.append(rung)
            elif provenance == "pushed":   # a in (hi, big]: its excess fl(a - dt_ref) goes onto b
                out += _landing(rung, dt_ref + 1.5 * hyst, lambda a: a - dt_ref)
            elif provenance == "merged":   # a < lo is added to b: TimeDiff(i+1) + TimeDiff(i)
                out += _landing(rung, 0.35 * dt_ref)
            elif thr != lo:                # halved (a half exceeds dt_ref: never near dt_ref - hyst)
                out.append(2 * rung)
    if pair == DEFAULTS and provenance == "input":
        out += list(absorb(rng, dt_ref)) + [0.2]
    out += list(absorb(rng, dt_ref))
    return np.array(out)


def creep_dt(rng, T, start, length):
    """an excess handed on from interval `start` over `length` rule evaluations: 0.41, 0.3 .., an absorbing 0.25"""
    dt = dead(rng, T)
    dt[start] = 0.41; dt[start + 1:start + length - 1] = 0.3; dt[start + length - 1] = 0.25
    return dt


def mix_dt(rng, T):
    dt = dead(rng, T)
    marks = set()
    for m in range(64, T + 1, 64):
        marks |= {m - 1, m}
    marks |= set(int(v) for v in rng.choice(T, T // 12, replace=False)) if T >= 12 else set()
    kinds = (0.08, 0.47, 0.12, 0.75, 0.09)   # merge, push, merge, split, merge: the band shrinks (a band at its layout's capacity fits)
    for q, p in enumerate(sorted(m for m in marks if m < T)):
        dt[p] = kinds[q % 5] * rng.uniform(0.97, 1.03)
    return dt


def _case(family, dt, rng, pair=DEFAULTS, min_samples=3, max_samples=2000, fast=True, calls=2, cap=None, generic=False, ladder=False,
          variants=None, n=None):
    x, y, th = poses(rng, len(dt) + 1)
    c = dict(family=family, members=[dict(x=x, y=y, theta=th, dt=np.asarray(dt, np.float64))], dt_ref=pair[0], hyst=pair[1],
             min_samples=min_samples, max_samples=max_samples, fast=fast, calls=calls if fast else 1, cap=cap, ladder=ladder, nan_member=-1)
    if variants is None:
        variants = [("auto", False, False)] + [(L, False, False) for L in layouts_for(cap)]
        if generic:
            variants += [(L, True, False) for L in ["auto"] + layouts_for(cap)]
    c["variants"] = variants
    return c


def _seed(name):
    return zlib.crc32(name.encode())   # the whole name: every case its own stream


def _builders():
    B = {}

    def add(name, fn):
        assert name not in B
        B[name] = fn

    # ladder
    for pname, pair in (("def", DEFAULTS), ("dy", DYADIC)):
        for prov in ("input", "pushed", "merged", "halved"):
            for mode in ("fast", "full"):
                add("ladder_%s_%s_%s" % (pname, prov, mode), lambda rng, pair=pair, prov=prov, mode=mode: _case(
                    "ladder", ladder_dt(rng, pair, prov), rng, pair=pair, max_samples=500, fast=mode == "fast", cap=96, generic=True, ladder=True))
    # guards
    T = 40

    def guard_band(rng, shorts, splits, pushes, short_last=False):
        dt = dead(rng, T)
        for p in shorts: dt[p] = 0.1 + rng.uniform(0, 0.01)   # (irregular: no sum lands next to a threshold by accident)
        for p in splits: dt[p] = 0.7 + rng.uniform(0, 0.01)
        for p in pushes: dt[p] = 0.5 + rng.uniform(0, 0.01)
        if short_last: dt[-1] = 0.1 + rng.uniform(0, 0.01)
        return dt
    for mode in ("fast", "full"):
        for k in range(4):
            add("guards_max%d_%s" % (k, mode), lambda rng, k=k, mode=mode: _case(
                "guards", guard_band(rng, (), (4, 10, 16, 22, 28, 34), (7, 19, 31, 37)), rng, max_samples=T + k, fast=mode == "fast", cap=64))
            add("guards_min%d_%s" % (k, mode), lambda rng, k=k, mode=mode: _case(
                "guards", guard_band(rng, (4, 10, 16, 22, 28, 34), (), (), short_last=True), rng, min_samples=T - k, max_samples=500,
                fast=mode == "fast", cap=64))
        add("guards_release_%s" % mode, lambda rng, mode=mode: _case(
            "guards", guard_band(rng, (20, 21, 30), (4, 10), (6,)), rng, min_samples=3, max_samples=T + 1, fast=mode == "fast", calls=3, cap=64))
        add("guards_flip_%s" % mode, lambda rng, mode=mode: _case(
            "guards", guard_band(rng, (8, 9, 20, 21, 32), (4, 14, 26, 36), (6, 30)), rng, min_samples=3, max_samples=T + 1, fast=mode == "fast",
            calls=3, cap=64))

    def lastlong(rng):
        dt = dead(rng, T); dt[-1] = 0.5 + rng.uniform(0, 0.01)
        return dt
    add("guards_lastlong_fast", lambda rng: _case("guards", lastlong(rng), rng, cap=64))   # :256: the last interval's excess goes nowhere

    def tree(rng):
        dt = dead(rng, 11); dt[5] = 1000.0
        return dt
    add("guards_tree28_fast", lambda rng: _case("guards", tree(rng), rng, max_samples=12 + 28, cap=64))
    add("guards_tree28_full", lambda rng: _case("guards", tree(rng), rng, max_samples=12 + 28, fast=False, cap=64))
    add("guards_tree500_fast", lambda rng: _case("guards", tree(rng), rng, max_samples=500, cap=512))
    # chain limits
    for length in (63, 64, 65):
        add("chain_creep%d_n100" % length, lambda rng, length=length: _case("chain", creep_dt(rng, 99, 0, length), rng, cap=128))
        add("chain_creep%d_n330" % length, lambda rng, length=length: _case("chain", creep_dt(rng, 329, 256 - 30, length), rng, cap=337))
        add("chain_creep%d_n600" % length, lambda rng, length=length: _case("chain", creep_dt(rng, 599, 512 - 30, length), rng, cap=700))
    for factor in (16, 32):
        def split_band(rng, T, at, factor=factor):
            dt = dead(rng, T)
            for p in at: dt[p] = factor * 0.3 * (1 + 2.0 ** -20)
            return dt
        add("chain_split%d_n60" % factor, lambda rng, f=split_band: _case("chain", f(rng, 59, (0, 30, 58)), rng, cap=238))
        add("chain_split%d_n280" % factor, lambda rng, f=split_band: _case("chain", f(rng, 279, (255,)), rng, cap=337))
        add("chain_split%d_n540" % factor, lambda rng, f=split_band: _case("chain", f(rng, 539, (256, 511, 512)), rng, cap=700))
    # sizes
    for group, Ts in SIZES.items():
        for T_ in Ts:
            small = 1 if T_ <= 3 else 3   # (T = 1: sizeTimeDiffs() > min_samples is false, no rule fires at i = 0)

            def taillast(rng, T_=T_):
                dt = dead(rng, T_); dt[-1] = 0.05
                return dt

            def trigfirst(rng, T_=T_):
                dt = dead(rng, T_); dt[0] = 0.05
                return dt
            mix = lambda rng, T_=T_: mix_dt(rng, T_)
            for pat, fn in (("taillast", taillast), ("trigfirst", trigfirst), ("mix", mix)):
                add("sizes_%s_T%d_%s" % (group, T_, pat), lambda rng, fn=fn, small=small, group=group: _case(
                    "sizes", fn(rng), rng, min_samples=small, cap=SIZE_CAP[group]))
                if T_ < 63:
                    continue
                # the same pattern for the SEQUENTIAL machine: min_samples = T - (merges of the sweep) makes the chains hand the sweep over
                # (T_in - merges <= min_samples: the guard may bind) while sizeTimeDiffs() > min_samples holds at every merge, so every
                # rule still fires - one run record over the band plus the tail, run records and ballot masks up to interval 942

                def seq(rng, fn=fn, group=group):
                    dt = fn(rng)
                    z = np.zeros(len(dt) + 1)
                    merges = HA.restate(z, z, z, dt, DEFAULTS[0], DEFAULTS[1], 1, 2000, True, high_precision=False)["merges"][0]
                    assert merges >= 1
                    return _case("sizes", dt, rng, min_samples=len(dt) - merges, calls=1, cap=SIZE_CAP[group])
                add("sizes_%s_T%d_%s_seq" % (group, T_, pat), seq)
    # capacity
    def grow(rng, n, at, value):
        dt = dead(rng, n - 1)
        for p in at: dt[p] = value * (1 + rng.uniform(0, 0.01))
        return dt
    chains_at, seq_at = tuple(range(2, 49, 4)), (10, 30)
    add("capacity_chains_fit", lambda rng: _case("capacity", grow(rng, 50, chains_at, 1.3), rng, cap=50 + 3 * len(chains_at)))
    add("capacity_chains_over", lambda rng: _case("capacity", grow(rng, 50, chains_at, 1.3), rng, cap=50 + 3 * len(chains_at) - 1))
    add("capacity_seq_fit", lambda rng: _case("capacity", grow(rng, 50, seq_at, 9.7), rng, cap=50 + 31 * len(seq_at)))
    add("capacity_seq_over", lambda rng: _case("capacity", grow(rng, 50, seq_at, 9.7), rng, cap=50 + 31 * len(seq_at) - 1))
    for lay, cap in (("band", 337), ("bandg", 944)):   # n = 200: the host launches the blocks layout (238 poses), the sweep leaves 320
        add("capacity_outgrow_%s" % lay, lambda rng, cap=cap: _case("capacity", grow(rng, 200, tuple(range(3, 199, 5)), 1.3), rng, cap=cap,
                                                                   variants=[("auto", False, False), ("auto", False, True)]))
    add("batch_eight", _batch)
    return B


def _batch(rng):
    """eight bands, one configuration (the defaults, max_samples = 2000, fast mode), one launch; member 5 has a NaN time difference"""
    dts = [ladder_dt(rng, DEFAULTS, "input"), creep_dt(rng, 99, 0, 64), creep_dt(rng, 199, 100, 65), mix_dt(rng, 257),
           np.concatenate([dead(rng, 20), [32 * 0.3 * (1 + 2.0 ** -20)], dead(rng, 20)]), mix_dt(rng, 129), np.concatenate([dead(rng, 64), [0.05]]),
           np.concatenate([dead(rng, 2), [0.05]])]
    dts[5][60] = math.nan
    c = _case("batch", dts[0], rng, cap=337, calls=2, variants=[("auto", False, False), ("band", False, False), ("bandg", False, False)])
    for dt in dts[1:]:
        x, y, th = poses(rng, len(dt) + 1)
        c["members"].append(dict(x=x, y=y, theta=th, dt=np.asarray(dt, np.float64)))
    c["nan_member"] = 5
    c["ladder"] = True   # (member 0 is a ladder band)
    return c


_BUILDERS = _builders()
CASES = list(_BUILDERS)
FAMILIES = ("ladder", "guards", "chain", "sizes", "capacity", "batch")


def build(name):
    c = _BUILDERS[name](np.random.default_rng(_seed(name)))
    c["name"] = name
    assert c["min_samples"] >= 1 and c["cap"] <= 944
    for m in c["members"]:
        assert len(m["x"]) <= c["cap"] and len(m["dt"]) == len(m["x"]) - 1 >= 1
        assert not np.isinf(m["dt"]).any()
    return c


def group_of(name):
    """the fixture file of a case: one per family; the sizes family one per layout group, the band-in-HBM sizes one per T (each file
    within make_hp_autoresize.MAX_FILE_BYTES)"""
    t = name.split("_")
    if t[0] != "sizes":
        return "hp_autoresize_" + t[0]
    return "hp_autoresize_sizes_" + t[1] + ("_" + t[2] if t[1] == "hbm" else "")


def params_of(c):
    return (c["dt_ref"], c["hyst"], c["min_samples"], c["max_samples"], bool(c["fast"]), c["calls"], c["cap"])


def reference(c, member=0, mutation=None, high_precision=True):
    """the restatement on one member: full mode one call, fast mode `calls` calls in a row (hp_autoresize.restate)"""
    m = c["members"][member]
    return HA.restate(m["x"], m["y"], m["theta"], m["dt"], c["dt_ref"], c["hyst"], c["min_samples"], c["max_samples"], False,
                      capacity=c["cap"], mutation=mutation, high_precision=high_precision, max_sweeps=c["calls"] if c["fast"] else 100, stop_unmodified=not c["fast"])


# -- which machine a sweep belongs to, decided on the inputs ----------------------------------------------------------------------------
_HOST = None


def host_lib():
    global _HOST
    if _HOST is None:
        so = os.path.join(tempfile.mkdtemp(prefix="teb_ar_"), "libar_host.so")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off",
                               os.path.join(HERE, "host", "autoresize_chains_host.cpp"), "-o", so])
        L = C.CDLL(so)
        pd, pi = C.POINTER(C.c_double), C.POINTER(C.c_int)
        L.teb_host_autoresize_chains.restype = C.c_int
        L.teb_host_autoresize_chains.argtypes = [pd, C.c_int, C.c_double, C.c_double, C.c_int, C.c_int, C.c_int, pd, pi, pi, pd, pi]
        _HOST = L
    return _HOST


def sweep_class(dt, c, fired):
    """(class, longest member chain in rule evaluations) of one sweep over the time differences dt"""
    if not fired:
        return CLASS_NOTHING, 0
    cap = 4096
    d = np.ascontiguousarray(dt, np.float64)
    odt = np.zeros(cap); desc = np.zeros(cap + 1, np.int32); rec = np.zeros(cap, np.int32); tail = np.zeros(1); info = np.zeros(10, np.int32)
    as_d = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    as_i = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
    rc = host_lib().teb_host_autoresize_chains(as_d(d), len(d), c["dt_ref"], c["hyst"], c["min_samples"], c["max_samples"], cap, as_d(odt),
                                               as_i(desc), as_i(rec), as_d(tail), as_i(info))
    assert rc == 0
    return int(info[5]), int(info[7])
