"""The reference's own outputs for the tests that call it (oracle/_ref) on seeded cases, kept for checkouts without that library.

Where oracle/_ref is built, `python tests/golden/ref_replay.py` runs those tests against it and records, per test case, every call they
make to the reference and what it returned, into ref_replay_<group>.npz. Without the library the tests get the recorded values back,
call by call in the same order, and check the oracle against them exactly as they check it against the live code. The files hold data
only: arrays, and the shape of the tuples / dicts / host batches that held them."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
RECORD = None   # {group: {case: [(method, output), ..]}} while main() records


def reference(group, case, live):
    """What a test calls the reference through: `live` (the loaded oracle/_ref module, or None) if there is one, else the replay of
    the recorded case."""
    if live is None:
        return _Replay(group, str(case))
    if RECORD is None:
        return live
    rec = _Recorder(live)
    RECORD.setdefault(group, {})[str(case)] = rec.calls
    return rec


class _Recorder:
    def __init__(self, live):
        self._live, self.calls = live, []

    def __getattr__(self, name):
        fn = getattr(self._live, name)

        def call(*a, **k):
            out = fn(*a, **k)
            self.calls.append((name, out))
            return out
        return call


_FILES = {}


class _Replay:
    def __init__(self, group, case):
        if group not in _FILES:
            with np.load(os.path.join(HERE, "ref_replay_%s.npz" % group)) as g:
                _FILES[group] = {k: g[k] for k in g.files}
        self._g, self._case, self._next = _FILES[group], case, 0
        assert case + "#calls" in self._g, "no recorded reference calls for %s case %s" % (group, case)

    def __getattr__(self, name):
        def call(*a, **k):
            key = "%s/%d" % (self._case, self._next)
            assert self._next < int(self._g[self._case + "#calls"]) and str(self._g[key + "#method"]) == name, \
                "the test calls the reference differently from the recording (%s, call %d: %s)" % (self._case, self._next, name)
            self._next += 1
            return _unflat(self._g, key)
        return call


def _flat(obj, key, out):
    from teb_local_planner_amd import _abi
    if isinstance(obj, dict):
        out[key + "#dict"] = np.array(list(obj.keys()))
        for k, v in obj.items():
            _flat(v, key + "/" + k, out)
    elif isinstance(obj, _abi.TebBatchHost):
        out[key + "#batch"] = np.array([obj.count, obj.stride])
        for k in ("n", "x", "y", "theta", "dt", "has_vel_start", "vel_start", "has_vel_goal", "vel_goal", "prefer_rotdir", "via_points_enabled"):
            out[key + "/" + k] = getattr(obj, k)
    elif isinstance(obj, list) and obj and all(isinstance(v, list) for v in obj):   # ragged rows of ints (adjacency lists)
        out[key + "#ragged"] = np.cumsum([0] + [len(v) for v in obj])
        out[key + "/values"] = np.array([x for v in obj for x in v], np.int64)
    elif isinstance(obj, (tuple, list)):
        out[key + "#" + type(obj).__name__] = np.array(len(obj))
        for i, v in enumerate(obj):
            _flat(v, "%s/%d" % (key, i), out)
    elif obj is None:
        out[key + "#none"] = np.array(0)
    else:
        a = np.asarray(obj)
        assert a.dtype != object, (key, type(obj))
        out[key] = a


def _unflat(g, key):
    if key + "#dict" in g:
        return {str(k): _unflat(g, key + "/" + str(k)) for k in g[key + "#dict"]}
    if key + "#batch" in g:
        from teb_local_planner_amd import _abi
        count, stride = (int(v) for v in g[key + "#batch"])
        b = _abi.TebBatchHost(count, stride)
        for k in ("n", "x", "y", "theta", "dt", "has_vel_start", "vel_start", "has_vel_goal", "vel_goal", "prefer_rotdir", "via_points_enabled"):
            setattr(b, k, g[key + "/" + k].copy())
        return b
    if key + "#ragged" in g:
        off, v = g[key + "#ragged"], g[key + "/values"]
        return [v[off[i]:off[i + 1]].tolist() for i in range(len(off) - 1)]
    for tag, ty in (("#tuple", tuple), ("#list", list)):
        if key + tag in g:
            return ty(_unflat(g, "%s/%d" % (key, i)) for i in range(int(g[key + tag])))
    if key + "#none" in g:
        return None
    a = g[key]
    return a[()] if a.ndim == 0 else a.copy()


def main():
    """Records the reference's calls of the tests below (needs oracle/_ref) into ref_replay_<group>.npz."""
    root = os.path.dirname(os.path.dirname(HERE))
    for p in (root, os.path.dirname(HERE)):
        if p not in sys.path:
            sys.path.insert(0, p)
    from oracle import oracle_py, ref_py
    assert ref_py.available(), "oracle/_ref is not built"
    oracle_py.build()
    import test_reference_pinning as P
    import test_feasibility_oracle as F
    import ref_replay as M   # the module the tests use (this file runs as __main__)
    M.RECORD = RECORD = {}
    P.test_reference_unit_tests_on_reference_implementation()
    for seed in range(40):
        P.test_f1_f2_randomized_strip_functions_are_bit_equal_to_reference_code(oracle_py, seed)
        P.test_randomized_optimizeTEB_is_bit_equal_to_reference_code(oracle_py, seed)
        try:
            P.test_f3_randomized_candidate_generation_is_bit_equal_to_reference_code(oracle_py, seed)
        except BaseException as e:   # pytest.skip ("path enumeration bounded") comes after the reference's call: the recording stands
            if type(e).__name__ != "Skipped":
                raise
    for seed in range(0, 80, 4):
        for mode in (2, 3):
            P.test_f3_randomized_h_signatures_are_bit_equal_to_reference_code(oracle_py, mode, seed)
    for seed in range(60):
        F.test_oracle_equals_reference_code(seed)
    for group, cases in sorted(RECORD.items()):
        out = {}
        for case, calls in cases.items():
            out[case + "#calls"] = np.array(len(calls))
            for i, (name, value) in enumerate(calls):
                out["%s/%d#method" % (case, i)] = np.array(name)
                _flat(value, "%s/%d" % (case, i), out)
        path = os.path.join(HERE, "ref_replay_%s.npz" % group)
        np.savez_compressed(path, **out)
        print(path, len(cases), "cases", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
