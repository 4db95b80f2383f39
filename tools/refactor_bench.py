"""What the refactor benches share (tools/renew_refactor_bench.py, tools/handle_refactor_bench.py): a cell is run three times - the parent's library (TEB_AMD_LIB), this
build, the parent's again -, each in a process of its own under a time limit; a cell is level if this build lies no further above the
parent's slower run than the parent's two runs lie apart; every cell that is not gets a second pass in fresh processes. A process that
fails or passes its limit ends the run. The table is rewritten after every cell, so what is measured survives a later failure."""
import json
import os
import subprocess
import sys


def run_worker(script, args, lib, timeout_s):
    """One process of `script --worker args`: its last JSON line, or (None, why) when it failed or passed its limit."""
    env = dict(os.environ)
    if lib:
        env["TEB_AMD_LIB"] = os.path.abspath(lib)
    try:
        p = subprocess.run([sys.executable, os.path.abspath(script), "--worker"] + [str(a) for a in args], capture_output=True, text=True,
                           timeout=timeout_s, env=env)
    except subprocess.TimeoutExpired:
        return None, "passed its limit of %d s" % timeout_s
    done = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    if p.returncode != 0 or not done:
        sys.stderr.write(p.stdout + p.stderr)
        return None, "ended with status %d" % p.returncode
    return json.loads(done[-1]), None


def level(r):
    p1, t, p2 = r["parent1"]["ms"], r["this"]["ms"], r["parent2"]["ms"]
    return t <= max(p1, p2) + abs(p1 - p2)


def same(r, keys=("digest",)):
    return all(r["this"][k] == r["parent1"][k] == r["parent2"][k] for k in keys)


def three_way(script, cells, parent_lib, out, timeout_s, line, report, keys=("digest",)):
    """Runs the cells (argument tuples of the worker), then the second pass; report(rows, again, note) is the text of the table. Exits
    with a message when a process failed or a compared key differs from the parent's."""
    rows, again, note = [], [], None

    def three(cell, into):
        r = {}
        for key, lib in (("parent1", parent_lib), ("this", None), ("parent2", parent_lib)):
            r[key], why = run_worker(script, cell, lib, timeout_s)
            if why:
                return "%s (%s) %s: nothing more was started" % (cell, key, why)
        r["cell"] = cell
        into.append(r)
        print(line(r), flush=True)
        with open(out, "w") as fh:
            fh.write(report(rows, again, None))
        return None
    for cell in cells:
        note = three(cell, rows)
        if note:
            break
    if not note:
        for r in [r for r in rows if not level(r)]:
            note = three(r["cell"], again)
            if note:
                break
    text = report(rows, again, note)
    with open(out, "w") as fh:
        fh.write(text)
    print(text)
    if note:
        sys.exit(note)
    if not all(same(r, keys) for r in rows + again):
        sys.exit("a result differs from the parent's")


def summary(rows, again, keys=("digest",)):
    return "# %d cells, %d equal to the parent's, %d level in the first pass%s" % (
        len(rows), sum(same(r, keys) for r in rows), sum(level(r) for r in rows),
        (", %d of %d level in the second" % (sum(level(r) for r in again), len(again))) if again else "")
