"""Golden vectors at the PATH ROWS: the reference's own functions run on every
row of tests/dpll_paths.py, dp_paths.py, res_paths.py and cdcl_paths.py, on the
scan-class rows of tests/test_dpll_gpu.py and on the batched rows
(tests/dp_batch_rows.py, tests/res_batch_rows.py).

Run here (the container that holds /root/reference), after the oracle library
is built (the row modules import it; nothing recorded comes from it):
    python tests/golden/make_golden_paths.py [dpll|dp|res|cdcl|batch ...]

The committed files come from `python tests/golden/make_golden_paths.py` on 8
cores (CPython 3.10.12), run solver by solver (`... make_golden_paths.py dpll`
and so on): dpll + scan 6 minutes of wall clock, dp 6, res 3, cdcl and batch
a few seconds.  Wall-clock budgets make a prefix row's length differ from run
to run; everything recorded is the reference's and any run's files pass the
tests.

The reference is loaded and observed by the existing generators, imported:
make_golden.py (dpll_optimized with a caller's dict, davis_putnam_solver:
`ast` loader, `sys.settrace` observers; resolution_solver under
make_golden_bench.py's `sys.setprofile` observation, observe_resolution
below), make_golden_sound.py (dpll_optimized with the branch statements rewritten: SOUND mode) and
make_golden_cdcl.py (CDCLSolver under its iteration bound).  Plain-data JSON
only, no reference text; bytecode caching is off.

Every row runs in a pool of at most 16 processes under ROW_BUDGET_S of wall
clock.  The budget decides only how much data there is:
  * Davis-Putnam steps and resolution passes are observed as they happen, so
    a row that runs out of time keeps the steps / passes it completed and is
    marked "complete": false;
  * a DPLL or CDCL row that does not finish records nothing ("data": null).
The cap on rows without data (tests/paths_rows.py check_cap) is checked here
and again by tests/test_oracle_paths_golden.py on the committed files.

What is stored
  paths_dpll.json   rows: mode, the first sol_cap solutions in dict order (the
                    first in full, all of them by one sha256), the count
                    beyond, the six counters, the caller's dict after the
                    call.  scan: per core instance (tests/scan_cores.py)
                    verdict, counters and first model of the SOUND reference
                    stopped at its first model; per (core, N) row the same
                    for one instance RENAMED into 1..N (dpll_optimized holds
                    no container ordered by a variable's hash, so its search
                    is the core's under the renaming: asserted here on that
                    instance, and what lets the other instances' records
                    stand for the row).
  paths_dp.json     the popped variable of every step; the clause list after
                    every completed step (clause order, each set's iteration
                    order) as count, literal count and sha256 -- the first
                    steps one by one (FULL_STEPS of them in full where small),
                    all of them folded into one sha256 (paths_rows.dp_digest;
                    at most DP_REC_STEPS steps are kept).
  paths_res.json    per pass the new-clause set, canonical: count and sha256,
                    in full where small.
  paths_cdcl.json   the fields of cdcl_ref.json.
  paths_batch.json  the reference's verdict per formula of each batched set.
"""
import json
import multiprocessing as mp
import os
import signal
import sys
import time

sys.dont_write_bytecode = True

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [HERE, os.path.join(ROOT, "tests"), os.path.join(ROOT, "sat-mpi-stana-andrei_amd"),
                os.path.join(ROOT, "oracle")]

ROW_BUDGET_S = 90.0       # wall clock per row
POOL = 16                 # processes, at most
FULL_STEPS = 4            # Davis-Putnam: steps stored in full ...
FULL_LITS = 200           # ... where the list has at most this many literals
FULL_CLAUSES = 120        # resolution: a pass stored in full up to this many clauses

import make_golden as mg            # noqa: E402  (loads the reference functions)
import make_golden_bench as mb      # noqa: E402  (the hashes of dp_php65.json / resolution_php43.json)
import make_golden_cdcl as mc       # noqa: E402
import make_golden_sound as ms      # noqa: E402
import paths_rows as R              # noqa: E402


class Deadline(BaseException):
    """Raised by the alarm around make_golden_cdcl.run_cdcl, which catches Exception."""


# ---------------------------------------------------------------- one row each

def job_dpll(name):
    import dpll_paths
    _, _, k, _ = dpll_paths.row(name)
    f = dpll_paths.row_formula(name)
    init = None
    if k["init"] is not None:
        init = {}
        for x in k["init"]:
            init[abs(x)] = x > 0
    entry = {"formula_sha": R.dpll_row_sha(name), "mode": k["mode"], "sol_cap": k["sol_cap"], "complete": False,
             "data": None}
    if k["mode"] == dpll_paths.REF:
        c = mg.dpll_case(f, init, seconds=ROW_BUDGET_S)
        if c is not None:
            sols = c["solutions"]
            entry["data"] = {**R.dpll_solutions_digest(sols[:k["sol_cap"]]), "solutions_beyond_cap": max(0, len(sols) - k["sol_cap"]),
                             "counters": dict(c["counters"], solutions=len(sols)),
                             "init_after": c.get("init_after")}
    else:
        c = ms.run_sound(f, ROW_BUDGET_S, init=init, sol_cap=k["sol_cap"])
        if "full" in c:
            n = c["full"]["solutions"]
            entry["data"] = {**R.dpll_solutions_digest(c["full"]["solution_list"]), "solutions_beyond_cap": max(0, n - k["sol_cap"]),
                             "counters": dict(c["full"]["counters"], solutions=n),
                             "init_after": c.get("init_after")}
    entry["complete"] = entry["data"] is not None
    return entry


def _first_model(f):
    c = ms.run_sound(f, ROW_BUDGET_S, first_only=True)
    if "first" not in c:
        return None
    return {"sat": c["first"]["model"] is not None, "counters": c["first"]["counters"], "model": c["first"]["model"]}


def job_scan_core(key):
    import scan_cores
    core, b = key
    f = scan_cores.core_formulas(core)[b]
    return {"formula_sha": R.formula_sha(f), "data": _first_model(f)}


def job_scan_row(key):
    """Instance b of the row's batch, renamed into 1..N (main() picks b: the
    core instance the reference searched with the fewest calls)."""
    core, N, b = key
    img, fs = R.scan_row_formulas(core, N)
    return {"formula_sha": R.scan_row_sha(core, N), "instance": b, "data": _first_model(fs[b])}


def job_dp(name):
    import dp_paths
    f = dp_paths.row_formula(name)
    res, obs = mg.run_traced("davis_putnam_solver", f, ROW_BUDGET_S)
    done = res is not mg.Timeout
    return dict({"formula_sha": R.dp_row_sha(name), "complete": done, "result": bool(res) if done else None},
                **R.dp_digest([s["var"] for s in obs["dp_steps"]], [s["clauses"] for s in obs["dp_steps"] if "clauses" in s],
                              step_limit=dp_paths.ROWS[name][1], full_steps=FULL_STEPS, full_lits=FULL_LITS))


def observe_resolution(f, seconds):
    """resolution_solver on a copy of f, observed as make_golden_bench.py
    observes PHP(4,3): `sys.setprofile`, where only C-function calls fire, and
    REF.py:94 `seen.update(new_clauses)` is the one `update` the resolution
    frame makes -- the pair loops run untraced (abuf's first pass is 2.2e7
    pairs, beyond the budget under make_golden.run_traced's line tracer).
    Returns (verdict or mg.Timeout, the canonical new-clause set of every
    completed pass)."""
    fn = mg.NS["resolution_solver"]
    code = fn.__code__
    got = []

    def prof(frame, event, arg):
        if event == "c_call" and frame.f_code is code and getattr(arg, "__name__", "") == "update":
            got.append(sorted(sorted(c) for c in frame.f_locals["new_clauses"]))

    signal.signal(signal.SIGALRM, mg._alarm)
    signal.setitimer(signal.ITIMER_REAL, seconds)
    sys.setprofile(prof)
    try:
        res = fn([list(c) for c in f])
    except mg.Timeout:
        res = mg.Timeout
    finally:
        sys.setprofile(None)
        signal.setitimer(signal.ITIMER_REAL, 0)
    return res, got


def job_res(name):
    import res_paths
    f, _ = res_paths.row(name)
    res, got = observe_resolution(f, ROW_BUDGET_S)
    passes = []
    for p in got:
        e = {"count": len(p), "sha256": mb.canon_sha(p)}
        if len(p) <= FULL_CLAUSES:
            e["clauses"] = p
        passes.append(e)
    done = res is not mg.Timeout
    return {"formula_sha": R.res_row_sha(name), "complete": done, "result": bool(res) if done else None,
            "passes": passes}


def _deadline(signum, frame):
    raise Deadline()


def job_cdcl(name):
    import cdcl_paths
    row = next(r for r in cdcl_paths.CDCL_PATH_ROWS if r[0] == name)
    entry = {"formula_sha": R.cdcl_row_sha(name), "max_iter": row[2], "complete": False, "data": None}
    signal.signal(signal.SIGALRM, _deadline)
    signal.setitimer(signal.ITIMER_REAL, ROW_BUDGET_S)
    try:
        c = mc.run_cdcl(cdcl_paths.row_formula(name), row[2])
        del c["formula"]
        entry.update(complete=True, data=c)
    except Deadline:
        sys.settrace(None)
    finally:
        signal.setitimer(signal.ITIMER_REAL, 0)
    return entry


def job_batch(key):
    """The reference's verdict of every formula of one batched set (one budget
    per set; the formulas are tiny)."""
    kind, name = key
    fs = (R.dp_batch_sets() if kind == "dp" else R.res_batch_sets())[name]
    fn = mg.NS["davis_putnam_solver" if kind == "dp" else "resolution_solver"]
    signal.signal(signal.SIGALRM, _deadline)
    signal.setitimer(signal.ITIMER_REAL, ROW_BUDGET_S)
    verdicts = []
    try:
        for f in fs:
            verdicts.append(int(bool(fn([list(c) for c in f]))))
    except Deadline:
        pass
    finally:
        signal.setitimer(signal.ITIMER_REAL, 0)
    return {"formula_sha": R.batch_set_sha(fs), "count": len(fs), "complete": len(verdicts) == len(fs),
            "verdicts": verdicts}


JOBS = {"dpll": job_dpll, "scan_core": job_scan_core, "scan_row": job_scan_row, "dp": job_dp, "res": job_res,
        "cdcl": job_cdcl, "batch": job_batch}


def _run(job):
    kind, key = job
    sys.setrecursionlimit(200000)   # the reference recurses once per decision and pure-literal round
    t = time.time()
    out = JOBS[kind](key)
    return kind, key, out, time.time() - t


def _pool_run(jobs):
    out = {}
    with mp.get_context("fork").Pool(min(POOL, os.cpu_count() or 1), maxtasksperchild=1) as pool:
        for kind, key, entry, dt in pool.imap_unordered(_run, jobs, chunksize=1):
            out[(kind, key if not isinstance(key, list) else tuple(key))] = entry
            print("  %-9s %-28s %6.1f s" % (kind, key, dt), flush=True)
    return out


def _write(solver, body, meta):
    path = os.path.join(HERE, R.FIXTURES[solver])
    with open(path, "w") as fh:
        json.dump(dict({"meta": meta}, **body), fh, separators=(",", ":"))
    size = os.path.getsize(path)
    assert size < 1 << 20, (path, size)
    print(f"{path}: {size} bytes")


def _report(solver, rows, state):
    by = {"complete": [], "prefix": [], "no data": []}
    for n in rows:
        by[state(n)].append(n)
    for k, v in by.items():
        print(f"{solver}: {len(v)} {k}: {' '.join(map(str, v))}")


def main():
    which = sys.argv[1:] or list(R.FIXTURES)
    meta = {"generator": "tests/golden/make_golden_paths.py", "python": sys.version.split()[0],
            "reference": os.path.basename(mg.REF_FILE), "row_budget_s": ROW_BUDGET_S}
    t0 = time.time()
    bad = []

    if "dpll" in which:
        import scan_cores
        cores = [(c, b) for c in scan_cores.CORES for b in range(scan_cores.CORES[c][0])]
        got = _pool_run([("scan_core", k) for k in cores] + [("dpll", n) for n in R.dpll_rows()])
        # a row's renamed instance: the core instance the reference searched with the fewest calls
        pick = {}
        for c in scan_cores.CORES:
            done = [(got[("scan_core", (c, b))]["data"]["counters"]["nodes"], b)
                    for b in range(scan_cores.CORES[c][0]) if got[("scan_core", (c, b))]["data"] is not None]
            pick[c] = min(done)[1] if done else 0
        got.update(_pool_run([("scan_row", (c, N, pick[c])) for c, N in R.scan_rows()]))
        rows = {n: got[("dpll", n)] for n in R.dpll_rows()}
        scan = {"cores": {c: [got[("scan_core", (c, b))] for b in range(scan_cores.CORES[c][0])] for c in scan_cores.CORES},
                "rows": {}}
        for c, N in R.scan_rows():
            e = got[("scan_row", (c, N, pick[c]))]
            base = scan["cores"][c][pick[c]]["data"]
            if e["data"] is not None and base is not None:   # the reference's search is the core's, renamed
                img = R.scan_row_formulas(c, N)[0]
                assert e["data"]["counters"] == base["counters"] and e["data"]["sat"] == base["sat"], (c, N)
                assert e["data"]["model"] == (scan_cores.rename([base["model"]], img)[0] if base["sat"] else None), (c, N)
            scan["rows"][f"{c}-{N}"] = e
        _write("dpll", {"rows": rows, "scan": scan}, meta)
        _report("dpll", R.dpll_rows(), lambda n: "complete" if rows[n]["complete"] else "no data")
        _report("scan cores", cores, lambda k: "complete" if got[("scan_core", k)]["data"] is not None else "no data")
        _report("scan rows", list(scan["rows"]), lambda n: "complete" if scan["rows"][n]["data"] is not None else "no data")
        bad += R.check_cap("dpll", R.dpll_rows(), lambda n: rows[n]["complete"], R.dpll_groups())
        bad += R.check_cap("scan", list(scan["rows"]), lambda n: scan["rows"][n]["data"] is not None, {})

    if "dp" in which:
        got = _pool_run([("dp", n) for n in sorted(R.dp_rows(), key=lambda n: -len(R.dp_paths.row_formula(n)))])
        rows = {n: got[("dp", n)] for n in R.dp_rows()}
        _write("dp", {"rows": rows}, meta)
        _report("dp", R.dp_rows(), lambda n: "complete" if rows[n]["complete"] else
                "prefix" if rows[n]["lists"] else "no data")
        bad += R.check_cap("dp", R.dp_rows(), lambda n: rows[n]["complete"] or rows[n]["lists"] > 0, R.dp_groups())

    if "res" in which:
        bases = sorted({R.res_base(n) for n in R.res_rows()}, key=lambda n: -len(R.res_paths.row(n)[0]))
        got = _pool_run([("res", n) for n in bases])
        rows = {n: (got[("res", n)] if n == R.res_base(n) else {"same_as": R.res_base(n)}) for n in R.res_rows()}
        _write("res", {"rows": rows}, meta)
        ent = lambda n: got[("res", R.res_base(n))]   # noqa: E731
        _report("res", R.res_rows(), lambda n: "complete" if ent(n)["complete"] else "prefix" if ent(n)["passes"] else "no data")
        bad += R.check_cap("res", R.res_rows(), lambda n: ent(n)["complete"] or len(ent(n)["passes"]) > 0, R.res_groups())

    if "cdcl" in which:
        got = _pool_run([("cdcl", n) for n in R.cdcl_rows()])
        rows = {n: got[("cdcl", n)] for n in R.cdcl_rows()}
        _write("cdcl", {"rows": rows}, meta)
        _report("cdcl", R.cdcl_rows(), lambda n: "complete" if rows[n]["complete"] else "no data")
        bad += R.check_cap("cdcl", R.cdcl_rows(), lambda n: rows[n]["complete"], {"CDCL_PATH_ROWS": R.cdcl_rows()})

    if "batch" in which:
        keys = [("dp", n) for n in R.dp_batch_sets()] + [("res", n) for n in R.res_batch_sets()]
        got = _pool_run([("batch", k) for k in keys])
        body = {"dp": {n: got[("batch", ("dp", n))] for n in R.dp_batch_sets()},
                "res": {n: got[("batch", ("res", n))] for n in R.res_batch_sets()}}
        _write("batch", body, meta)
        _report("batch", keys, lambda k: "complete" if got[("batch", k)]["complete"] else
                "prefix" if got[("batch", k)]["verdicts"] else "no data")
        bad += R.check_cap("batch", keys, lambda k: got[("batch", k)]["complete"], {})

    print("%.0f s" % (time.time() - t0))
    if bad:
        print("THE CAP ON ROWS WITHOUT DATA IS MISSED:\n  " + "\n  ".join(bad))
        sys.exit(1)


if __name__ == "__main__":
    main()
