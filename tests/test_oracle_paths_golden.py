"""The CPU oracle against the reference's own runs AT THE PATH ROWS
(tests/golden/paths_*.json, recorded by tests/golden/make_golden_paths.py from
the reference's functions on every row of dpll_paths.py, dp_paths.py,
res_paths.py and cdcl_paths.py, the scan-class rows and the batched rows).

tests/test_oracle_golden.py pins the oracle to the reference at small random
and bench-shaped formulas; the paths tests pin the kernels to the oracle at
the rows.  These tests join the two: past one resize of a CPython set, under a
caller's dict, at a snapshot's stopping point, the oracle is held to what the
reference did, not to a second restatement of it.

A fixture entry holds the hash of the formula the reference ran on, so a row
edited since fails here until its fixture is regenerated.  A row the reference
did not finish holds the steps / passes it completed ("complete": false) or,
for DPLL and CDCL, nothing; the cap on rows without data is asserted on the
committed files.  Nothing here reads the reference."""
import os

import pytest

import cdcl_paths
import dp_batch_rows
import dp_paths
import dpll_paths
import oracle
import paths_rows as R
import res_paths
import scan_cores
from conftest import clause_set_sha

CTR5 = ("nodes", "decisions", "unit_props", "pure_assigns", "conflicts")


FX = {s: R.load(os.path.join(R.HERE, "golden"), s) for s in R.FIXTURES}


@pytest.fixture(scope="module")
def fx():
    return FX


# the rows with reference data (the others are counted by test_committed_fixtures_meet_the_cap);
# a row added since is test_every_row_has_an_entry_of_its_formula's to report
DPLL_DATA = [n for n in R.dpll_rows() if FX["dpll"]["rows"].get(n, {}).get("data") is not None]
SCAN_DATA = [(c, N) for c, N in R.scan_rows() if FX["dpll"]["scan"]["rows"].get(f"{c}-{N}", {}).get("data") is not None]
DP_DATA = [n for n in R.dp_rows() if n in FX["dp"]["rows"] and R.dp_has_data(FX["dp"]["rows"][n])]
RES_DATA = [n for n in sorted({R.res_base(n) for n in R.res_rows()})
            if n in FX["res"]["rows"] and (FX["res"]["rows"][n]["passes"] or FX["res"]["rows"][n]["complete"])]
CDCL_DATA = [n for n in R.cdcl_rows() if FX["cdcl"]["rows"].get(n, {}).get("data") is not None]


# ---------------------------------------------------------------- rows and fixtures in step

def test_every_row_has_an_entry_of_its_formula(fx):
    bad = []
    for names, rows, sha in ((R.dpll_rows(), fx["dpll"]["rows"], R.dpll_row_sha), (R.dp_rows(), fx["dp"]["rows"], R.dp_row_sha),
                             (R.cdcl_rows(), fx["cdcl"]["rows"], R.cdcl_row_sha)):
        assert sorted(rows) == sorted(names)
        bad += [n for n in names if rows[n]["formula_sha"] != sha(n)]
    rows = fx["res"]["rows"]
    assert sorted(rows) == sorted(R.res_rows())
    for n in R.res_rows():
        e = rows[n]
        assert e.get("same_as", n) == R.res_base(n), n
        if rows[R.res_base(n)]["formula_sha"] != R.res_row_sha(n):
            bad.append(n)
    scan = fx["dpll"]["scan"]
    assert sorted(scan["rows"]) == sorted(f"{c}-{N}" for c, N in R.scan_rows())
    bad += [f"{c}-{N}" for c, N in R.scan_rows() if scan["rows"][f"{c}-{N}"]["formula_sha"] != R.scan_row_sha(c, N)]
    for c in scan_cores.CORES:
        fs = scan_cores.core_formulas(c)
        assert len(scan["cores"][c]) == len(fs)
        bad += [f"core {c}[{b}]" for b, f in enumerate(fs) if scan["cores"][c][b]["formula_sha"] != R.formula_sha(f)]
    for kind, sets in (("dp", R.dp_batch_sets()), ("res", R.res_batch_sets())):
        assert sorted(fx["batch"][kind]) == sorted(sets)
        bad += [f"batch {kind} {n}" for n, fs in sets.items() if fx["batch"][kind][n]["formula_sha"] != R.batch_set_sha(fs)]
    assert not bad, f"rows changed since their fixtures were recorded (run tests/golden/make_golden_paths.py): {bad}"


def _res_entry(rows, n):
    return rows[R.res_base(n)]


def test_committed_fixtures_meet_the_cap(fx):
    """Per solver at most one row in five without reference data, and every
    named group of a paths module keeps a row with data."""
    d, p, r, c = (fx[s]["rows"] for s in ("dpll", "dp", "res", "cdcl"))
    scan = fx["dpll"]["scan"]["rows"]
    bad = R.check_cap("dpll", R.dpll_rows(), lambda n: d[n]["data"] is not None, R.dpll_groups())
    bad += R.check_cap("scan", list(scan), lambda n: scan[n]["data"] is not None, {})
    bad += R.check_cap("dp", R.dp_rows(), lambda n: R.dp_has_data(p[n]), R.dp_groups())
    bad += R.check_cap("res", R.res_rows(), lambda n: len(_res_entry(r, n)["passes"]) > 0 or _res_entry(r, n)["complete"],
                       R.res_groups())
    bad += R.check_cap("cdcl", R.cdcl_rows(), lambda n: c[n]["data"] is not None, {"CDCL_PATH_ROWS": R.cdcl_rows()})
    for kind in ("dp", "res"):
        bad += [f"batch {kind} {n}" for n, e in fx["batch"][kind].items() if not e["complete"]]
    verdicts = set()
    for core, inst in fx["dpll"]["scan"]["cores"].items():
        if not any(e["data"] is not None for e in inst):
            bad.append(f"core {core}: no instance with reference data")
        verdicts |= {e["data"]["sat"] for e in inst if e["data"] is not None}
    assert verdicts == {True, False}   # (the exhausted trees the reference finished in its budget are cores B's and C's)
    assert not bad, bad


# ---------------------------------------------------------------- DPLL

@pytest.mark.parametrize("name", DPLL_DATA)
def test_dpll_row_matches_reference(fx, name):
    """Solutions with their dict order, the six counters and the caller's dict
    after the call.  The reference has no node limit, so neither has this run
    of the oracle (the row's own limit is the kernel tests' knob)."""
    e = fx["dpll"]["rows"][name]
    k = dpll_paths.row(name)[2]
    assert (e["mode"], e["sol_cap"]) == (k["mode"], k["sol_cap"])
    o = oracle.dpll(dpll_paths.row_formula(name), k["mode"], max_solutions=0, node_limit=0, init=k["init"],
                    sol_cap=k["sol_cap"])
    want = e["data"]
    assert o["status"] == 0
    assert o["counters"] == want["counters"]
    got = R.dpll_solutions_digest(o["solutions"])
    assert got["first_solution"] == want["first_solution"]
    assert got == {k: want[k] for k in got}
    assert o["counters"]["solutions"] - len(o["solutions"]) == want["solutions_beyond_cap"]
    if want["init_after"] is not None:
        assert o["root_assign"] == want["init_after"]


def _first_model(o):
    return {"sat": o["counters"]["solutions"] > 0, "counters": {k: o["counters"][k] for k in CTR5},
            "model": o["solutions"][0] if o["solutions"] else None}


@pytest.mark.parametrize("core", list(scan_cores.CORES))
def test_scan_core_instances_match_reference(fx, core):
    """The first-model SOUND search of every core instance the reference
    finished: verdict, counters, first model."""
    inst = fx["dpll"]["scan"]["cores"][core]
    base = scan_cores.core_oracle(core)
    n = 0
    for b, e in enumerate(inst):
        if e["data"] is not None:
            assert _first_model(base[b]) == e["data"], (core, b)
            n += 1
    assert n > 0


@pytest.mark.parametrize("core,N", SCAN_DATA, ids=[f"{c}-{N}" for c, N in SCAN_DATA])
def test_scan_row_matches_reference(fx, core, N):
    """One instance of the row's batch, renamed into 1..N, as the reference
    searched it -- and that search is the core's under the renaming, which is
    what lets test_scan_core_instances_match_reference speak for the row's
    other instances."""
    e = fx["dpll"]["scan"]["rows"][f"{core}-{N}"]
    img, fs = R.scan_row_formulas(core, N)
    o = oracle.dpll(fs[e["instance"]], "sound", max_solutions=1, sol_cap=1)
    assert _first_model(o) == e["data"]
    base = fx["dpll"]["scan"]["cores"][core][e["instance"]]["data"]
    assert base is not None and base["counters"] == e["data"]["counters"]
    assert e["data"]["model"] == (scan_cores.rename([base["model"]], img)[0] if base["sat"] else None)


# ---------------------------------------------------------------- Davis-Putnam

@pytest.mark.parametrize("name", DP_DATA)
def test_dp_row_matches_reference(fx, name):
    """The popped variable of every step and the clause list after it (clause
    order, each clause in its set's iteration order) over the steps the
    reference completed, up to the row's own step limit; the verdict where the
    reference finished and the row runs to its verdict."""
    R.dp_check(fx["dp"]["rows"][name], dp_paths.row_oracle(name), dp_paths.ROWS[name][1])


# ---------------------------------------------------------------- resolution

@pytest.mark.parametrize("name", RES_DATA)
def test_resolution_row_matches_reference(fx, name):
    """Every pass's new-clause set over the passes the reference completed, the
    verdict where it finished; a row that carries its own expected first pass
    (the product and pair-buffer rows) also against the reference's."""
    e = fx["res"]["rows"][name]
    f, want = res_paths.row(name)
    n = R.res_passes_compared(e, len(f))
    o = oracle.resolution(f, max_passes=0 if e["complete"] else n, record=True, rec_cap=1 << 23)
    if e["complete"]:
        assert o["result"] == int(e["result"])
        assert o["passes"] in (n, n + 1)   # (the pass that adds nothing is counted, not recorded, by the reference's observer)
    else:
        assert o["passes"] == n
    assert o["pass_new"][:n] == [p["count"] for p in e["passes"][:n]] and not any(o["pass_new"][n:])
    for k, p in enumerate(e["passes"][:n]):
        assert clause_set_sha(o["clauses"][k]) == p["sha256"], (name, k)
        if "clauses" in p:
            assert sorted(sorted(c) for c in o["clauses"][k]) == p["clauses"], (name, k)
    if want is not None:
        assert n >= 1 and len(want) == e["passes"][0]["count"] and clause_set_sha(want) == e["passes"][0]["sha256"]


# ---------------------------------------------------------------- CDCL

@pytest.mark.parametrize("name", CDCL_DATA)
def test_cdcl_row_matches_reference(fx, name):
    """Every field test_cdcl_matches_reference_class compares."""
    e = fx["cdcl"]["rows"][name]
    c, r = e["data"], cdcl_paths.row_oracle(name)
    assert c["max_iter"] == e["max_iter"] == next(x for x in cdcl_paths.CDCL_PATH_ROWS if x[0] == name)[2]
    assert r["result"] == c["result"]
    assert r["assignment"] == c["assignment"]
    assert r["var_inc"] == c["var_inc"]
    assert r["stats"]["level"] == c["level"]
    assert r["stats"]["clauses"] == c["clauses"] and r["stats"]["watch_keys"] == c["watch_keys"]
    for k in ("iterations", "conflicts", "decisions", "learned"):
        assert r["stats"][k] == c["stats"][k], k


# ---------------------------------------------------------------- batched rows

@pytest.mark.parametrize("name", list(R.dp_batch_sets()))
def test_dp_batch_rows_match_reference(fx, name):
    """The reference's verdict of every formula: the oracle's, and the
    frozenset restatement's of dp_batch_rows.model wherever its slot rule
    yields a variable at every step."""
    e = fx["batch"]["dp"][name]
    fs = R.dp_batch_sets()[name]
    assert e["complete"] and len(e["verdicts"]) == len(fs)
    restated = 0
    for f, v in zip(fs, e["verdicts"]):
        assert oracle.dp(f)["result"] == v, f
        m = dp_batch_rows.model(f)["result"]
        if m is not None:
            assert m == v, f
            restated += 1
    assert restated >= len(fs) - 2   # (the collision rows are handed back: edge has one, slot two)


@pytest.mark.parametrize("name", list(R.res_batch_sets()))
def test_res_batch_rows_match_reference(fx, name):
    e = fx["batch"]["res"][name]
    fs = R.res_batch_sets()[name]
    assert e["complete"] and len(e["verdicts"]) == len(fs)
    for f, v in zip(fs, e["verdicts"]):
        assert oracle.resolution(f)["result"] == v, f
