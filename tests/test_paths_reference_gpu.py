"""GPU: the kernels against the REFERENCE's own runs at the path rows
(tests/golden/paths_*.json, tests/golden/make_golden_paths.py), directly: no
oracle stands between.  The paths tests hold every row bit-exact to the
oracle and tests/test_oracle_paths_golden.py holds the oracle to these
fixtures; this file closes the triangle with one run per row of the entry
point, the arguments and the storage forms the row's own GPU test uses, and
compares what the fixture holds: a row's whole run where the reference
finished it, the steps / passes it completed otherwise.  Rows without
reference data are not run here.  Reads tests/golden/ only."""
import os

import pytest

import cdcl_paths
import dp_paths
import dpll_paths
import paths_rows as R
import res_paths
import scan_cores
from conftest import clause_set_sha
from satmi import _capi
from satmi.cdcl import CDCL_ERROR, CDCL_LIMIT, CDCL_SAT, CDCL_UNSAT, cdcl_batch
from satmi.dp import eliminate, eliminate_batch
from satmi.dpll import dpll_batch
from satmi.resolution import resolve, resolve_batch

pytestmark = pytest.mark.gpu

FX = {s: R.load(os.path.join(R.HERE, "golden"), s) for s in R.FIXTURES}
CTR5 = ("nodes", "decisions", "unit_props", "pure_assigns", "conflicts")


# ---------------------------------------------------------------- DPLL

def _dpll_rows(names):
    """The rows of `names` the reference finished."""
    return [n for n in names if FX["dpll"]["rows"][n]["data"] is not None]


def _node_limit(rows):
    """The rows' own node limit where every reference search stays under it;
    0 (none) otherwise: the reference has no such limit (shape_4_waves, limit
    60, is a search of 75 calls)."""
    k = dpll_paths.row(rows[0])[2]
    under = all(FX["dpll"]["rows"][n]["data"]["counters"]["nodes"] < dpll_paths.row(n)[2]["node_limit"] for n in rows)
    return k["node_limit"] if under else 0


def _dpll_mismatches(names, policy):
    """One launch per mode of the rows `names`, each compared in its own mode."""
    bad = []
    for mode in ("ref", "sound"):
        rows = [n for n in names if dpll_paths.row(n)[2]["mode"] == mode]
        if not rows:
            continue
        k = dpll_paths.row(rows[0])[2]
        assert all((dpll_paths.row(n)[2]["node_limit"], dpll_paths.row(n)[2]["sol_cap"]) == (k["node_limit"], k["sol_cap"])
                   for n in rows)
        _capi.set_kernel(policy)
        try:
            r = dpll_batch([dpll_paths.row_formula(n) for n in rows], mode=mode, max_solutions=0,
                           node_limit=_node_limit(rows), sol_cap=k["sol_cap"],
                           inits=[dpll_paths.row(n)[2]["init"] or [] for n in rows])
        finally:
            _capi.set_kernel(_capi.KERNEL_AUTO)
        for b, n in enumerate(rows):
            want = FX["dpll"]["rows"][n]["data"]
            sols = R.dpll_solutions_digest(r.solutions(b))
            checks = [("status", int(r.status[b]), 0), ("counters", r.counter_dict(b), dict(r.counter_dict(b), **want["counters"])),
                      ("first solution", sols["first_solution"], want["first_solution"]),
                      ("solutions", sols, {k: want[k] for k in sols})]
            if want["init_after"] is not None:
                checks.append(("root assignment", r.root_assignment(b), want["init_after"]))
            bad += [f"policy {policy} {mode} {n}: {what} = {str(have)[:80]}, reference {str(ref)[:80]}"
                    for what, have, ref in checks if have != ref]
    return bad


MAIN = _dpll_rows([n for n in R.dpll_rows() if n not in dpll_paths.SHAPE_ROWS and n not in dpll_paths.LONG_ROWS])
LONG = _dpll_rows(["long_255"] + list(dpll_paths.LONG_ROWS))
SHAPE = _dpll_rows(list(dpll_paths.SHAPE_ROWS))


@pytest.mark.parametrize("policy", [_capi.KERNEL_GENERAL, _capi.KERNEL_WIDE], ids=["general", "wide"])
def test_dpll_rows_match_reference(policy):
    """The rows of test_rows_batched_match_oracle, one launch per mode in the
    LDS and in the wide form: solutions in dict order, six counters, the
    caller's dict after the call."""
    assert len(MAIN) >= 30
    bad = _dpll_mismatches(MAIN, policy)
    assert not bad, (len(bad), bad[:8])


@pytest.mark.parametrize("policy", [_capi.KERNEL_WIDE, _capi.KERNEL_AUTO], ids=["wide", "auto"])
def test_dpll_long_clause_rows_match_reference(policy):
    assert len(LONG) >= 2
    bad = _dpll_mismatches(LONG, policy)
    assert not bad, bad[:8]


@pytest.mark.parametrize("name", SHAPE)
def test_dpll_shape_row_matches_reference(name):
    """A shape row alone (its LDS class is its own launch's), both forms."""
    bad = _dpll_mismatches([name], _capi.KERNEL_GENERAL) + _dpll_mismatches([name], _capi.KERNEL_WIDE)
    assert not bad, bad[:8]


SCAN_DATA = [(c, N) for c, N in R.scan_rows() if FX["dpll"]["scan"]["rows"][f"{c}-{N}"]["data"] is not None]


@pytest.mark.parametrize("core,N", SCAN_DATA, ids=[f"{c}-{N}" for c, N in SCAN_DATA])
def test_scan_class_row_matches_reference(core, N):
    """The row's batch under the incremental and the plain scan kernel, unsplit
    (the split protocol is held to the unsplit search by
    test_scan_kernel_classes_decide_unsat): the instance the reference searched
    renamed into 1..N against that record, every other instance the reference
    finished on the core against the core's record mapped through the
    renaming."""
    from test_dpll_gpu import _run_split
    e = FX["dpll"]["scan"]["rows"][f"{core}-{N}"]
    inst = FX["dpll"]["scan"]["cores"][core]
    img, fs = R.scan_row_formulas(core, N)
    want = {}
    for b, c in enumerate(inst):
        if c["data"] is not None:
            d = c["data"]
            want[b] = (d["sat"], d["counters"], scan_cores.rename([d["model"]], img)[0] if d["sat"] else None)
    want[e["instance"]] = (e["data"]["sat"], e["data"]["counters"], e["data"]["model"])
    bad = []
    for kern in (_capi.KERNEL_INC, _capi.KERNEL_SCAN):
        r = _run_split(fs, False, kern, warmup=0, max_solutions=1, sol_cap=1)
        for b, (sat, ctr, model) in want.items():
            got = r.counter_dict(b)
            have = (got["solutions"] > 0, {k: got[k] for k in CTR5}, r.solutions(b)[0] if r.solutions(b) else None)
            if have != (sat, ctr, model):
                bad.append(f"kernel {kern} instance {b}: {str(have)[:120]}, reference {str((sat, ctr, model))[:120]}")
    assert not bad, bad[:8]


# ---------------------------------------------------------------- Davis-Putnam

DP_DATA = [n for n in R.dp_rows() if R.dp_has_data(FX["dp"]["rows"][n])]


@pytest.fixture(params=["pipeline", "inline"])
def dp_mode(request, monkeypatch):
    if request.param == "inline":
        monkeypatch.setenv("SATMI_DP_INLINE", "1")
    else:
        monkeypatch.delenv("SATMI_DP_INLINE", raising=False)
    return request.param


@pytest.mark.parametrize("name", DP_DATA)
def test_dp_row_matches_reference(name, dp_mode):
    """eliminate(record=True) under the row's step limit: the popped variables
    and every recorded list (clause order, each clause's set iteration order,
    by count, literal count and sha256; in full where the fixture is) over the
    steps the reference completed, the verdict where it finished."""
    step_limit = dp_paths.ROWS[name][1]
    R.dp_check(FX["dp"]["rows"][name], eliminate(dp_paths.row_formula(name), step_limit=step_limit, record=True), step_limit)


# ---------------------------------------------------------------- resolution

RES_DATA = [n for n in sorted({R.res_base(n) for n in R.res_rows()})
            if FX["res"]["rows"][n]["passes"] or FX["res"]["rows"][n]["complete"]]


@pytest.mark.parametrize("name", RES_DATA)
def test_resolution_row_matches_reference(name):
    """resolve(record=True) over the passes the reference completed: every
    pass's new-clause set, the verdict where the reference finished."""
    e = FX["res"]["rows"][name]
    f, _ = res_paths.row(name)
    n = R.res_passes_compared(e, len(f))
    r = resolve(f, max_passes=0 if e["complete"] else n, record=True, rec_cap=1 << 24)
    if e["complete"]:
        assert r["result"] == int(e["result"]) and r["passes"] in (n, n + 1)
    else:
        assert r["passes"] == n
    assert list(r["pass_new"][:n]) == [p["count"] for p in e["passes"][:n]] and not any(r["pass_new"][n:])
    for k, p in enumerate(e["passes"][:n]):
        assert clause_set_sha(r["clauses"][k]) == p["sha256"], (name, k)
        if "clauses" in p:
            assert sorted(sorted(c) for c in r["clauses"][k]) == p["clauses"], (name, k)


# ---------------------------------------------------------------- CDCL

CDCL_DATA = [n for n in R.cdcl_rows() if FX["cdcl"]["rows"][n]["data"] is not None]
STATUS = {1: CDCL_SAT, 0: CDCL_UNSAT, -1: CDCL_LIMIT, -2: CDCL_ERROR}


def test_cdcl_rows_match_reference():
    """Every row alone (the LDS placement) and, per iteration bound, all in one
    launch beside test_cdcl_paths_gpu's 420-variable filler (the arena
    placement): verdict and the assignment dict in insertion order; var_inc
    and the loop's counts too."""
    from test_cdcl_paths_gpu import filler, in_lds
    bad = []
    by_cap = {}
    for n in CDCL_DATA:
        by_cap.setdefault(FX["cdcl"]["rows"][n]["max_iter"], []).append(n)
    for cap, names in by_cap.items():
        fs = [cdcl_paths.row_formula(n) for n in names]
        assert all(in_lds([f]) for f in fs) and not in_lds(fs + [filler()])
        runs = [("lds", [cdcl_batch([f], max_iter=cap)[0] for f in fs]),
                ("arena", cdcl_batch(fs + [filler()], max_iter=cap)[:len(fs)])]
        for tag, rs in runs:
            for n, r in zip(names, rs):
                c = FX["cdcl"]["rows"][n]["data"]
                have = (r["status"], r["assignment"], r["var_inc"], r["stats"]["level"], r["stats"]["clauses"],
                        r["stats"]["watch_keys"]) + tuple(r["stats"][k] for k in ("iterations", "conflicts", "decisions", "learned"))
                want = (STATUS[c["result"]], c["assignment"], c["var_inc"], c["level"], c["clauses"], c["watch_keys"]) + \
                    tuple(c["stats"][k] for k in ("iterations", "conflicts", "decisions", "learned"))
                if have != want:
                    bad.append(f"{tag} {n}: {str(have)[:100]}, reference {str(want)[:100]}")
    assert len(CDCL_DATA) >= 15 and not bad, bad[:8]


# ---------------------------------------------------------------- batched rows

@pytest.mark.parametrize("name", list(R.dp_batch_sets()))
def test_dp_batch_verdicts_match_reference(name):
    fs = R.dp_batch_sets()[name]
    got = eliminate_batch(fs)
    assert [r["result"] for r in got] == FX["batch"]["dp"][name]["verdicts"]


@pytest.mark.parametrize("name", list(R.res_batch_sets()))
def test_res_batch_verdicts_match_reference(name):
    fs = R.res_batch_sets()[name]
    got = resolve_batch(fs)
    assert [r["result"] for r in got] == FX["batch"]["res"][name]["verdicts"]
