"""Every row of the four paths modules, the scan-class rows and the batched rows
under one naming, with each row's formula hash and its named groups: what
tests/golden/make_golden_paths.py runs the reference on, and what
tests/test_oracle_paths_golden.py and tests/test_paths_reference_gpu.py look
up in tests/golden/paths_*.json.

A fixture entry carries `formula_sha` (formula_sha below) of the formula the
reference was run on; a row whose formula has changed since no longer matches
its entry.  The cap on rows without reference data (check_cap): per solver at
most one row in five, and every named group keeps a row with data.
"""
import hashlib
import json
import os
import re

import cdcl_paths
import dp_batch_rows
import dp_paths
import dpll_paths
import res_batch_rows
import res_paths
import scan_cores

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURES = {"dpll": "paths_dpll.json", "dp": "paths_dp.json", "res": "paths_res.json", "cdcl": "paths_cdcl.json",
            "batch": "paths_batch.json"}
MISSING_MAX = 0.2   # per solver: the share of rows that may be without reference data


def formula_sha(formula, *extra):
    """sha256 of a formula (clause and literal order kept) and whatever else
    decides the run (a caller's dict, a mode), as compact JSON."""
    s = json.dumps([[list(c) for c in formula]] + list(extra), separators=(",", ":"))
    return hashlib.sha256(s.encode()).hexdigest()


def load(golden_dir, solver):
    with open(os.path.join(golden_dir, FIXTURES[solver])) as fh:
        return json.load(fh)


# ---------------------------------------------------------------- DPLL

def dpll_rows():
    return [r[0] for r in dpll_paths.DPLL_PATH_ROWS]


def dpll_row_sha(name):
    k = dpll_paths.row(name)[2]
    return formula_sha(dpll_paths.row_formula(name), k["mode"], k["init"] or [])


def _sha(obj):
    return hashlib.sha256(json.dumps(obj, separators=(",", ":")).encode()).hexdigest()


def dpll_solutions_digest(sols):
    """A row's kept solutions as the fixture stores them: how many, the first in
    full, all of them (each in its dict order) by one sha256."""
    return {"solutions_kept": len(sols), "first_solution": sols[0] if sols else None,
            "solutions_sha": _sha([list(s) for s in sols])}


def dpll_groups():
    """The comment-delimited sections of DPLL_PATH_ROWS, read from the module's
    text (`# ---- title` opens a section; a row is a line that begins with its
    quoted name), and the module's own tuples."""
    text = open(os.path.join(HERE, "dpll_paths.py")).read()
    body = text[text.index("DPLL_PATH_ROWS = ["):text.index("LONG_ROWS = ")]
    groups, cur, names = {}, None, set(dpll_rows())
    for line in body.splitlines():
        m = re.match(r"\s*# ---- (.*)", line)
        if m:
            cur = m.group(1).strip()
            groups[cur] = []
            continue
        m = re.match(r"\s*\(\"(\w+)\",", line)
        if m and cur is not None and m.group(1) in names:   # (a continuation line opens with a counter's name)
            groups[cur].append(m.group(1))
    shape = next(k for k in groups if k.startswith("LDS shape classes"))
    groups[shape] = list(dpll_paths.SHAPE_ROWS)
    groups["LONG_ROWS"] = list(dpll_paths.LONG_ROWS)
    assert sorted(n for k, g in groups.items() if k != "LONG_ROWS" for n in g) == sorted(dpll_rows()), "a row outside every section"
    return groups


def scan_rows():
    import test_dpll_gpu
    return [(r[0], r[1]) for r in test_dpll_gpu.SCAN_CLASS_ROWS]


def scan_row_formulas(core, N):
    img = scan_cores.renaming(core, N)
    return img, [scan_cores.rename(f, img) for f in scan_cores.core_formulas(core)]


def scan_row_sha(core, N):
    return formula_sha([c for f in scan_row_formulas(core, N)[1] for c in f])


# ---------------------------------------------------------------- Davis-Putnam

def dp_rows():
    return list(dp_paths.ROWS)


def dp_row_sha(name):
    return formula_sha(dp_paths.row_formula(name))


DP_REC_STEPS = 320    # steps of a Davis-Putnam run the fixture keeps (chain_300 whole)
DP_HEAD_STEPS = 4     # ... of which the first are stored one by one


def dp_digest(vars_, lists, step_limit=0, full_steps=0, full_lits=0):
    """A Davis-Putnam run as the fixture stores it and as the tests digest the
    oracle's and the kernel's: `vars` the popped variables, `lists` how many
    completed clause lists (both of the first DP_REC_STEPS steps, or of the
    row's own step_limit where that is fewer: the tests run no further), `head` the
    first DP_HEAD_STEPS lists as count, literal count and sha256 of the
    ordered list (in full up to step full_steps where a list has at most
    full_lits literals), `lists_sha` one sha256 over (count, literal count,
    sha256) of every one of the `lists` lists."""
    keep = min(DP_REC_STEPS, step_limit or DP_REC_STEPS)
    lists = lists[:keep]
    rows = [[len(cl), sum(len(c) for c in cl), _sha([list(c) for c in cl])] for cl in lists]
    head = []
    for k, (n, lits, sha) in enumerate(rows[:DP_HEAD_STEPS]):
        e = {"n": n, "lits": lits, "sha256": sha}
        if k < full_steps and lits <= full_lits:
            e["clauses"] = [list(c) for c in lists[k]]
        head.append(e)
    return {"vars": list(vars_[:keep]), "lists": len(rows), "head": head, "lists_sha": _sha(rows)}


def dp_has_data(e):
    return e["complete"] or e["lists"] > 0


def dp_check(e, r, step_limit):
    """Assert that a run r (the oracle's or eliminate()'s dict of a recorded run
    under the row's step_limit) reproduces the fixture entry e: the popped
    variables and every clause list over the steps the reference completed,
    the first lists one by one, and the verdict where the reference finished
    a row that runs to its verdict."""
    assert len(r["vars"]) >= len(e["vars"]) >= 1 and len(r["clauses"]) >= e["lists"]
    got = dp_digest(r["vars"][:len(e["vars"])], r["clauses"][:e["lists"]], step_limit)
    assert got["vars"] == e["vars"]
    for k, (g, w) in enumerate(zip(got["head"], e["head"])):
        if "clauses" in w:
            assert r["clauses"][k] == w["clauses"], k
        assert g == {x: w[x] for x in ("n", "lits", "sha256")}, k
    assert (got["lists"], got["lists_sha"]) == (e["lists"], e["lists_sha"])
    if e["complete"] and step_limit == 0:
        assert r["result"] == int(e["result"]) and len(r["vars"]) == len(e["vars"])
    elif e["complete"]:
        assert r["result"] == (-1 if len(e["vars"]) == step_limit else int(e["result"]))


def dp_groups():
    P = dp_paths
    return {"KEY_WIDTH_ROWS": list(P.KEY_WIDTH_ROWS), "POPSET_ROWS": list(P.POPSET_ROWS),
            "FIRSTPOS_ROWS": list(P.FIRSTPOS_ROWS), "LARGE_ROWS": list(P.LARGE_ROWS),
            "WIDTH_CHANGE_SEQUENCE": sorted(set(P.WIDTH_CHANGE_SEQUENCE)), "RESUME_ROWS": list(P.RESUME_ROWS)}


# ---------------------------------------------------------------- resolution

def res_rows():
    """Every name res_paths.row() serves: the rows of PATHS, PRODUCT_ROWS and PAIRBUF_ROWS."""
    names = list(res_paths.PRODUCT_ROWS) + list(res_paths.PAIRBUF_ROWS)
    for rows in res_paths.PATHS.values():
        names += [n for n in rows if n not in names]
    names += [b for b in dict.fromkeys(map(res_base, names)) if b not in names]   # (chain40: named by its variants only)
    return names


def res_base(name):
    """The row whose formula `name` shares (limit_chain30 runs chain30's formula)."""
    for base in ("chain30", "chain40"):
        if name.endswith(base):
            return base
    return name


RES_COMPARE_MAX = 30000   # clauses: the tests replay a prefix row's recorded passes up to this list size


def res_passes_compared(entry, n0):
    """How many of a fixture entry's recorded passes the tests replay: all of a
    row the reference finished; of a prefix, those that keep the clause list
    (n0 input clauses) within RES_COMPARE_MAX -- a pass over n clauses is n^2 / 2
    pairs on the oracle's side too -- and never fewer than one."""
    counts = [p["count"] for p in entry["passes"]]
    if entry["complete"]:
        return len(counts)
    k, n = 0, n0
    while k < len(counts) and n + counts[k] <= RES_COMPARE_MAX:
        n += counts[k]
        k += 1
    return max(k, min(1, len(counts)))


def res_row_sha(name):
    return formula_sha(res_paths.row(name)[0])


def res_groups():
    g = {"PRODUCT_ROWS": list(res_paths.PRODUCT_ROWS), "PAIRBUF_ROWS": list(res_paths.PAIRBUF_ROWS)}
    g.update({path: list(rows) for path, rows in res_paths.PATHS.items()})
    return g


# ---------------------------------------------------------------- CDCL

def cdcl_rows():
    return [r[0] for r in cdcl_paths.CDCL_PATH_ROWS]


def cdcl_row_sha(name):
    row = next(r for r in cdcl_paths.CDCL_PATH_ROWS if r[0] == name)
    return formula_sha(cdcl_paths.row_formula(name), row[2])


# ---------------------------------------------------------------- batched rows

def dp_batch_sets():
    """name -> the formulas of a batched Davis-Putnam test (tests/dp_batch_rows.py)."""
    R = dp_batch_rows
    return {"edge": R.EDGE, "slot": [R.SLOT, R.SLOT37, R.COLLIDE0, R.COLLIDE1], "mix": R.mix(),
            "sparse_mix": R.sparse_mix(), "wave": [R.WAVE_ROWS[k] for k in R.WAVE_ROWS] + [R.D32],
            "capacity": R.capacity_rows()}


def res_batch_sets():
    return {"edge": res_batch_rows.EDGE, "mix": res_batch_rows.mix()}


def batch_set_sha(formulas):
    return formula_sha([c + [0] for f in formulas for c in f], [len(f) for f in formulas])


# ---------------------------------------------------------------- the cap

def check_cap(solver, rows, has_data, groups):
    """The list of what misses the cap: `rows` the solver's row names,
    `has_data(name)` whether the fixture holds reference data of it."""
    bad = []
    missing = [n for n in rows if not has_data(n)]
    if len(missing) > MISSING_MAX * len(rows):
        bad.append(f"{solver}: {len(missing)} of {len(rows)} rows without reference data: {missing}")
    for g, names in groups.items():
        if names and not any(has_data(n) for n in names):
            bad.append(f"{solver}: no row of group {g!r} has reference data")
    return bad
