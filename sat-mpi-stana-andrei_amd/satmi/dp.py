"""Davis-Putnam elimination on the GPU (libsatmi.so, csrc/dp.hip, csrc/dp_batch.hip).

`eliminate(formula, ...)` runs REF.py:98-130 step by step -- variables in the
reference's own order (CPython's `set.pop()`, modelled on the device) -- and can
return every intermediate clause list; `davis_putnam_solve` is the reference's
boolean entry point.  `eliminate_batch` / `davis_putnam_solve_batch` run many small
formulas in one launch, one workgroup per formula.
"""
import ctypes

import numpy as np

from . import _batch, _capi
from ._batch import _csr, _p


class DavisPutnamLimit(Exception):
    """A step / clause / time limit stopped the elimination before a verdict."""


def eliminate(formula, step_limit=0, clause_limit=0, time_limit=0.0, record=False, rec_cap=1 << 22):
    """Returns {"result": 1 (True) | 0 (False) | -1 (limit), "vars": [eliminated
    variable per step], "steps": int, "clauses": [clause list after each completed
    step, every clause in its Python set iteration order] (record=True)}."""
    L = _capi.load()
    _capi.require_gpu()
    off, lits = _csr(formula)
    nv = max(int(np.abs(lits.astype(np.int64)).max()) if len(formula) and off[-1] else 1, 1)
    res = ctypes.c_int32(0)
    steps = ctypes.c_int32(0)
    trace = np.zeros(nv + 1, dtype=np.int32)
    if record:
        rl = np.zeros(rec_cap, dtype=np.int32)
        rco = np.zeros(rec_cap + 1, dtype=np.int64)
        rso = np.full(nv + 2, -1, dtype=np.int64)   # untouched (-1) for a step that ended the search
        rc = L.satmi_dp_host(len(formula), _p(off), _p(lits), int(step_limit), int(clause_limit), float(time_limit),
                             ctypes.byref(res), _p(trace), nv + 1, ctypes.byref(steps), _p(rl), rec_cap,
                             _p(rco, ctypes.c_int64), rec_cap + 1, _p(rso, ctypes.c_int64), nv + 2)
    else:
        rc = L.satmi_dp_host(len(formula), _p(off), _p(lits), int(step_limit), int(clause_limit), float(time_limit),
                             ctypes.byref(res), _p(trace), nv + 1, ctypes.byref(steps), None, 0, None, 0, None, 0)
    _capi.check(rc, "satmi_dp_host")
    n = steps.value
    out = {"result": res.value, "vars": trace[:min(n, nv + 1)].tolist(), "steps": n}
    if record:
        done = []
        for s in range(min(n, nv + 1)):
            if rso[s + 1] < 0:
                break
            done.append([rl[rco[c]:rco[c + 1]].tolist() for c in range(rso[s], rso[s + 1])])
        out["clauses"] = done
    return out


def last_stats():
    """Work of the last eliminate() call in this thread (satmi_dp_last_stats):
    steps, subset tests, new resolvents, kernel launches, key words, the
    device time of the elimination steps (ms), and how often a step was run
    again after each buffer ran out (satmi_dp_last_resumes)."""
    v = [ctypes.c_int64(0) for _ in range(4)]
    w = ctypes.c_int(0)
    ms = ctypes.c_double(0.0)
    _capi.check(_capi.load().satmi_dp_last_stats(*(ctypes.byref(x) for x in v), ctypes.byref(w), ctypes.byref(ms)),
                "satmi_dp_last_stats")
    rs = (ctypes.c_int32 * 4)()
    _capi.check(_capi.load().satmi_dp_last_resumes(rs), "satmi_dp_last_resumes")
    return {"steps": v[0].value, "subset_tests": v[1].value, "new_clauses": v[2].value,
            "launches": v[3].value, "words": w.value, "device_ms": ms.value,
            "resumes": dict(zip(("pairs", "clauses", "arena", "scratch"), rs))}


def davis_putnam_solve(formula, time_limit=0.0):
    """davis_putnam_solver(formula) -> bool (REF.py:98-130)."""
    r = eliminate(formula, time_limit=time_limit)
    if r["result"] < 0:
        raise DavisPutnamLimit(f"Davis-Putnam stopped by its limit after {r['steps']} steps")
    return bool(r["result"])


# ---------------------------------------------------------------- the batch
_STEP_CAP = 64   # the device keeps rows for 64 steps: at most 31 variables, each popped at most twice


def order_free_pop(ids):
    """What `set(ids).pop()` returns for distinct small positive ints whatever
    their insertion order, or None when the order decides.  A fresh set of n
    such ints has 8 slots for n <= 4, 32 for n <= 18, 128 for n <= 76, ...
    (CPython's growth rule); when the home slots `id & (slots - 1)` are
    pairwise distinct every id sits at its home and pop() takes the lowest
    home -- {3, 4, 5, 9} pops 9, {15, 16} pops 16.  With colliding homes
    ({3, 11}) the insertion order decides: None.  The batched kernel orders
    its variables by this rule (csrc/dp_batch.hip)."""
    ids = list(ids)
    n = len(ids)
    if n == 0 or len(set(ids)) != n or min(ids) < 1:
        return None
    mask = 7
    while True:
        thr = (mask * 3 + 4) // 5            # the fill that triggers the next resize
        if n < thr:
            break
        minused = thr * 2 if thr > 50000 else thr * 4
        size = 8
        while size <= minused:
            size <<= 1
        mask = size - 1
    homes = {}
    for v in ids:
        if homes.setdefault(v & mask, v) != v:
            return None
    return homes[min(homes)]


def debug_batch(grid=0, clause_cap=0):
    """Test knob of eliminate_batch (satmi_dp_debug_batch; 0 = default): at most
    `grid` workgroups, at most `clause_cap` clauses per clause list."""
    _capi.check(_capi.load().satmi_dp_debug_batch(int(grid), int(clause_cap)), "satmi_dp_debug_batch")


def _lit_order(clause):
    """A clause in the batch record's literal order: ascending variable id, +v before -v."""
    return sorted(set(clause), key=lambda l: (abs(l), l < 0))


def eliminate_batch(formulas, step_limit=0, clause_limit=0, time_limit=0.0, record=False, rec_cap=1 << 20):
    """eliminate() for many small formulas in one launch (csrc/dp_batch.hip: one
    workgroup per formula, every step in LDS).  `formulas` is a list of formulas
    or a cnf.CnfBatch; returns a list of eliminate()'s dicts, each with
      "path": "batch", or "single" for a formula the batched kernel does not
          take (more than 31 variables, a clause list beyond its capacity, or
          live variable ids whose set-table homes collide: order_free_pop),
          which is run through eliminate() -- `time_limit` applies to those
          calls only: the batched kernel's work is bounded by its capacity;
      "step_clauses": the clause count after every completed step (a step that
          ended the elimination completed none).  For a "single" result it is
          taken from the record when record=True and omitted otherwise;
      "clauses" (record=True): the clause list after every completed step, in
          list order, every clause's literals ascending by variable id (+v
          before -v) -- not eliminate()'s set iteration order; "single"
          results are normalised to the same order."""
    L = _capi.load()
    inp = _batch.packed(formulas)
    if inp is None:
        return []
    cb, arrays = inp
    B = cb.num_instances
    res = np.zeros(B, dtype=np.int32)
    steps = np.zeros(B, dtype=np.int32)
    trace = np.zeros((B, _STEP_CAP), dtype=np.int32)
    sc = np.zeros((B, _STEP_CAP), dtype=np.int64)
    i64 = ctypes.c_int64
    args = (B, *map(_p, arrays), int(step_limit), int(clause_limit), _p(res), _p(steps), _p(trace),
            _p(sc, i64), _STEP_CAP)
    if not record:
        _capi.check(L.satmi_dp_batch_host(*args, None, 0, None, 0, None), "satmi_dp_batch_host")
    else:
        while True:
            rl = np.zeros(rec_cap, dtype=np.int32)
            rco = np.zeros(rec_cap + 1, dtype=np.int64)
            rso = np.zeros((B, _STEP_CAP + 1), dtype=np.int64)
            _capi.check(L.satmi_dp_batch_host(*args, _p(rl), rec_cap, _p(rco, i64), rec_cap + 1, _p(rso, i64)),
                        "satmi_dp_batch_host")
            # the record is truncated silently at its capacities: complete iff it
            # holds every counted clause and the literals did not run out
            if int(rso[-1, -1]) == int(sc.sum()) and int(rco[int(rso[-1, -1])]) < rec_cap:
                break
            rec_cap *= 4
    out = []
    for b in range(B):
        if res[b] == _capi.DP_BATCH_UNFIT:
            r = eliminate(cb.instance(b), step_limit=step_limit, clause_limit=clause_limit, time_limit=time_limit,
                          record=record)
            if record:
                r["clauses"] = [[_lit_order(c) for c in cl] for cl in r["clauses"]]
                r["step_clauses"] = [len(cl) for cl in r["clauses"]]
            r["path"] = "single"
        else:
            n = int(steps[b])
            # a completed list is empty only when it ends the elimination with
            # True, so a last step with count 0 under another verdict is the
            # step that ended it
            done = n if n == 0 or res[b] == 1 or sc[b, n - 1] > 0 else n - 1
            r = {"result": int(res[b]), "vars": trace[b, :n].tolist(), "steps": n,
                 "step_clauses": sc[b, :done].tolist()}
            if record:
                r["clauses"] = [[rl[rco[c]:rco[c + 1]].tolist() for c in range(rso[b, k], rso[b, k + 1])]
                                for k in range(done)]
            r["path"] = "batch"
        out.append(r)
    return out


def davis_putnam_solve_batch(formulas, time_limit=0.0):
    """davis_putnam_solve for a list of formulas (or a cnf.CnfBatch) -> List[bool]."""
    out = []
    for r in eliminate_batch(formulas, time_limit=time_limit):
        if r["result"] < 0:
            raise DavisPutnamLimit(f"Davis-Putnam stopped by its limit after {r['steps']} steps")
        out.append(bool(r["result"]))
    return out
