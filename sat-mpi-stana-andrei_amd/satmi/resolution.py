"""Resolution saturation on the GPU (libsatmi.so, csrc/resolution.hip).

`resolve(formula, ...)` runs REF.py:63-95's saturation and returns the verdict
plus, optionally, the set of clauses each pass added; `resolution_solve` is the
reference's boolean entry point.
"""
import ctypes

import numpy as np

from . import _batch, _capi
from ._batch import _csr, _p


class ResolutionLimit(Exception):
    """A pass / clause / time limit stopped the saturation before a verdict."""


def resolve(formula, max_passes=0, clause_limit=0, time_limit=0.0, record=False, rec_cap=1 << 22):
    """Returns {"result": 1 (True) | 0 (False) | -1 (limit), "passes": int,
    "pass_new": [...], "clauses": [[sorted clause, ...] per pass] (record=True)}."""
    L = _capi.load()
    _capi.require_gpu()
    off, lits = _csr(formula)
    res = ctypes.c_int32(0)
    passes = ctypes.c_int32(0)
    pcap = int(max_passes) if 0 < max_passes < (1 << 16) else 1 << 16
    pass_new = np.zeros(pcap, dtype=np.int64)
    if record:
        rl = np.zeros(rec_cap, dtype=np.int32)
        rco = np.zeros(rec_cap + 1, dtype=np.int64)
        rpo = np.zeros(pcap + 1, dtype=np.int64)
        rc = L.satmi_resolution_host(len(formula), _p(off), _p(lits), int(max_passes), int(clause_limit),
                                     float(time_limit), ctypes.byref(res), ctypes.byref(passes),
                                     _p(pass_new, ctypes.c_int64), pcap, _p(rl), rec_cap,
                                     _p(rco, ctypes.c_int64), rec_cap + 1, _p(rpo, ctypes.c_int64), pcap + 1)
    else:
        rc = L.satmi_resolution_host(len(formula), _p(off), _p(lits), int(max_passes), int(clause_limit),
                                     float(time_limit), ctypes.byref(res), ctypes.byref(passes),
                                     _p(pass_new, ctypes.c_int64), pcap, None, 0, None, 0, None, 0)
    _capi.check(rc, "satmi_resolution_host")
    n = passes.value
    out = {"result": res.value, "passes": n, "pass_new": pass_new[:min(n, pcap)].tolist()}
    if record:
        out["clauses"] = [[rl[rco[c]:rco[c + 1]].tolist() for c in range(rpo[p], rpo[p + 1])]
                          for p in range(min(n, pcap))]
    return out


# Per-pass counts a batched call keeps per formula at first (a saturation of a
# small set rarely takes more than a dozen passes); a formula with more passes
# is run again with room for every pass its capacity allows.
_PASS_CAP = 32
_PASS_CAP_MAX = 4096   # the largest key capacity: every completed pass adds a key


def debug_batch(grid=0, key_cap=0):
    """Test knob of resolve_batch (satmi_resolution_debug_batch; 0 = default): at most
    `grid` workgroups, at most `key_cap` keys per formula."""
    _capi.check(_capi.load().satmi_resolution_debug_batch(int(grid), int(key_cap)), "satmi_resolution_debug_batch")


def _batch_call(L, cb, arrays, max_passes, clause_limit, record, pcap, rec_cap):
    """One satmi_resolution_batch_host call -> (result[B], passes[B], pass_new[B, pcap], clauses or None),
    clauses[b][p] = the sorted clauses formula b's pass p added."""
    B = cb.num_instances
    res = np.zeros(B, dtype=np.int32)
    passes = np.zeros(B, dtype=np.int32)
    pass_new = np.zeros((B, pcap), dtype=np.int64)
    args = (B, *map(_p, arrays), int(max_passes), int(clause_limit),
            _p(res), _p(passes), _p(pass_new, ctypes.c_int64), pcap)

    if not record:
        _capi.check(L.satmi_resolution_batch_host(*args, None, 0, None, 0, None), "satmi_resolution_batch_host")
        return res, passes, pass_new, None
    while True:
        rl = np.zeros(rec_cap, dtype=np.int32)
        rco = np.zeros(rec_cap + 1, dtype=np.int64)
        rpo = np.zeros((B, pcap + 1), dtype=np.int64)
        _capi.check(L.satmi_resolution_batch_host(*args, _p(rl), rec_cap, _p(rco, ctypes.c_int64), rec_cap + 1,
                                                  _p(rpo, ctypes.c_int64)), "satmi_resolution_batch_host")
        # the record is truncated silently at its capacities: complete iff it holds every counted clause
        if int(rpo[-1, -1]) == int(pass_new.sum()):
            break
        rec_cap *= 4
    clauses = [[[rl[rco[c]:rco[c + 1]].tolist() for c in range(rpo[b, p], rpo[b, p + 1])]
                for p in range(min(int(passes[b]), pcap))] for b in range(B)]
    return res, passes, pass_new, clauses


def resolve_batch(formulas, max_passes=0, clause_limit=0, time_limit=0.0, record=False, rec_cap=1 << 20):
    """resolve() for many small formulas in one launch (csrc/resolution_batch.hip:
    one workgroup per formula, saturated in LDS).  `formulas` is a list of
    formulas or a cnf.CnfBatch; returns the list of resolve()'s dicts, each
    with "path": "batch", or "single" for a formula the batched kernel does not
    take (more than 31 variables, or more clauses than its capacity), which is
    run through resolve() -- `time_limit` applies to those calls only: the
    batched kernel's work is bounded by its capacity."""
    L = _capi.load()
    inp = _batch.packed(formulas)
    if inp is None:
        return []
    cb = inp[0]
    B = cb.num_instances
    pcap = int(max_passes) if 0 < max_passes < _PASS_CAP else _PASS_CAP

    out = [None] * B

    def fill(rows, call):   # out[b] for every (b, k) of rows: formula b from row k of a call's outputs
        res, passes, pass_new, clauses = call
        for b, k in rows:
            if res[k] == _capi.RES_BATCH_UNFIT:
                r = resolve(cb.instance(b), max_passes=max_passes, clause_limit=clause_limit, time_limit=time_limit,
                            record=record)
                r["path"] = "single"
            else:
                n = int(passes[k])
                r = {"result": int(res[k]), "passes": n, "pass_new": pass_new[k, :n].tolist()}   # (at most the row)
                if record:
                    r["clauses"] = clauses[k]
                r["path"] = "batch"
            out[b] = r

    fill(zip(range(B), range(B)), _batch_call(L, *inp, max_passes, clause_limit, record, pcap, rec_cap))
    # formulas with more passes than the first call kept counts for: once more, with room for all
    # (the same capacity rule, so none of them is expected to come back UNFIT)
    more = [b for b in range(B) if out[b]["path"] == "batch" and out[b]["passes"] > pcap]
    if more:
        sub = _batch.packed([cb.instance(b) for b in more])
        fill(zip(more, range(len(more))), _batch_call(L, *sub, max_passes, clause_limit, record, _PASS_CAP_MAX, rec_cap))
    return out


def resolution_solve_batch(formulas, time_limit=0.0):
    """resolution_solve for a list of formulas (or a cnf.CnfBatch) -> List[bool]."""
    out = []
    for r in resolve_batch(formulas, time_limit=time_limit):
        if r["result"] < 0:
            raise ResolutionLimit(f"resolution stopped by its limit after {r['passes']} passes")
        out.append(bool(r["result"]))
    return out


def last_stats():
    """Work and device time of the last resolve() call: pairs, candidate
    resolvents, pair-kernel ms, claim (hash dedup) kernel ms, and the pass
    kernels' live shader clock (Hz; 0 on the general path); "regrowths": what
    the call regrew or ran again (satmi_resolution_last_regrowths) -- passes of
    the packed path run again for the stage / the key buffer / the table, and
    the general path's chunks, candidate-buffer re-runs, mid-pass table
    rebuilds and clause-buffer growths."""
    L = _capi.load()
    pairs, cand = ctypes.c_int64(0), ctypes.c_int64(0)
    pms, cms = ctypes.c_double(0.0), ctypes.c_double(0.0)
    _capi.check(L.satmi_resolution_last_stats(ctypes.byref(pairs), ctypes.byref(cand), ctypes.byref(pms),
                                              ctypes.byref(cms)), "satmi_resolution_last_stats")
    hz = ctypes.c_double(0.0)
    _capi.check(L.satmi_resolution_last_clock(ctypes.byref(hz)), "satmi_resolution_last_clock")
    rg = (ctypes.c_int64 * len(_capi.RES_REGROWTHS))()
    _capi.check(L.satmi_resolution_last_regrowths(rg, len(rg)), "satmi_resolution_last_regrowths")
    return {"pairs": pairs.value, "candidates": cand.value, "pair_ms": pms.value, "claim_ms": cms.value,
            "shader_clock_hz": hz.value, "regrowths": dict(zip(_capi.RES_REGROWTHS, rg))}


def resolution_solve(formula, time_limit=0.0):
    """resolution_solver(formula) -> bool (REF.py:63-95)."""
    r = resolve(formula, time_limit=time_limit)
    if r["result"] < 0:
        raise ResolutionLimit(f"resolution stopped by its limit after {r['passes']} passes")
    return bool(r["result"])
