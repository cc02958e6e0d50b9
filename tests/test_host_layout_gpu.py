"""GPU: satmi_dpll_batch_host (SOUND and REF) and satmi_cdcl_batch_host on three
tiny formulas laid out as a window into larger arrays -- icb[0] > 0, clb[0] > 0,
literals that belong to no clause before and after the window, clauses that
belong to no formula before it, one formula empty -- against the same formulas
packed from offset 0: every output identical.  The staging copies the arrays
whole and the kernels index them absolutely; the shape the entry points measure
covers the window's formulas.  (The ordinary layout through the same staging:
test_dpll_host_staging_gpu.py and the CDCL tests.)"""
import ctypes

import numpy as np
import pytest

from satmi import _capi, cnf

pytestmark = pytest.mark.gpu

FS = [[[1, 2, 3], [-1, 2], [-2, 3], [-3, -1], [1, -2, -3]], [], [[4, 5], [-4, 5], [4, -5], [-4, -5, 6], [-6, -4]]]
PRE = [[2, -1, 3], [-2]]   # clauses before the window: lengths and variables within the formulas'
PAD = 5                    # literals before clb[0] and behind the last clause: zeros, never read
STRIDE = 6


def _p(a, t=ctypes.c_int32):
    return a.ctypes.data_as(ctypes.POINTER(t))


def _layouts():
    b = cnf.pack(FS)
    packed = tuple(np.ascontiguousarray(a, dtype=np.int32) for a in (b.inst_clause_begin, b.clause_lit_begin, b.lits))
    pre_lits = [l for c in PRE for l in c]
    pre_off = np.cumsum([0] + [len(c) for c in PRE])
    icb = packed[0] + len(PRE)
    clb = np.concatenate([PAD + pre_off, PAD + len(pre_lits) + packed[1][1:]]).astype(np.int32)
    lits = np.concatenate([np.zeros(PAD), pre_lits, packed[2][:packed[1][-1]], np.zeros(PAD)]).astype(np.int32)
    assert icb[0] > 0 and clb[0] > 0 and clb[icb[0]] > clb[0]
    return {"packed": packed, "window": (icb.astype(np.int32), clb, lits)}, b.inst_nvars.astype(np.int32)


def _dpll(arrays, nvars, mode):
    B, cap = len(FS), 16
    out = {"status": np.full(B, -9, np.int32), "counters": np.full((B, _capi.NCOUNTERS), -9, np.int64),
           "sol_len": np.full((B, cap), -9, np.int32), "sol_lits": np.full((B, cap, STRIDE), -9, np.int32),
           "root_len": np.full(B, -9, np.int32), "root_lits": np.full((B, STRIDE), -9, np.int32)}
    rc = _capi.load().satmi_dpll_batch_host(
        B, _p(arrays[0]), _p(arrays[1]), _p(arrays[2]), _p(nvars), None, None, mode,
        1 if mode == _capi.MODE_SOUND else 0, 0, 0.0, cap, STRIDE, _p(out["status"]),
        _p(out["counters"], ctypes.c_int64), _p(out["sol_len"]), _p(out["sol_lits"]), _p(out["root_len"]),
        _p(out["root_lits"]))
    _capi.check(rc, "satmi_dpll_batch_host")
    # what the call defines: the counters but the clock's ticks, the stored models, the root literals
    k = np.minimum(out["counters"][:, _capi.COUNTER_NAMES.index("solutions")], cap)
    return {"status": out["status"].tolist(), "counters": out["counters"][:, :_capi.COUNTER_NAMES.index("ticks")].tolist(),
            "models": [[out["sol_lits"][b, s, :out["sol_len"][b, s]].tolist() for s in range(k[b])] for b in range(B)],
            "roots": [out["root_lits"][b, :out["root_len"][b]].tolist() for b in range(B)]}


def _cdcl(arrays, nvars, mode):
    B = len(FS)
    out = {"status": np.full(B, -9, np.int32), "assign_len": np.full(B, -9, np.int32),
           "assign": np.full((B, STRIDE), -9, np.int32), "stats": np.full((B, 8), -9, np.int64),
           "var_inc": np.full(B, -9.0, np.float64)}
    rc = _capi.load().satmi_cdcl_batch_host(
        B, _p(arrays[0]), _p(arrays[1]), _p(arrays[2]), 0, 0, 0.0, _p(out["status"]), _p(out["assign_len"]),
        _p(out["assign"]), STRIDE, _p(out["stats"], ctypes.c_int64), _p(out["var_inc"], ctypes.c_double))
    _capi.check(rc, "satmi_cdcl_batch_host")
    return {"status": out["status"].tolist(), "stats": out["stats"].tolist(), "var_inc": out["var_inc"].tolist(),
            "assignment": [out["assign"][b, :out["assign_len"][b]].tolist() for b in range(B)]}


@pytest.mark.parametrize("solver,mode", [(_dpll, _capi.MODE_SOUND), (_dpll, _capi.MODE_REF), (_cdcl, None)],
                         ids=["dpll-sound", "dpll-ref", "cdcl"])
def test_window_equals_packed(solver, mode):
    _capi.require_gpu()
    layouts, nvars = _layouts()
    want, got = solver(layouts["packed"], nvars, mode), solver(layouts["window"], nvars, mode)
    print(want)
    assert -9 not in want["status"]
    assert got == want


def test_resolution_of_no_clause_reads_neither_array():
    """satmi_resolution_host with nclauses = 0 and both arrays NULL, as ever: the same
    answer as with arrays it has no reason to read."""
    _capi.require_gpu()
    L = _capi.load()
    seen, off, lits = [], np.array([3], np.int32), np.zeros(4, np.int32)
    for arrays in ((None, None), (_p(off), _p(lits))):
        result, passes = np.full(1, -9, np.int32), np.full(1, -9, np.int32)
        rc = L.satmi_resolution_host(0, arrays[0], arrays[1], 0, 0, 0.0, _p(result), _p(passes), None, 0, None, 0,
                                     None, 0, None, 0)
        _capi.check(rc, "satmi_resolution_host")
        seen.append((int(result[0]), int(passes[0])))
    assert seen[0] == seen[1] and seen[0][0] in (0, 1) and seen[0][1] == 0
