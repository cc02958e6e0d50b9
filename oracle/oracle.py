"""ctypes front-end for the CPU oracle (liboracle.so built from oracle/*.c).

TEST INFRASTRUCTURE ONLY: imported by tests/, by __graft_entry__.smoke() as the
checker and by bench.py's cpu_baseline leg.  The product package never imports it.
"""
import ctypes
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = os.path.join(_HERE, "liboracle.so")
_lib = None


class Counters(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int64) for n in
                ("nodes", "decisions", "unit_props", "pure_assigns", "conflicts", "solutions")]


def build():
    subprocess.run(["make", "-s", "-C", _HERE], check=True)


def _rebuild():
    subprocess.run(["make", "-s", "-B", "-C", _HERE], check=True)


# entry points a library kept from an older tree lacks
_NEWEST_ENTRIES = ("oracle_cdcl_paths", "oracle_dpll_paths")


def _open(path=_LIB, rebuild=_rebuild):
    """The library at `path`, rebuilt once if it predates an entry point this
    module binds (a library kept from an older tree): never a silent pass."""
    L = ctypes.CDLL(path)
    if all(hasattr(L, n) for n in _NEWEST_ENTRIES):
        return L
    import _ctypes
    _ctypes.dlclose(L._handle)   # or the next CDLL returns the old mapping
    del L
    rebuild()
    L = ctypes.CDLL(path)
    missing = [n for n in _NEWEST_ENTRIES if not hasattr(L, n)]
    if missing:
        _ctypes.dlclose(L._handle)
        raise RuntimeError(f"{path} has no {', '.join(missing)} after a rebuild: a stale oracle library")
    return L


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(_LIB):
            build()
        L = _open()
        P = ctypes.POINTER
        i32p, i64p = P(ctypes.c_int32), P(ctypes.c_int64)
        L.oracle_dpll.restype = ctypes.c_int
        L.oracle_dpll.argtypes = [ctypes.c_int, ctypes.c_int, i32p, i32p, ctypes.c_int, ctypes.c_int64,
                                  ctypes.c_int64, i32p, ctypes.c_int, i32p, ctypes.c_int64, i64p,
                                  ctypes.c_int64, i32p, P(ctypes.c_int), P(Counters)]
        L.oracle_dpll_paths.restype = ctypes.c_int
        L.oracle_dpll_paths.argtypes = L.oracle_dpll.argtypes + [i64p, ctypes.c_int]
        L.oracle_dp.restype = ctypes.c_int
        L.oracle_dp.argtypes = [ctypes.c_int, i32p, i32p, ctypes.c_int64, ctypes.c_int64, i32p, ctypes.c_int,
                                P(ctypes.c_int), i32p, ctypes.c_int64, i64p, ctypes.c_int64, i64p, ctypes.c_int]
        L.oracle_resolution.restype = ctypes.c_int
        L.oracle_resolution.argtypes = [ctypes.c_int, i32p, i32p, ctypes.c_int, ctypes.c_int64, i64p,
                                        ctypes.c_int, P(ctypes.c_int), i32p, ctypes.c_int64, i64p,
                                        ctypes.c_int64, i64p, ctypes.c_int]
        L.oracle_cdcl.restype = ctypes.c_int
        L.oracle_cdcl.argtypes = [ctypes.c_int, i32p, i32p, ctypes.c_int64, i32p, P(ctypes.c_int32), i64p,
                                  P(ctypes.c_double)]
        L.oracle_cdcl_paths.restype = ctypes.c_int
        L.oracle_cdcl_paths.argtypes = L.oracle_cdcl.argtypes + [i64p, ctypes.c_int]
        L.pyset_probe_from_list.restype = ctypes.c_int
        L.pyset_probe_from_list.argtypes = [i64p, ctypes.c_int, i64p]
        L.pyset_probe_resolvent.restype = ctypes.c_int
        L.pyset_probe_resolvent.argtypes = [i64p, ctypes.c_int, ctypes.c_int64, i64p, ctypes.c_int,
                                            ctypes.c_int64, i64p]
        L.pyset_probe_var_pop.restype = ctypes.c_int64
        L.pyset_probe_var_pop.argtypes = [i64p, P(ctypes.c_int), ctypes.c_int]
        _lib = L
    return _lib


def _csr(formula):
    off = np.zeros(len(formula) + 1, dtype=np.int32)
    for i, c in enumerate(formula):
        off[i + 1] = off[i] + len(c)
    lits = np.array([l for c in formula for l in c] or [0], dtype=np.int32)
    return off, lits


def _p(a, t=ctypes.c_int32):
    return a.ctypes.data_as(ctypes.POINTER(t))


# The path counters of oracle_dpll_paths, in the order of sat_oracle.c's DP_*
# (which says what each counts): which code paths of csrc/dpll.hip a formula
# drives.  Maxima of an index are -1 where the event never happened.
DPLL_PATHS = (
    "snapshot_len_max", "collected_snapshot_len_max", "stamp_drop_len_max", "mismatch_index_max",
    "emptied_index_max", "undone_after_stop_max", "cut_round_len_max", "snapshot_same_var_same_sign",
    "snapshot_same_var_opposite_sign", "snapshot_same_var_earlier_chunk", "skip_assigned_equal",
    "empty_clause_with_units", "empty_clause_no_units", "empty_clause_first_index_max",
    "occ_single_len_max", "flat_total_max", "flat_list_straddles_window", "unit_clause_index_max",
    "conflict_clauses_max", "pure_count_max", "pure_first_pos_max", "branch_var_max",
    "branch_tie_across_groups", "undo_len_max", "undo_non_effective", "init_overwrite",
    "init_var_beyond_formula", "init_mismatch", "decision_mismatch", "sols_past_cap", "clause_len_max",
    "model_mismatch")


def dpll(formula, mode="ref", max_solutions=0, node_limit=0, init=None, sol_cap=1 << 16, paths=False):
    """Run the DPLL restatement.  mode 'ref' = REF.py:133-214 exactly; 'sound' =
    decisions applied as unit clauses.  Returns dict with status, solutions
    (lists of signed literals in assignment-dict order), counters, root_assign;
    with paths=True also "paths": DPLL_PATHS of the same search."""
    off, lits = _csr(formula)
    nv = max([abs(l) for c in formula for l in c] + [abs(l) for l in (init or [])] + [1])
    init_a = np.array(list(init or []) or [0], dtype=np.int32)
    cap_l = max(1, sol_cap * (nv + 1))
    sol_lits = np.zeros(cap_l, dtype=np.int32)
    sol_off = np.zeros(sol_cap + 1, dtype=np.int64)
    root = np.zeros(nv + 1, dtype=np.int32)
    root_len = ctypes.c_int(0)
    ctr = Counters()
    args = (nv, len(formula), _p(off), _p(lits), 0 if mode == "ref" else 1,
            max_solutions, node_limit, _p(init_a), len(init or []),
            _p(sol_lits), cap_l, _p(sol_off, ctypes.c_int64), sol_cap,
            _p(root), ctypes.byref(root_len), ctypes.byref(ctr))
    if paths:
        pc = np.zeros(len(DPLL_PATHS), dtype=np.int64)
        st = lib().oracle_dpll_paths(*args, _p(pc, ctypes.c_int64), len(pc))
        if st == -3:
            raise RuntimeError("oracle_dpll_paths: DPLL_PATHS does not match the library's counters")
    else:
        st = lib().oracle_dpll(*args)
    nsol = min(ctr.solutions, sol_cap)
    sols = [sol_lits[sol_off[k]:sol_off[k + 1]].tolist() for k in range(nsol)]
    out = {"status": st, "solutions": sols,
           "counters": {n: getattr(ctr, n) for n, _ in Counters._fields_},
           "root_assign": root[:root_len.value].tolist()}
    if paths:
        out["paths"] = dict(zip(DPLL_PATHS, pc.tolist()))
    return out


def dp(formula, step_limit=0, clause_limit=0, record=False, rec_cap=1 << 20):
    off, lits = _csr(formula)
    nv = max([abs(l) for c in formula for l in c] + [1])
    trace = np.zeros(nv + 1, dtype=np.int32)
    nsteps = ctypes.c_int(0)
    if record:
        rl = np.zeros(rec_cap, dtype=np.int32)
        rco = np.zeros(rec_cap + 1, dtype=np.int64)
        rso = np.zeros(nv + 2, dtype=np.int64)
        r = lib().oracle_dp(len(formula), _p(off), _p(lits), step_limit, clause_limit, _p(trace), nv + 1,
                            ctypes.byref(nsteps), _p(rl), rec_cap, _p(rco, ctypes.c_int64), rec_cap,
                            _p(rso, ctypes.c_int64), nv + 1)
    else:
        r = lib().oracle_dp(len(formula), _p(off), _p(lits), step_limit, clause_limit, _p(trace), nv + 1,
                            ctypes.byref(nsteps), None, 0, None, 0, None, 0)
    out = {"result": r, "vars": trace[:min(nsteps.value, nv + 1)].tolist(), "steps": nsteps.value}
    if record:
        steps = []
        for s in range(min(nsteps.value, nv + 1)):
            if rso[s + 1] < rso[s]:
                break
            cl = [rl[rco[c]:rco[c + 1]].tolist() for c in range(rso[s], rso[s + 1])]
            steps.append(cl)
        out["clauses"] = steps
    return out


def resolution(formula, max_passes=0, clause_limit=0, record=False, rec_cap=1 << 20):
    off, lits = _csr(formula)
    pass_new = np.zeros(4096, dtype=np.int64)
    npass = ctypes.c_int(0)
    if record:
        rl = np.zeros(rec_cap, dtype=np.int32)
        rco = np.zeros(rec_cap + 1, dtype=np.int64)
        rpo = np.zeros(4097, dtype=np.int64)
        r = lib().oracle_resolution(len(formula), _p(off), _p(lits), max_passes, clause_limit,
                                    _p(pass_new, ctypes.c_int64), 4096, ctypes.byref(npass), _p(rl), rec_cap,
                                    _p(rco, ctypes.c_int64), rec_cap, _p(rpo, ctypes.c_int64), 4096)
    else:
        r = lib().oracle_resolution(len(formula), _p(off), _p(lits), max_passes, clause_limit,
                                    _p(pass_new, ctypes.c_int64), 4096, ctypes.byref(npass), None, 0, None, 0,
                                    None, 0)
    out = {"result": r, "passes": npass.value, "pass_new": pass_new[:npass.value].tolist()}
    if record:
        out["clauses"] = [[rl[rco[c]:rco[c + 1]].tolist() for c in range(rpo[p], rpo[p + 1])]
                          for p in range(npass.value)]
    return out


def pyset_from_list(keys):
    a = np.array(list(keys) or [0], dtype=np.int64)
    out = np.zeros(max(1, len(keys)), dtype=np.int64)
    n = lib().pyset_probe_from_list(_p(a, ctypes.c_int64), len(keys), _p(out, ctypes.c_int64))
    return out[:n].tolist()


def pyset_resolvent(a, x, b, y):
    A = np.array(list(a) or [0], dtype=np.int64)
    B = np.array(list(b) or [0], dtype=np.int64)
    out = np.zeros(len(a) + len(b) + 1, dtype=np.int64)
    n = lib().pyset_probe_resolvent(_p(A, ctypes.c_int64), len(a), x, _p(B, ctypes.c_int64), len(b), y,
                                    _p(out, ctypes.c_int64))
    return out[:n].tolist()


def pyset_var_pop(lists):
    off = np.zeros(len(lists) + 1, dtype=np.int32)
    for i, c in enumerate(lists):
        off[i + 1] = off[i] + len(c)
    lits = np.array([l for c in lists for l in c] or [0], dtype=np.int64)
    return lib().pyset_probe_var_pop(_p(lits, ctypes.c_int64), _p(off, ctypes.c_int), len(lists))


CDCL_STATS = ("iterations", "conflicts", "decisions", "learned", "clauses", "watch_keys", "level")


# The path counters of oracle_cdcl_paths, in the order of cdcl_oracle.c's
# CDCL_P_* (which says what each counts): which code paths of csrc/cdcl.hip a
# formula drives.  Maxima of a position are -1 where the event never happened.
CDCL_PATHS = (
    "false_key_index_max", "stream_len_max", "conflict_pos_max", "conflict_later_chunk",
    "conflict_later_window", "straddle_members", "repl_pos_max",
    "tail_skip_self", "dup_visit_passes",
    "conflict_len_max", "learned_len_max", "maxlevel_pos_max", "learned_repeat_le64", "learned_repeat_gt64",
    "learned_len_64", "learned_len_65", "resolve_steps", "resolve_alen_max", "learned_unit",
    "table_slots_max", "resize_le_4096", "resize_gt_4096", "resize_used_gt_50000", "add_dummy_reuse",
    "add_multi_run", "add_single_slot", "add_single_slot_big", "add_present",
    "decide_tie", "decide_low_word")


def cdcl(formula, max_iter=0, paths=False):
    """cdcl_solve (REF.py:382-384) restated: {"result": 1 True | 0 False | -1 the
    iteration cap | -2 the reference raises, "assignment": the assignment dict as
    signed literals in insertion order (the model for result 1), "var_inc",
    "stats": CDCL_STATS}; with paths=True also "paths": CDCL_PATHS of the same
    search."""
    off, lits = _csr(formula)
    nv = max([abs(l) for c in formula for l in c] + [1])
    model = np.zeros(nv + 1, dtype=np.int32)
    mlen = ctypes.c_int32(0)
    st = np.zeros(len(CDCL_STATS), dtype=np.int64)
    vi = ctypes.c_double(0.0)
    if paths:
        pc = np.zeros(len(CDCL_PATHS), dtype=np.int64)
        r = lib().oracle_cdcl_paths(len(formula), _p(off), _p(lits), int(max_iter), _p(model), ctypes.byref(mlen),
                                    _p(st, ctypes.c_int64), ctypes.byref(vi), _p(pc, ctypes.c_int64), len(pc))
        if r == -3:
            raise RuntimeError("oracle_cdcl_paths: CDCL_PATHS does not match the library's counters")
    else:
        r = lib().oracle_cdcl(len(formula), _p(off), _p(lits), int(max_iter), _p(model), ctypes.byref(mlen),
                              _p(st, ctypes.c_int64), ctypes.byref(vi))
    out = {"result": r, "assignment": model[:mlen.value].tolist(), "var_inc": vi.value,
           "stats": dict(zip(CDCL_STATS, st.tolist()))}
    if paths:
        out["paths"] = dict(zip(CDCL_PATHS, pc.tolist()))
    return out
