"""Batched model check on the GPU (libsatmi.so, csrc/check.hip): evaluate
assignment rows against their clause sets, one wavefront per formula.

A literal l is true if l is in the row, false if -l is in the row and l is not,
else unassigned; a clause is satisfied if some literal is true, falsified if
every literal is false (the empty clause always is), else undetermined.  Per row
the check returns _capi.CHECK_WORDS: clauses falsified, clauses undetermined,
the index of the first falsified clause (-1: none) and flags
(CHECK_CONTRADICTORY: some v with +v and -v in the row; CHECK_BAD_LITERAL: a
literal 0 or beyond the table, ignored).  A row is a model iff words 0, 1 and 3
are all 0.  UNSAT answers are certified by satmi/refute.py (check_refutations).
"""
import numpy as np

from . import _capi
from ._batch import _p
from .cnf import CnfBatch, pack


def debug_grid(workgroups=0, waves_per_wg=0):
    """Test knob (0 = default): at most `workgroups` workgroups of `waves_per_wg` (1, 2, 4) wavefronts."""
    _capi.check(_capi.load().satmi_check_debug_grid(int(workgroups), int(waves_per_wg)), "satmi_check_debug_grid")


def check_packed(batch, rows, lens, lits):
    """satmi_check_models_host on a CnfBatch: `lens` [B, cap] and `lits` [B, cap, stride]
    are the row arrays (DpllResult.sol_len / sol_lits as they are), `rows` [B] the rows to
    check per formula (None = cap; the others come back as zeros).  Returns int32 [B, cap, 4]."""
    lens = np.ascontiguousarray(lens, dtype=np.int32)
    lits = np.ascontiguousarray(lits, dtype=np.int32)
    B = batch.num_instances
    if lens.ndim == 1:   # one row per formula (satmi_cdcl_batch_host's assign_len / assign)
        lens, lits = lens.reshape(B, 1), lits.reshape(B, 1, -1)
    if lens.ndim != 2 or lits.ndim != 3 or lens.shape != lits.shape[:2] or lens.shape[0] != B:
        raise ValueError("lens must be [B, cap] and lits [B, cap, stride]")
    cap, stride = lens.shape[1], lits.shape[2]
    if rows is not None:
        rows = np.ascontiguousarray(rows, dtype=np.int32)
        if rows.shape != (B,):
            raise ValueError("rows must have one entry per formula")
    out = np.zeros((B, cap, _capi.CHECK_NWORDS), dtype=np.int32)
    if B == 0:
        return out
    icb, clb, fl = (np.ascontiguousarray(a, dtype=np.int32)
                    for a in (batch.inst_clause_begin, batch.clause_lit_begin, batch.lits))
    rc = _capi.load().satmi_check_models_host(B, _p(icb), _p(clb), _p(fl), None if rows is None else _p(rows),
                                              _p(lens), _p(lits), cap, stride, _p(out))
    _capi.check(rc, "satmi_check_models_host")
    return out


def _row(model):
    """A model as signed literals: a dict {variable: bool} or an iterable of literals."""
    if isinstance(model, dict):
        return [int(v) if val else -int(v) for v, val in model.items()]
    return [int(l) for l in model]


def check_models(formulas_or_batch, models):
    """Check `models[b]` -- a list of models of formula b, each a list of signed
    literals or a dict {variable: bool} -- against formula b.  Returns, per formula,
    one dict per model: falsified, undetermined, first_falsified, flags, ok."""
    batch = formulas_or_batch if isinstance(formulas_or_batch, CnfBatch) else pack(formulas_or_batch)
    B = batch.num_instances
    rows_of = [[_row(m) for m in ms] for ms in models]
    if len(rows_of) != B:
        raise ValueError("models must have one list per formula")
    cap = max([len(r) for r in rows_of] + [1])
    stride = max([len(x) for r in rows_of for x in r] + [1])
    rows = np.fromiter((len(r) for r in rows_of), dtype=np.int32, count=B)
    lens = np.zeros((B, cap), dtype=np.int32)
    lits = np.zeros((B, cap, stride), dtype=np.int32)
    for b, r in enumerate(rows_of):
        for k, x in enumerate(r):
            lens[b, k] = len(x)
            lits[b, k, :len(x)] = x
    out = check_packed(batch, rows, lens, lits)
    return [[dict(zip(_capi.CHECK_WORDS, map(int, w)), ok=bool(w[0] == 0 and w[1] == 0 and w[3] == 0))
             for w in out[b, :rows[b]]] for b in range(B)]


def check_device(num_instances, icb, clb, lits, max_vars, max_clause_len, rows, lens, row_lits, cap, stride, out,
                 stream=None):
    """satmi_check_models_device on device pointers (ints, e.g. a tensor's data_ptr();
    `rows` may be None); asynchronous on `stream`."""
    rc = _capi.load().satmi_check_models_device(int(num_instances), icb, clb, lits, int(max_vars),
                                                int(max_clause_len), rows, lens, row_lits, int(cap), int(stride),
                                                out, stream)
    _capi.check(rc, "satmi_check_models_device")
