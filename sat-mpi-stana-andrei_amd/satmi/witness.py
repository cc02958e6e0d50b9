"""Batched witness models on the GPU (libsatmi.so, csrc/witness.hip): rebuild an
assignment from the record of a Davis-Putnam elimination or of a resolution
saturation that answered True, and evaluate it against the formula, one
wavefront per formula.

Formula b (m clauses) comes with a record (P clauses) and an ordered list of
stages (x, lo, hi): a variable and a clause range lo <= hi <= m + P, where index
c < m is formula clause c and index m + j record clause j.  The assignment is
total and starts all False.  A stage reads the clauses of its range under the
assignment as it stands: a clause with +x and -x is passed, and with
`highest_only` so is one whose largest |literal| is not x; needP holds if some
clause holds +x and every other literal of it is false, needN likewise with -x;
with both the stage is stuck; in every case x becomes needP.  After the last
stage every clause of the formula is evaluated.  Per formula the call returns
_capi.WITNESS_WORDS: status (WITNESS_MODEL iff no clause is falsified, whatever
the stages were), the stuck stages, the first of them (-1: none), flags
(WITNESS_BAD_LITERAL, WITNESS_BAD_STAGE, WITNESS_ROW_TRUNCATED), the falsified
clauses and the first of them (-1: none) -- and the assignment as a row that
check_models reads: one signed literal per variable of the formula, ascending.

stages_of_elimination and stages_of_resolution build the stages from the dicts
of eliminate / eliminate_batch and resolve / resolve_batch made with
record=True; record_of gives the record's clauses in the order the stages count
them.
"""
import numpy as np

from . import _capi
from ._batch import _p
from .cnf import CnfBatch, pack


def debug_grid(workgroups=0, waves_per_wg=0):
    """Test knob (0 = default): at most `workgroups` workgroups of `waves_per_wg` (1, 2, 4) wavefronts."""
    _capi.check(_capi.load().satmi_witness_debug_grid(int(workgroups), int(waves_per_wg)),
                "satmi_witness_debug_grid")


def _csr(batch):
    return tuple(np.ascontiguousarray(a, dtype=np.int32)
                 for a in (batch.inst_clause_begin, batch.clause_lit_begin, batch.lits))


def _stage_arrays(stages, B):
    """`stages[b]`, a list of (x, lo, hi) -> (inst_stage_begin [B + 1], var, lo, hi) int32."""
    if len(stages) != B:
        raise ValueError("stages must have one list per formula")
    isb = np.zeros(B + 1, dtype=np.int64)
    np.cumsum(np.fromiter(map(len, stages), dtype=np.int64, count=B), out=isb[1:])
    flat = np.array([t for s in stages for t in s], dtype=np.int64).reshape(-1, 3)
    if flat.size and (flat.max() > 2 ** 31 - 1 or flat.min() < -(2 ** 31)):
        raise ValueError("stages must lie within int32")
    cols = [np.ascontiguousarray(flat[:, k], dtype=np.int32) if flat.size else np.zeros(1, np.int32) for k in range(3)]
    return (isb.astype(np.int32), *cols)


def witness_models_packed(batch, record_batch, stages, highest_only=False, stride=None):
    """satmi_witness_models_host on two CnfBatches, the formulas and their records (formula b's
    record is "formula" b of `record_batch`), and `stages[b]`, a list of (x, lo, hi).  Returns
    (int32 [B, 6] words, int32 [B] row lengths, int32 [B, stride] rows); stride=None: as many
    literals as a formula has at the most, so no row is truncated."""
    B = batch.num_instances
    if record_batch.num_instances != B:
        raise ValueError("records must have one list of clauses per formula")
    st = _stage_arrays(stages, B)
    if stride is None:
        stride = max(1, min(batch.maxima()[0], batch.maxima()[2])) if B else 1
    out = np.zeros((B, _capi.WITNESS_NWORDS), dtype=np.int32)
    lens = np.zeros(B, dtype=np.int32)
    rows = np.zeros((B, int(stride)), dtype=np.int32)
    if B:
        f, p = _csr(batch), _csr(record_batch)
        rc = _capi.load().satmi_witness_models_host(B, *map(_p, f), *map(_p, p), *map(_p, st),
                                                    int(bool(highest_only)), _p(out), _p(lens), _p(rows),
                                                    int(stride))
        _capi.check(rc, "satmi_witness_models_host")
    return out, lens, rows


def witness_models(formulas_or_batch, records, stages, highest_only=False):
    """Rebuild and check an assignment of formula b from `records[b]`, a list of clauses, and
    `stages[b]`, a list of (x, lo, hi).  Returns one dict per formula: status, stuck,
    first_stuck, flags, falsified, first_falsified, ok (status == WITNESS_MODEL and flags == 0)
    and "model": the assignment as signed literals, ascending by variable."""
    batch = formulas_or_batch if isinstance(formulas_or_batch, CnfBatch) else pack(formulas_or_batch)
    record_batch = records if isinstance(records, CnfBatch) else pack(records)
    out, lens, rows = witness_models_packed(batch, record_batch, stages, highest_only)
    return [dict(zip(_capi.WITNESS_WORDS, map(int, w)), ok=bool(w[0] == _capi.WITNESS_MODEL and w[3] == 0),
                 model=rows[b, :min(int(lens[b]), rows.shape[1])].tolist()) for b, w in enumerate(out)]


def witness_models_device(num_instances, icb, clb, lits, record_icb, record_clb, record_lits, inst_stage_begin,
                          stage_var, stage_lo, stage_hi, highest_only, max_vars, max_clause_len, out, row_len,
                          row_lits, stride, stream=None):
    """satmi_witness_models_device on device pointers (ints, e.g. a tensor's data_ptr());
    asynchronous on `stream`.  row_len / row_lits / stride are what check.check_device reads
    with cap = 1."""
    rc = _capi.load().satmi_witness_models_device(int(num_instances), icb, clb, lits, record_icb, record_clb,
                                                  record_lits, inst_stage_begin, stage_var, stage_lo, stage_hi,
                                                  int(bool(highest_only)), int(max_vars), int(max_clause_len), out,
                                                  row_len, row_lits, int(stride), stream)
    _capi.check(rc, "satmi_witness_models_device")


# ---- the solvers' records as stages
def record_of(r):
    """The record's clauses in a resolve / resolve_batch / eliminate / eliminate_batch dict
    made with record=True, in order: record clause j of the stages below."""
    if "clauses" not in r:
        raise ValueError("record_of: the result carries no record (run the solver with record=True)")
    return [list(c) for group in r["clauses"] for c in group]


def _true_record(r, what):
    if "clauses" not in r:
        raise ValueError(f"{what}: the result carries no record (run the solver with record=True)")
    if r["result"] != 1:
        raise ValueError(f"{what}: the result is {r['result']}, not 1 (True): there is nothing to witness")


def stages_of_elimination(formula, r):
    """The stages of an eliminate / eliminate_batch dict made with record=True whose result is
    1: step k popped vars[k] from the clause list S_k -- S_0 is the formula, [0, m), S_k the
    record's list after step k - 1 -- and the steps are walked backwards, so that every popped
    variable gets the value the clauses it was popped from need under the later ones."""
    _true_record(r, "stages_of_elimination")
    lo, spans = len(formula), [(0, len(formula))]
    for group in r["clauses"]:
        spans.append((lo, lo + len(group)))
        lo += len(group)
    return [(int(r["vars"][k]), *spans[k]) for k in range(len(r["clauses"]) - 1, -1, -1)]


def stages_of_resolution(formula, r):
    """The stages of a resolve / resolve_batch dict made with record=True whose result is 1:
    one stage (v, 0, m + P) per distinct variable of formula and record, ascending, for
    highest_only=True -- every variable gets the value that the saturated set's clauses with
    no larger variable need under the smaller ones."""
    _true_record(r, "stages_of_resolution")
    record = record_of(r)
    top = len(formula) + len(record)
    return [(v, 0, top) for v in sorted({abs(l) for c in list(formula) + record for l in c})]
