"""Batched refutation check on the GPU (libsatmi.so, csrc/refute.hip): verify
UNSAT answers by forward reverse unit propagation (RUP), one wavefront per formula.

A proof is an ordered list of lemma clauses.  Lemma i is verified if assigning
every literal of it false and running unit propagation to a fixpoint over the
formula and the lemmas before it reaches a conflict (a clause whose literals
are all false, or a variable needed with both signs).  An earlier lemma is a
premise whether or not it verified.  Checking ends with the first empty lemma.
Per formula the check returns _capi.REFUTE_WORDS: status (REFUTE_FAILED: a
checked lemma failed; REFUTE_PROVEN: none failed and an empty lemma was
reached; REFUTE_OPEN: none failed, no empty lemma), the number of failed lemmas,
the index of the first (-1: none) and flags (REFUTE_TAUTOLOGY: a checked lemma
holds +v and -v; REFUTE_BAD_LITERAL).

The records of resolve / resolve_batch and eliminate / eliminate_batch are such
proofs (proof_of_resolution, proof_of_elimination): every recorded clause is a
resolvent of two clauses before it, and the empty clause that ends a False
answer comes from two opposite unit clauses.

trim_refutations (csrc/trim.hip) is the backward form: from the first empty lemma
downwards it checks only the lemmas that lemma needs, and returns which formula
clauses (the UNSAT core) and which lemmas (the trimmed proof) the refutation uses.
"""
import ctypes

import numpy as np

from . import _capi
from ._batch import _p
from .cnf import CnfBatch, pack


def debug_grid(workgroups=0, waves_per_wg=0):
    """Test knob (0 = default): at most `workgroups` workgroups of `waves_per_wg` (1, 2, 4) wavefronts."""
    _capi.check(_capi.load().satmi_refute_debug_grid(int(workgroups), int(waves_per_wg)), "satmi_refute_debug_grid")


def _csr(batch):
    return tuple(np.ascontiguousarray(a, dtype=np.int32)
                 for a in (batch.inst_clause_begin, batch.clause_lit_begin, batch.lits))


def check_refutations_packed(batch, proof_batch, lemmas=False):
    """satmi_check_refutations_host on two CnfBatches, the formulas and their proofs
    (formula b's lemmas are "formula" b of `proof_batch`).  Returns int32 [B, 4], and with
    lemmas=True also int32 [P]: 1 verified, 0 failed, -1 not checked, per lemma."""
    B = batch.num_instances
    if proof_batch.num_instances != B:
        raise ValueError("proofs must have one list of lemmas per formula")
    out = np.zeros((B, _capi.REFUTE_NWORDS), dtype=np.int32)
    ok = np.full(int(proof_batch.inst_clause_begin[B]) if B else 0, -1, dtype=np.int32)
    if B:
        f, p = _csr(batch), _csr(proof_batch)
        rc = _capi.load().satmi_check_refutations_host(B, *map(_p, f), *map(_p, p), _p(out),
                                                       _p(ok) if lemmas and ok.size else None)
        _capi.check(rc, "satmi_check_refutations_host")
    return (out, ok) if lemmas else out


def check_refutations(formulas_or_batch, proofs, lemmas=False):
    """Check `proofs[b]`, a list of lemma clauses, against formula b.  Returns one dict per
    formula: status, failed, first_failed, flags, proven (status == REFUTE_PROVEN), and with
    lemmas=True "lemma_ok": 1 / 0 / -1 per lemma."""
    batch = formulas_or_batch if isinstance(formulas_or_batch, CnfBatch) else pack(formulas_or_batch)
    proof_batch = proofs if isinstance(proofs, CnfBatch) else pack(proofs)
    got = check_refutations_packed(batch, proof_batch, lemmas)
    out, ok = got if lemmas else (got, None)
    res = [dict(zip(_capi.REFUTE_WORDS, map(int, w)), proven=bool(w[0] == _capi.REFUTE_PROVEN)) for w in out]
    if lemmas:
        pib = proof_batch.inst_clause_begin
        for b, r in enumerate(res):
            r["lemma_ok"] = ok[pib[b]:pib[b + 1]].tolist()
    return res


def check_refutation(formula, proof):
    """check_refutations on one formula: whether `proof` refutes it."""
    return check_refutations([formula], [proof])[0]["proven"]


def check_refutations_device(num_instances, icb, clb, lits, proof_icb, proof_clb, proof_lits, max_vars,
                             max_clause_len, out, lemma_ok=None, stream=None):
    """satmi_check_refutations_device on device pointers (ints, e.g. a tensor's data_ptr();
    `lemma_ok` may be None); asynchronous on `stream`."""
    rc = _capi.load().satmi_check_refutations_device(int(num_instances), icb, clb, lits, proof_icb, proof_clb,
                                                     proof_lits, int(max_vars), int(max_clause_len), out, lemma_ok,
                                                     stream)
    _capi.check(rc, "satmi_check_refutations_device")


# ---- the backward form: UNSAT cores and trimmed proofs (csrc/trim.hip)
def trim_debug_grid(workgroups=0, waves_per_wg=0):
    """debug_grid for the trim's launches."""
    _capi.check(_capi.load().satmi_trim_debug_grid(int(workgroups), int(waves_per_wg)), "satmi_trim_debug_grid")


def trim_refutations_packed(batch, proof_batch):
    """satmi_trim_refutations_host on two CnfBatches, as check_refutations_packed.  Returns
    (int32 [B, 6] words, int32 [C] core marks: 1 / 0 per formula clause, int32 [P] lemma marks:
    1 needed and verified, 0 needed and failed, -1 not needed)."""
    B = batch.num_instances
    if proof_batch.num_instances != B:
        raise ValueError("proofs must have one list of lemmas per formula")
    out = np.zeros((B, _capi.TRIM_NWORDS), dtype=np.int32)
    core = np.zeros(int(batch.inst_clause_begin[B]) if B else 0, dtype=np.int32)
    lemma = np.full(int(proof_batch.inst_clause_begin[B]) if B else 0, -1, dtype=np.int32)
    if B:
        f, p = _csr(batch), _csr(proof_batch)
        rc = _capi.load().satmi_trim_refutations_host(B, *map(_p, f), *map(_p, p), _p(out),
                                                      _p(core) if core.size else None,
                                                      _p(lemma) if lemma.size else None)
        _capi.check(rc, "satmi_trim_refutations_host")
    return out, core, lemma


def trim_refutations(formulas_or_batch, proofs):
    """Trim `proofs[b]` against formula b by the backward check: only the lemmas that the
    first empty lemma needs are checked, and what they use is marked.  Returns one dict per
    formula: status, failed, first_failed, flags, proven (status == REFUTE_PROVEN: the core
    clauses with the kept lemmas are a proof check_refutations accepts), "core": ascending
    clause indices into the formula, "kept": ascending lemma indices (the ending empty lemma
    included), "proof": the kept lemma clauses, in order.  Which core is found depends on the
    clause form the launch takes (satmi.h), never on anything else."""
    batch = formulas_or_batch if isinstance(formulas_or_batch, CnfBatch) else pack(formulas_or_batch)
    proof_batch = proofs if isinstance(proofs, CnfBatch) else pack(proofs)
    out, core, lemma = trim_refutations_packed(batch, proof_batch)
    icb, pib = batch.inst_clause_begin, proof_batch.inst_clause_begin
    res = []
    for b, w in enumerate(out):
        r = dict(zip(_capi.REFUTE_WORDS, map(int, w[:4])), proven=bool(w[0] == _capi.REFUTE_PROVEN))
        r["core"] = np.flatnonzero(core[icb[b]:icb[b + 1]] == 1).tolist()
        r["kept"] = np.flatnonzero(lemma[pib[b]:pib[b + 1]] >= 0).tolist()
        lemmas = proof_batch.instance(b)
        r["proof"] = [list(lemmas[j]) for j in r["kept"]]
        res.append(r)
    return res


def trim_refutations_device(num_instances, icb, clb, lits, proof_icb, proof_clb, proof_lits, max_vars,
                            max_clause_len, out, core, lemma, stream=None):
    """satmi_trim_refutations_device on device pointers (ints, e.g. a tensor's data_ptr());
    asynchronous on `stream`.  `core` and `lemma` are both required and need no initialisation."""
    rc = _capi.load().satmi_trim_refutations_device(int(num_instances), icb, clb, lits, proof_icb, proof_clb,
                                                    proof_lits, int(max_vars), int(max_clause_len), out, core, lemma,
                                                    stream)
    _capi.check(rc, "satmi_trim_refutations_device")


def _proof_of(r, what):
    if "clauses" not in r:
        raise ValueError(f"{what}: the result carries no record (run the solver with record=True)")
    proof = [list(c) for group in r["clauses"] for c in group]
    if r["result"] == 0:
        proof.append([])
    return proof


def proof_of_resolution(r):
    """The proof in a resolve / resolve_batch dict made with record=True: the clauses
    every pass added, in order, and the empty clause exactly when the result is 0."""
    return _proof_of(r, "proof_of_resolution")


def proof_of_elimination(r):
    """The proof in an eliminate / eliminate_batch dict made with record=True: the
    clause list after every completed step, in order, and the empty clause exactly
    when the result is 0."""
    return _proof_of(r, "proof_of_elimination")


# ---- refutations of sound DPLL's UNSAT answers (csrc/dpll.hip's logging kernels, csrc/dpll_proof.hip)
def _logging_args(mode, inits, who):
    """A lemma cannot discharge an assumption and REF-mode decisions do not rewrite the
    formula: logging is SOUND mode without a caller assignment (satmi.h: SATMI_ERR_ARG)."""
    if mode != "sound" or inits is not None:
        raise _capi.SatmiError(f"{who} failed ({_capi.ERR_ARG}): {who}: logging needs SOUND mode and no caller "
                               "assignment")


def dpll_refutations_packed(batch, max_solutions=1, node_limit=0, time_limit=0.0, sol_cap=None, mode="sound",
                            inits=None, room=None):
    """satmi_dpll_refutations_host on a CnfBatch: sound DPLL by the logging general kernel.
    Returns (DpllResult, proof CnfBatch, int64 [B, 4] info: _capi.DPLL_PROOF_WORDS).  Formula
    b's lemmas are "formula" b of the proof batch: the refutation of an instance that ended
    exhausted with no solution, else no lemma.  `room` = (lemmas, literals) the first call's
    proof arrays hold; a proof that outgrows them is asked for again with 4x the room (the
    totals, if those are more)."""
    from .dpll import DpllResult
    _logging_args(mode, inits, "satmi_dpll_refutations_host")
    L = _capi.load()
    _capi.require_gpu()
    B = batch.num_instances
    if sol_cap is None:
        sol_cap = max(1, max_solutions) if max_solutions > 0 else 1024
    stride = max(1, int(batch.inst_nvars.max(initial=0)))
    status = np.zeros(B, dtype=np.int32)
    counters = np.zeros((B, _capi.NCOUNTERS), dtype=np.int64)
    sol_len = np.zeros((B, max(sol_cap, 1)), dtype=np.int32)
    sol_lits = np.zeros((B, max(sol_cap, 1), stride), dtype=np.int32)
    root_len = np.zeros(B, dtype=np.int32)
    root_lits = np.zeros((B, stride), dtype=np.int32)
    info = np.zeros((B, _capi.DPLL_PROOF_NWORDS), dtype=np.int64)
    totals = np.zeros(2, dtype=np.int64)
    pib = np.zeros(B + 1, dtype=np.int32)
    ccap, lcap = room if room is not None else (max(1024, 64 * B), max(16384, 1024 * B))
    i64 = ctypes.c_int64
    while True:
        pcb = np.zeros(ccap + 1, dtype=np.int32)
        plits = np.zeros(lcap, dtype=np.int32)
        rc = L.satmi_dpll_refutations_host(
            B, _p(batch.inst_clause_begin), _p(batch.clause_lit_begin), _p(batch.lits), _p(batch.inst_nvars),
            int(max_solutions), int(node_limit), float(time_limit), int(sol_cap), int(stride), _p(status),
            _p(counters, i64), _p(sol_len), _p(sol_lits), _p(root_len), _p(root_lits), _p(pib), _p(pcb), int(ccap),
            _p(plits), int(lcap), _p(info, i64), _p(totals, i64))
        _capi.check(rc, "satmi_dpll_refutations_host")
        if B == 0 or (int(totals[0]) <= ccap and int(totals[1]) <= lcap):
            break
        # truncated: again with 4x the room
        ccap, lcap = max(4 * ccap, int(totals[0])), max(4 * lcap, int(totals[1]))
    P = int(pib[B]) if B else 0
    proof = CnfBatch(pib, pcb[:P + 1].copy(), plits[:max(int(pcb[P]), 1)].copy(),   # (as pack: never an empty array)
                     np.zeros(B, dtype=np.int32))   # (inst_nvars of a proof batch: unused by the checks)
    return DpllResult(status, counters, sol_len, sol_lits, root_len, root_lits), proof, info


def dpll_refutations(formulas, max_solutions=1, node_limit=0, time_limit=0.0, mode="sound", inits=None, room=None):
    """Sound DPLL on `formulas` (a CnfBatch or a list of formulas) with its refutations.  One
    dict per formula: "status" (_capi.DPLL_*), "counters" (name -> count), "sat" (True: a
    model was found; False: exhausted without one; None: a limit stopped the search),
    "model" (signed literals in assignment order, or None), "root" (the assignment after
    the root's unit propagation), "proof" (the lemma clauses that refute the formula, the
    empty clause last: what check_refutations verifies; None unless sat is False) and
    "lemmas" / "log_words" (what the search logged)."""
    batch = formulas if isinstance(formulas, CnfBatch) else pack(formulas)
    r, proof, info = dpll_refutations_packed(batch, max_solutions, node_limit, time_limit, None, mode, inits, room)
    out = []
    for b in range(batch.num_instances):
        nsol = r.num_solutions(b)
        st = int(r.status[b])
        sat = True if nsol > 0 else False if st == _capi.DPLL_EXHAUSTED else None
        out.append({"status": st, "counters": r.counter_dict(b), "sat": sat,
                    "model": r.solutions(b)[0] if nsol > 0 else None, "root": r.root_assignment(b),
                    "proof": [list(c) for c in proof.instance(b)] if sat is False else None,
                    "lemmas": int(info[b, 0]), "log_words": int(info[b, 1])})
    return out


def proof_of_dpll(r):
    """The proof in a dpll_refutations dict: the logged lemmas of an UNSAT answer."""
    if r.get("sat") is not False or r.get("proof") is None:
        raise ValueError("proof_of_dpll: the search did not end exhausted without a model: it has no refutation")
    return [list(c) for c in r["proof"]]


def proof_of_cdcl(r):
    """The proof in a cdcl_sound.cdcl_sound_batch dict: the learned clauses of an UNSAT answer,
    in learning order, the empty clause last."""
    if r.get("sat") is not False or r.get("proof") is None:
        raise ValueError("proof_of_cdcl: the search did not end UNSAT: it has no refutation")
    return [list(c) for c in r["proof"]]


def proof_of_cdcl_assumed(formula, r):
    """The refutation in a cdcl_sound.cdcl_assume_batch dict that is unsatisfiable under its
    assumptions, as the pair check_refutations / trim_refutations take: (the formula plus
    the core's literals as unit clauses, the learned clauses in learning order, the empty
    clause last).  Every lemma but the last follows from the formula alone; the empty clause
    needs the core.  For a plain UNSAT answer the core is empty and the pair is the formula
    and proof_of_cdcl's list.  Built on the host."""
    if r.get("sat") is not False or r.get("proof") is None or r.get("core") is None:
        raise ValueError("proof_of_cdcl_assumed: the search did not end UNSAT or unsatisfiable under its "
                         "assumptions: it has no refutation")
    if r.get("core_len", len(r["core"])) != len(r["core"]):
        raise ValueError("proof_of_cdcl_assumed: the core was cut at core_stride")
    return [list(c) for c in formula] + [[int(l)] for l in r["core"]], [list(c) for c in r["proof"]]


def dpll_refutations_device(num_instances, icb, clb, lits, inst_nvars, max_vars, max_clauses, max_lits,
                            max_clause_len, status, counters, sol_len, sol_lits, root_len, root_lits, sol_cap,
                            sol_stride, log, log_begin, proof_icb, proof_clb, proof_clause_cap, proof_lits,
                            proof_lit_cap, info, totals, max_solutions=1, node_limit=0, time_limit=0.0, stream=None):
    """satmi_dpll_refutations_device on device pointers (ints, e.g. a tensor's data_ptr());
    asynchronous on `stream`.  The proof triple it writes is what check_refutations_device
    and trim_refutations_device read, on the same stream with no copy."""
    rc = _capi.load().satmi_dpll_refutations_device(
        int(num_instances), icb, clb, lits, inst_nvars, int(max_vars), int(max_clauses), int(max_lits),
        int(max_clause_len), int(max_solutions), int(node_limit), float(time_limit), int(sol_cap), int(sol_stride),
        status, counters, sol_len, sol_lits, root_len, root_lits, log, log_begin, proof_icb, proof_clb,
        int(proof_clause_cap), proof_lits, int(proof_lit_cap), info, totals, stream)
    _capi.check(rc, "satmi_dpll_refutations_device")
