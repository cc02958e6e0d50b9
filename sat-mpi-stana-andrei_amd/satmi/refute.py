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
"""
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


def check_refutations_device(num_instances, icb, clb, lits, proof_icb, proof_clb, proof_lits, max_vars,
                             max_clause_len, out, lemma_ok=None, stream=None):
    """satmi_check_refutations_device on device pointers (ints, e.g. a tensor's data_ptr();
    `lemma_ok` may be None); asynchronous on `stream`."""
    rc = _capi.load().satmi_check_refutations_device(int(num_instances), icb, clb, lits, proof_icb, proof_clb,
                                                     proof_lits, int(max_vars), int(max_clause_len), out, lemma_ok,
                                                     stream)
    _capi.check(rc, "satmi_check_refutations_device")


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
