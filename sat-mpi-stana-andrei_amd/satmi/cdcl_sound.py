"""Sound CDCL on the GPU (libsatmi.so, csrc/cdcl_sound.hip): a clause-learning search,
one wavefront per formula, whose learned clauses are its refutation.

Unlike satmi.cdcl, the reference's CDCLSolver step for step, this is a decision
procedure.  A SAT answer carries a model that check.check_models accepts; an UNSAT
answer carries the learned clauses in learning order, closed by the empty clause,
which refute.check_refutations and refute.trim_refutations verify.  Every output is
a function of the formula alone: include/satmi.h states the search rule in full and
tests/cdcl_sound_rows.py restates it in Python.
"""
import ctypes

import numpy as np

from . import _capi
from ._batch import _p
from .cnf import CnfBatch, pack


def debug_grid(workgroups=0, waves_per_wg=0):
    """Test knob (0 = default): at most `workgroups` workgroups of `waves_per_wg` (1, 2, 4) wavefronts."""
    _capi.check(_capi.load().satmi_cdcl_sound_debug_grid(int(workgroups), int(waves_per_wg)),
                "satmi_cdcl_sound_debug_grid")


def debug_room(words=0):
    """Test knob (0 = default): the region words every formula gets in the host form's first run."""
    _capi.check(_capi.load().satmi_cdcl_sound_debug_room(int(words)), "satmi_cdcl_sound_debug_room")


def lds_bytes(max_vars):
    """LDS bytes one wavefront needs at this max_vars (0 = beyond CDCL_SOUND_MAX_VARS)."""
    return int(_capi.load().satmi_cdcl_sound_lds_bytes(int(max_vars)))


def cdcl_sound_packed(batch, conflict_limit=0, time_limit=0.0, room_cap=0, room=None):
    """satmi_cdcl_sound_batch_host on a CnfBatch.  Returns (status int32 [B], counters int64
    [B, 8]: _capi.CDCL_SOUND_COUNTERS, row_len int32 [B], row_lits int32 [B, stride], proof
    CnfBatch, info int64 [B, 4]: _capi.CDCL_SOUND_WORDS).  Formula b's lemmas are "formula" b of
    the proof batch: the refutation of an UNSAT instance, else no lemma.  `room_cap` = the most
    region words a formula may take (0 = no cap of the caller's): one that needs more ends
    CDCL_SOUND_FULL.  `room` = (lemmas, literals) the first call's proof arrays hold; a proof that
    outgrows them is asked for again with 4x the room (the totals, if those are more)."""
    L = _capi.load()
    _capi.require_gpu()
    B = batch.num_instances
    stride = max(1, int(batch.inst_nvars.max(initial=0)))
    status = np.zeros(B, dtype=np.int32)
    counters = np.zeros((B, _capi.CDCL_SOUND_NCOUNTERS), dtype=np.int64)
    row_len = np.zeros(B, dtype=np.int32)
    row_lits = np.zeros((B, stride), dtype=np.int32)
    info = np.zeros((B, _capi.CDCL_SOUND_NWORDS), dtype=np.int64)
    totals = np.zeros(2, dtype=np.int64)
    pib = np.zeros(B + 1, dtype=np.int32)
    ccap, lcap = room if room is not None else (max(1024, 64 * B), max(16384, 1024 * B))
    i64 = ctypes.c_int64
    while True:
        pcb = np.zeros(ccap + 1, dtype=np.int32)
        plits = np.zeros(lcap, dtype=np.int32)
        rc = L.satmi_cdcl_sound_batch_host(
            B, _p(batch.inst_clause_begin), _p(batch.clause_lit_begin), _p(batch.lits), _p(batch.inst_nvars),
            int(conflict_limit), float(time_limit), int(room_cap), _p(status), _p(counters, i64), _p(row_len),
            _p(row_lits), int(stride), _p(pib), _p(pcb), int(ccap), _p(plits), int(lcap), _p(info, i64),
            _p(totals, i64))
        _capi.check(rc, "satmi_cdcl_sound_batch_host")
        if B == 0 or (int(totals[0]) <= ccap and int(totals[1]) <= lcap):
            break
        ccap, lcap = max(4 * ccap, int(totals[0])), max(4 * lcap, int(totals[1]))
    P = int(pib[B]) if B else 0
    proof = CnfBatch(pib, pcb[:P + 1].copy(), plits[:max(int(pcb[P]), 1)].copy(),   # (as pack: never an empty array)
                     np.zeros(B, dtype=np.int32))   # (inst_nvars of a proof batch: unused by the checks)
    return status, counters, row_len, row_lits, proof, info


def cdcl_sound_batch(formulas, conflict_limit=0, time_limit=0.0, room_cap=0, room=None):
    """Sound CDCL on `formulas` (a CnfBatch or a list of formulas).  One dict per formula:
    "status" (_capi.CDCL_SOUND_*), "sat" (True / False / None: a limit, a full region or the
    layout stopped the search), "counters" (name -> count), "model" (one signed literal per
    variable of the formula, ascending, or None), "proof" (the learned clauses in learning
    order, the empty clause last: what check_refutations verifies; None unless sat is False)
    and "records" / "region_words" (what the search needed of its region)."""
    batch = formulas if isinstance(formulas, CnfBatch) else pack(formulas)
    status, counters, row_len, row_lits, proof, info = cdcl_sound_packed(batch, conflict_limit, time_limit,
                                                                        room_cap, room)
    out = []
    for b in range(batch.num_instances):
        st = int(status[b])
        sat = True if st == _capi.CDCL_SOUND_SAT else False if st == _capi.CDCL_SOUND_UNSAT else None
        out.append({"status": st, "sat": sat,
                    "counters": dict(zip(_capi.CDCL_SOUND_COUNTERS, map(int, counters[b]))),
                    "model": row_lits[b, :int(row_len[b])].tolist() if sat else None,
                    "proof": [list(c) for c in proof.instance(b)] if sat is False else None,
                    "records": int(info[b, 0]), "region_words": int(info[b, 1])})
    return out


def cdcl_sound_device(num_instances, icb, clb, lits, inst_nvars, max_vars, max_clause_len, lemmas, lemma_begin,
                      status, counters, row_len, row_lits, stride, info, conflict_limit=0, time_limit=0.0,
                      stream=None):
    """satmi_cdcl_sound_batch_device on device pointers (ints, e.g. a tensor's data_ptr());
    asynchronous on `stream`."""
    rc = _capi.load().satmi_cdcl_sound_batch_device(
        int(num_instances), icb, clb, lits, inst_nvars, int(max_vars), int(max_clause_len), int(conflict_limit),
        float(time_limit), lemmas, lemma_begin, status, counters, row_len, row_lits, int(stride), info, stream)
    _capi.check(rc, "satmi_cdcl_sound_batch_device")


# ---- under assumptions (satmi_cdcl_assume_*): failed-assumption cores with proofs
def pack_assumptions(assumptions, num_instances):
    """Per-formula assumption lists -> (assume_begin int32 [B + 1], assume_lits int32, never
    empty, the largest variable per formula int32 [B]).  None = no assumptions anywhere."""
    lists = [[] for _ in range(num_instances)] if assumptions is None else [list(a) for a in assumptions]
    if len(lists) != num_instances:
        raise ValueError("assumptions must have one list of literals per formula")
    begin = np.zeros(num_instances + 1, dtype=np.int32)
    np.cumsum([len(a) for a in lists], out=begin[1:])
    flat = [int(l) for a in lists for l in a]
    if any(l == 0 or not -2 ** 31 < l < 2 ** 31 for l in flat):
        raise ValueError("assumption literals must be nonzero and within int32 (INT32_MIN excluded)")
    top = np.array([max([abs(int(l)) for l in a] + [0]) for a in lists], dtype=np.int32)
    return begin, np.array(flat or [0], dtype=np.int32), top


def cdcl_assume_packed(batch, assume_begin, assume_lits, conflict_limit=0, time_limit=0.0, room_cap=0, room=None,
                       core_stride=None):
    """satmi_cdcl_assume_batch_host on a CnfBatch whose inst_nvars cover the assumptions'
    variables, formula b under assume_lits[assume_begin[b] : assume_begin[b + 1]] in that order.
    Returns cdcl_sound_packed's six and (core_len int32 [B], core_lits int32 [B, core_stride]):
    the failed assumptions of a formula that ended CDCL_SOUND_ASSUMED, whose lemmas are in the
    proof batch like those of an UNSAT one.  `core_stride` defaults to the longest assumption
    list, which holds every core."""
    L = _capi.load()
    _capi.require_gpu()
    B = batch.num_instances
    assume_begin = np.ascontiguousarray(assume_begin, dtype=np.int32)
    assume_lits = np.ascontiguousarray(assume_lits, dtype=np.int32)
    stride = max(1, int(batch.inst_nvars.max(initial=0)))
    if core_stride is None:
        core_stride = max(1, int(np.diff(assume_begin).max(initial=0)))
    status = np.zeros(B, dtype=np.int32)
    counters = np.zeros((B, _capi.CDCL_SOUND_NCOUNTERS), dtype=np.int64)
    row_len = np.zeros(B, dtype=np.int32)
    row_lits = np.zeros((B, stride), dtype=np.int32)
    core_len = np.zeros(B, dtype=np.int32)
    core_lits = np.zeros((B, max(core_stride, 1)), dtype=np.int32)
    info = np.zeros((B, _capi.CDCL_SOUND_NWORDS), dtype=np.int64)
    totals = np.zeros(2, dtype=np.int64)
    pib = np.zeros(B + 1, dtype=np.int32)
    ccap, lcap = room if room is not None else (max(1024, 64 * B), max(16384, 1024 * B))
    i64 = ctypes.c_int64
    while True:
        pcb = np.zeros(ccap + 1, dtype=np.int32)
        plits = np.zeros(lcap, dtype=np.int32)
        rc = L.satmi_cdcl_assume_batch_host(
            B, _p(batch.inst_clause_begin), _p(batch.clause_lit_begin), _p(batch.lits), _p(batch.inst_nvars),
            int(conflict_limit), float(time_limit), int(room_cap), _p(status), _p(counters, i64), _p(row_len),
            _p(row_lits), int(stride), _p(pib), _p(pcb), int(ccap), _p(plits), int(lcap), _p(info, i64),
            _p(totals, i64), _p(assume_begin), _p(assume_lits), _p(core_len), _p(core_lits), int(core_stride))
        _capi.check(rc, "satmi_cdcl_assume_batch_host")
        if B == 0 or (int(totals[0]) <= ccap and int(totals[1]) <= lcap):
            break
        ccap, lcap = max(4 * ccap, int(totals[0])), max(4 * lcap, int(totals[1]))
    P = int(pib[B]) if B else 0
    proof = CnfBatch(pib, pcb[:P + 1].copy(), plits[:max(int(pcb[P]), 1)].copy(), np.zeros(B, dtype=np.int32))
    return status, counters, row_len, row_lits, proof, info, core_len, core_lits[:, :core_stride]


def cdcl_assume_batch(formulas, assumptions, conflict_limit=0, time_limit=0.0, room_cap=0, room=None,
                      core_stride=None):
    """Sound CDCL on `formulas` (a CnfBatch or a list of formulas), formula b under the literals
    `assumptions[b]` in that order (None = none anywhere).  cdcl_sound_batch's dict per formula,
    where "sat" is False for CDCL_SOUND_UNSAT and for CDCL_SOUND_ASSUMED (unsatisfiable under
    the assumptions) alike and both carry "proof", the model is over the variables of formula
    and assumptions, and "core" is the failed assumptions: the refuted one first, then those it
    was refuted from ([] for UNSAT: the formula alone is refuted; None unless sat is False; the
    first `core_stride` literals if that is given and smaller, "core_len" being the count
    whatever was written).  refute.proof_of_cdcl_assumed
    turns such a dict into the pair check_refutations takes."""
    batch = formulas if isinstance(formulas, CnfBatch) else pack(formulas)
    begin, lits, top = pack_assumptions(assumptions, batch.num_instances)
    batch = CnfBatch(batch.inst_clause_begin, batch.clause_lit_begin, batch.lits,
                     np.maximum(np.asarray(batch.inst_nvars, dtype=np.int32), top))
    status, counters, row_len, row_lits, proof, info, core_len, core_lits = cdcl_assume_packed(
        batch, begin, lits, conflict_limit, time_limit, room_cap, room, core_stride)
    out = []
    for b in range(batch.num_instances):
        st = int(status[b])
        sat = True if st == _capi.CDCL_SOUND_SAT else \
            False if st in (_capi.CDCL_SOUND_UNSAT, _capi.CDCL_SOUND_ASSUMED) else None
        out.append({"status": st, "sat": sat,
                    "counters": dict(zip(_capi.CDCL_SOUND_COUNTERS, map(int, counters[b]))),
                    "model": row_lits[b, :int(row_len[b])].tolist() if sat else None,
                    "proof": [list(c) for c in proof.instance(b)] if sat is False else None,
                    "core": core_lits[b, :int(core_len[b])].tolist() if sat is False else None,
                    "core_len": int(core_len[b]),
                    "records": int(info[b, 0]), "region_words": int(info[b, 1])})
    return out


def cdcl_assume_device(num_instances, icb, clb, lits, inst_nvars, max_vars, max_clause_len, lemmas, lemma_begin,
                       status, counters, row_len, row_lits, stride, info, assume_begin, assume_lits, core_len,
                       core_lits, core_stride, conflict_limit=0, time_limit=0.0, stream=None):
    """satmi_cdcl_assume_batch_device on device pointers (ints, e.g. a tensor's data_ptr());
    asynchronous on `stream`."""
    rc = _capi.load().satmi_cdcl_assume_batch_device(
        int(num_instances), icb, clb, lits, inst_nvars, int(max_vars), int(max_clause_len), int(conflict_limit),
        float(time_limit), lemmas, lemma_begin, status, counters, row_len, row_lits, int(stride), info,
        assume_begin, assume_lits, core_len, core_lits, int(core_stride), stream)
    _capi.check(rc, "satmi_cdcl_assume_batch_device")


def assume_pack_device(num_instances, status, lemmas, lemma_begin, info, proof_icb, proof_clb, proof_clause_cap,
                       proof_lits, proof_lit_cap, totals, stream=None):
    """satmi_cdcl_assume_pack_device: pack_device for a cdcl_assume_device solve; the instances
    that ended CDCL_SOUND_ASSUMED have their lemmas in the proof triple too."""
    rc = _capi.load().satmi_cdcl_assume_pack_device(
        int(num_instances), status, lemmas, lemma_begin, info, proof_icb, proof_clb, int(proof_clause_cap),
        proof_lits, int(proof_lit_cap), totals, stream)
    _capi.check(rc, "satmi_cdcl_assume_pack_device")


def pack_device(num_instances, status, lemmas, lemma_begin, info, proof_icb, proof_clb, proof_clause_cap,
                proof_lits, proof_lit_cap, totals, stream=None):
    """satmi_cdcl_sound_pack_device: the regions of a cdcl_sound_device solve as the proof triple
    that check_refutations_device and trim_refutations_device read, on the same stream."""
    rc = _capi.load().satmi_cdcl_sound_pack_device(
        int(num_instances), status, lemmas, lemma_begin, info, proof_icb, proof_clb, int(proof_clause_cap),
        proof_lits, int(proof_lit_cap), totals, stream)
    _capi.check(rc, "satmi_cdcl_sound_pack_device")


# ---- with carried lemmas (satmi_cdcl_carry_*): one query after another on the same formula
def pack_carry(carry, num_instances):
    """Per-formula lists of carried clauses -> the carry triple (inst_begin int32 [B + 1],
    clause_begin int32, lits int32, never empty).  None = nothing carried anywhere."""
    lists = [[] for _ in range(num_instances)] if carry is None else [[list(c) for c in cl] for cl in carry]
    if len(lists) != num_instances:
        raise ValueError("carry must have one list of clauses per formula")
    flat = [int(l) for cl in lists for c in cl for l in c]
    if any(not -2 ** 31 < l < 2 ** 31 for l in flat):
        raise ValueError("carried literals must be within int32 (INT32_MIN excluded)")
    cib = np.zeros(num_instances + 1, dtype=np.int32)
    np.cumsum([len(cl) for cl in lists], out=cib[1:])
    ccb = np.zeros(int(cib[-1]) + 1, dtype=np.int32)
    np.cumsum([len(c) for cl in lists for c in cl], out=ccb[1:])
    top = np.array([max([abs(int(l)) for c in cl for l in c] + [0]) for cl in lists], dtype=np.int32)
    return cib, ccb, np.array(flat or [0], dtype=np.int32), top


def _carry_packed(shrink, batch, assume_begin, assume_lits, carry, conflict_limit, time_limit, room_cap, room,
                  core_stride, kept_room):
    """The host forms with carried lemmas: satmi_cdcl_carry_batch_host, or with `shrink`
    satmi_cdcl_shrink_batch_host, whose words per formula are the tenth value returned."""
    L = _capi.load()
    _capi.require_gpu()
    B = batch.num_instances
    assume_begin = np.ascontiguousarray(assume_begin, dtype=np.int32)
    assume_lits = np.ascontiguousarray(assume_lits, dtype=np.int32)
    cib, ccb, clits = (None, None, None) if carry is None else \
        (np.ascontiguousarray(a, dtype=np.int32) for a in carry)
    stride = max(1, int(batch.inst_nvars.max(initial=0)))
    if core_stride is None:
        core_stride = max(1, int(np.diff(assume_begin).max(initial=0)))
    status = np.zeros(B, dtype=np.int32)
    counters = np.zeros((B, _capi.CDCL_SOUND_NCOUNTERS), dtype=np.int64)
    row_len = np.zeros(B, dtype=np.int32)
    row_lits = np.zeros((B, stride), dtype=np.int32)
    core_len = np.zeros(B, dtype=np.int32)
    core_lits = np.zeros((B, max(core_stride, 1)), dtype=np.int32)
    info = np.zeros((B, _capi.CDCL_SOUND_NWORDS), dtype=np.int64)
    words = np.zeros((B, _capi.CDCL_SHRINK_NWORDS), dtype=np.int64)
    totals = np.zeros(4, dtype=np.int64)
    pib = np.zeros(B + 1, dtype=np.int32)
    kib = np.zeros(B + 1, dtype=np.int32)
    ccap, lcap = room if room is not None else (max(1024, 64 * B), max(16384, 1024 * B))
    carried = (0, 0) if carry is None else (int(cib[-1] - cib[0]), int(ccb[cib[-1]] - ccb[cib[0]]))
    kccap, klcap = kept_room if kept_room is not None else (ccap + carried[0], lcap + carried[1])
    i64 = ctypes.c_int64
    who = "satmi_cdcl_shrink_batch_host" if shrink else "satmi_cdcl_carry_batch_host"
    while True:
        pcb = np.zeros(ccap + 1, dtype=np.int32)
        plits = np.zeros(lcap, dtype=np.int32)
        kcb = np.zeros(kccap + 1, dtype=np.int32)
        klits = np.zeros(max(klcap, 1), dtype=np.int32)
        rc = getattr(L, who)(
            B, _p(batch.inst_clause_begin), _p(batch.clause_lit_begin), _p(batch.lits), _p(batch.inst_nvars),
            int(conflict_limit), float(time_limit), int(room_cap), _p(status), _p(counters, i64), _p(row_len),
            _p(row_lits), int(stride), _p(pib), _p(pcb), int(ccap), _p(plits), int(lcap), _p(info, i64),
            _p(totals, i64), _p(assume_begin), _p(assume_lits), _p(core_len), _p(core_lits), int(core_stride),
            None if cib is None else _p(cib), None if ccb is None else _p(ccb), None if clits is None else _p(clits),
            _p(kib), _p(kcb), int(kccap), _p(klits), int(klcap), *((_p(words, i64),) if shrink else ()))
        _capi.check(rc, who)
        if B == 0 or (int(totals[0]) <= ccap and int(totals[1]) <= lcap and
                      int(totals[2]) <= kccap and int(totals[3]) <= klcap):
            break
        if int(totals[0]) > ccap or int(totals[1]) > lcap:
            ccap, lcap = max(4 * ccap, int(totals[0])), max(4 * lcap, int(totals[1]))
        if int(totals[2]) > kccap or int(totals[3]) > klcap:
            kccap, klcap = max(4 * kccap, int(totals[2])), max(4 * klcap, int(totals[3]))
    P = int(pib[B]) if B else 0
    K = int(kib[B]) if B else 0
    zeros = np.zeros(B, dtype=np.int32)
    proof = CnfBatch(pib, pcb[:P + 1].copy(), plits[:max(int(pcb[P]), 1)].copy(), zeros)
    kept = CnfBatch(kib, kcb[:K + 1].copy(), klits[:max(int(kcb[K]), 1)].copy(), zeros)
    return status, counters, row_len, row_lits, proof, info, core_len, core_lits[:, :core_stride], kept, words


def cdcl_carry_packed(batch, assume_begin, assume_lits, carry=None, conflict_limit=0, time_limit=0.0, room_cap=0,
                      room=None, core_stride=None, kept_room=None):
    """satmi_cdcl_carry_batch_host on a CnfBatch whose inst_nvars cover the variables of the
    assumptions and of the carried clauses; `carry` = the triple (inst_begin, clause_begin,
    lits) of pack_carry, or None.  Returns cdcl_assume_packed's eight and the kept lemmas as a
    CnfBatch: "formula" b of it is what the next query on formula b carries, whatever this
    one's status.  `kept_room` = (lemmas, literals) the first call's kept arrays hold; like the
    proof's, kept arrays that are outgrown are asked for again with 4x the room."""
    return _carry_packed(False, batch, assume_begin, assume_lits, carry, conflict_limit, time_limit, room_cap, room,
                         core_stride, kept_room)[:9]


def _carry_batch(shrink, formulas, assumptions, carry, conflict_limit, time_limit, room_cap, room, core_stride,
                 kept_room):
    batch = formulas if isinstance(formulas, CnfBatch) else pack(formulas)
    B = batch.num_instances
    begin, lits, top = pack_assumptions(assumptions, B)
    cib, ccb, clits, ctop = pack_carry(carry, B)
    batch = CnfBatch(batch.inst_clause_begin, batch.clause_lit_begin, batch.lits,
                     np.maximum(np.maximum(np.asarray(batch.inst_nvars, dtype=np.int32), top), ctop))
    status, counters, row_len, row_lits, proof, info, core_len, core_lits, kept, words = _carry_packed(
        shrink, batch, begin, lits, None if carry is None else (cib, ccb, clits), conflict_limit, time_limit, room_cap,
        room, core_stride, kept_room)
    out = []
    for b in range(B):
        st = int(status[b])
        sat = True if st == _capi.CDCL_SOUND_SAT else \
            False if st in (_capi.CDCL_SOUND_UNSAT, _capi.CDCL_SOUND_ASSUMED) else None
        out.append({"status": st, "sat": sat,
                    "counters": dict(zip(_capi.CDCL_SOUND_COUNTERS, map(int, counters[b]))),
                    "model": row_lits[b, :int(row_len[b])].tolist() if sat else None,
                    "proof": [list(c) for c in proof.instance(b)] if sat is False else None,
                    "core": core_lits[b, :int(core_len[b])].tolist() if sat is False else None,
                    "core_len": int(core_len[b]),
                    "records": int(info[b, 0]), "region_words": int(info[b, 1]), "flags": int(info[b, 2]),
                    "kept": [list(c) for c in kept.instance(b)]})
        if shrink:
            out[-1]["shrink"] = dict(zip(_capi.CDCL_SHRINK_WORDS, map(int, words[b])))
    return out


def cdcl_carry_batch(formulas, assumptions, carry=None, conflict_limit=0, time_limit=0.0, room_cap=0, room=None,
                     core_stride=None, kept_room=None):
    """Sound CDCL on `formulas` under `assumptions`, formula b starting with the clauses
    `carry[b]` as learned clauses (None = nothing carried anywhere): lemmas an earlier query
    on the same formula, or on a subset of its clauses, kept.  cdcl_assume_batch's dict per
    formula (with "flags", the info flags) plus "kept", the list of clauses to carry into the
    next query: the carried ones and those this query learned, whatever its status.  With
    "sat" False, "proof" holds the carried lemmas too: they are part of the refutation, and
    that they follow from the formula is the caller's claim, which check_refutations tests."""
    return _carry_batch(False, formulas, assumptions, carry, conflict_limit, time_limit, room_cap, room, core_stride,
                        kept_room)


def cdcl_carry_device(num_instances, icb, clb, lits, inst_nvars, max_vars, max_clause_len, lemmas, lemma_begin,
                      status, counters, row_len, row_lits, stride, info, assume_begin, assume_lits, core_len,
                      core_lits, core_stride, carry_in, carry_out, conflict_limit=0, time_limit=0.0, stream=None):
    """satmi_cdcl_carry_batch_device on device pointers (ints, e.g. a tensor's data_ptr();
    `carry_in` may be None, or the same array as `carry_out`); asynchronous on `stream`."""
    rc = _capi.load().satmi_cdcl_carry_batch_device(
        int(num_instances), icb, clb, lits, inst_nvars, int(max_vars), int(max_clause_len), int(conflict_limit),
        float(time_limit), lemmas, lemma_begin, status, counters, row_len, row_lits, int(stride), info,
        assume_begin, assume_lits, core_len, core_lits, int(core_stride), carry_in, carry_out, stream)
    _capi.check(rc, "satmi_cdcl_carry_batch_device")


def carry_pack_device(num_instances, lemmas, lemma_begin, carry, kept_icb, kept_clb, kept_clause_cap, kept_lits,
                      kept_lit_cap, totals, stream=None):
    """satmi_cdcl_carry_pack_device: every formula's kept lemmas (its first carry[b] records) as
    a clause triple, on the same stream as the solve."""
    rc = _capi.load().satmi_cdcl_carry_pack_device(
        int(num_instances), lemmas, lemma_begin, carry, kept_icb, kept_clb, int(kept_clause_cap), kept_lits,
        int(kept_lit_cap), totals, stream)
    _capi.check(rc, "satmi_cdcl_carry_pack_device")


# ---- minimal cores (satmi_cdcl_shrink_*): the chain of trial queries of every formula in one launch
def cdcl_shrink_packed(batch, assume_begin, assume_lits, carry=None, conflict_limit=0, time_limit=0.0, room_cap=0,
                       room=None, core_stride=None, kept_room=None):
    """satmi_cdcl_shrink_batch_host: cdcl_carry_packed's arguments and its nine values, the core
    being the minimised one and the counters the chain's, and shrink int64 [B, 6]:
    _capi.CDCL_SHRINK_WORDS."""
    return _carry_packed(True, batch, assume_begin, assume_lits, carry, conflict_limit, time_limit, room_cap, room,
                         core_stride, kept_room)


def cdcl_shrink_batch(formulas, assumptions, carry=None, conflict_limit=0, time_limit=0.0, room_cap=0, room=None,
                      core_stride=None, kept_room=None):
    """cdcl_carry_batch where a formula that is unsatisfiable under its assumptions gets a minimal
    core: after the first query one trial query per core literal runs under the core less that
    literal, each carrying every lemma so far, and a literal stays when its trial is satisfiable
    (or reaches conflict_limit).  cdcl_carry_batch's dict per formula, "core" being the shrunk
    core in the first query's order, "proof" and "kept" the lemmas of the whole chain, the
    counters its sums, and "shrink" the chain's words by name (_capi.CDCL_SHRINK_WORDS): with
    "limit_trials" 0 the core less any one literal is satisfiable with the formula.  A formula
    that a trial refutes without assumptions ends CDCL_SOUND_UNSAT with the core []."""
    return _carry_batch(True, formulas, assumptions, carry, conflict_limit, time_limit, room_cap, room, core_stride,
                        kept_room)


def cdcl_shrink_device(num_instances, icb, clb, lits, inst_nvars, max_vars, max_clause_len, lemmas, lemma_begin,
                       status, counters, row_len, row_lits, stride, info, assume_begin, assume_lits, core_len,
                       core_lits, core_stride, carry_in, carry_out, work_lits, shrink_info, conflict_limit=0,
                       time_limit=0.0, stream=None):
    """satmi_cdcl_shrink_batch_device on device pointers (ints, e.g. a tensor's data_ptr();
    `carry_in` may be None, or the same array as `carry_out`; `work_lits` = two int32 words per
    assumption, `shrink_info` = six int64 words per formula); one launch, asynchronous on `stream`."""
    rc = _capi.load().satmi_cdcl_shrink_batch_device(
        int(num_instances), icb, clb, lits, inst_nvars, int(max_vars), int(max_clause_len), int(conflict_limit),
        float(time_limit), lemmas, lemma_begin, status, counters, row_len, row_lits, int(stride), info,
        assume_begin, assume_lits, core_len, core_lits, int(core_stride), carry_in, carry_out, work_lits, shrink_info,
        stream)
    _capi.check(rc, "satmi_cdcl_shrink_batch_device")
