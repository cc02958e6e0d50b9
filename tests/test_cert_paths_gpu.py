"""Every verdict at the Davis-Putnam and resolution path rows, certified on the
GPU: the rows of tests/cert_rows.py (tests/test_cert_rows.py holds the
selection to facts) are solved once with record=True, and the record goes
through the code between a record and its certificate (proof_of_elimination,
proof_of_resolution, record_of, stages_of_elimination, stages_of_resolution)
into the certifier kernels, at sizes their own suites do not reach: ids up to
11,100, records of up to 121,767 clauses, proofs of 45,150 lemmas, propagation
trails of more than 256 entries (with the trail of csrc/trim.hip wrapped at 256
entries the chain_300 rows fail, the trim answering PROVEN for a satisfiable
formula; chain_257 does not get past 256), 300 stages that tile a 45,000-clause
record.

  True   csrc/witness.hip rebuilds a model; it satisfies every clause in plain
         Python (exact), passes csrc/check.hip, no stage is stuck; host form,
         both device forms and a one-wave grid agree word for word.
  False  csrc/trim.hip answers PROVEN; its core with the kept lemmas passes
         csrc/refute.hip and the plain propagation of cert_rows.Rup; the core is
         unsatisfiable by cert_rows.unsat_by_oracle; a chain's core is every
         clause.  The whole record passes the forward check, every lemma
         verified, in the host form and both device forms.
  Soundness   no PROVEN and no MODEL for what is not: the record of a chain
         against the chain without one clause (a satisfiable formula), a True
         row's record closed with [], a False answer forged into True.

The forward check of a whole record by one wavefront, measured once per row on
an MI355X (host form, copies included): 0.71 s for php65 (26,694 lemmas of up
to 8 literals), 0.17 s for chain_300_unsat (45,150 lemmas), 0.12 s at 33,000,
0.06 s at 18,500, 0.02 s and less up to 8,385.  No row is left out for time.

Tests above 5 s on an MI355X: the whole-record forward check of php65, 14.5 s --
the one row at the clause forms' threshold, whose 26,694 lemmas of up to 8
literals also go through the wave-per-clause form (max_clause_len = 0), one
wavefront for them all, and through three Python conversions of 190,000
literals; and the witness of pairbuf_wide, 5.6 s -- 281 stages that each read
5,202 clauses, one of 200 literals, seven times over the forms and grids.  The
chain_300 soundness cases take 4.7 s each (nine launches over 45,150 lemmas)."""
import functools

import pytest

import cert_rows as C
import refute_rows as rr
import test_refute_gpu as RG
import test_trim_gpu as TG
import test_witness_gpu as WG
import trim_rows as tr
import witness_rows as wr
from satmi import _capi
from satmi import dp as dp_mod
from satmi import resolution as res_mod
from satmi.check import check_models
from satmi.refute import (check_refutations, proof_of_elimination, proof_of_resolution, trim_debug_grid,
                          trim_refutations)
from satmi.solvers import (davis_putnam_witness, davis_putnam_witness_batch, resolution_witness,
                           resolution_witness_batch)
from satmi.witness import debug_grid, record_of, stages_of_elimination, stages_of_resolution, witness_models

pytestmark = pytest.mark.gpu

GRIDS = ((0, 0), (1, 1))
TRUE_ROWS, FALSE_ROWS = C.table_rows(1), C.table_rows(0)
ROWS = TRUE_ROWS + FALSE_ROWS
TABLE = {r: C.table(*r)[0] for r in ROWS}
SMALL_TRUE_DP = [n for n, t in C.DP_TABLE.items() if t[0] == 1 and t[1] <= C.FORWARD_P_MAX]
KIND = {"dp": (proof_of_elimination, stages_of_elimination, False, davis_putnam_witness),
        "res": (proof_of_resolution, stages_of_resolution, True, resolution_witness)}


def _id(r):
    return "-".join(r)


def test_the_selection():
    assert len(TRUE_ROWS) >= 10 and len(FALSE_ROWS) >= 10 and sorted(ROWS) == sorted(C.rows())
    assert SMALL_TRUE_DP == ["chain_64_sat", "chain_65_sat", "chain_128_sat", "chain_129_sat", "disjoint_70"]


@functools.lru_cache(maxsize=None)
def solved(kind, name):
    """The kernel's recorded run of a row, once per process, as the row's own GPU test runs it."""
    f = C.formula(kind, name)
    r = dp_mod.eliminate(f, record=True) if kind == "dp" else res_mod.resolve(f, record=True)
    assert r["result"] == TABLE[(kind, name)], name
    return r


def _mv(f, rec):
    return max(abs(l) for c in f + rec for l in c)


def _mcl(f, rec):
    return max(len(c) for c in f + rec)


# ------------------------------------------------------------------ True rows: witness
def witness_all_forms(f, rec, stages, ho):
    """Host form, device form at the true max_clause_len and at 0, each under the default grid and
    one wave: identical words, lengths and rows (guard words asserted by the runners)."""
    stride = len(C.variables(f))
    mv = _mv(f, rec)
    want = WG.run_host([f], [rec], [stages], ho, stride)
    try:
        for grid in GRIDS:
            debug_grid(*grid)
            assert WG.run_host([f], [rec], [stages], ho, stride) == want, grid
            for mcl in (_mcl(f, rec), 0):
                assert WG.run_device([f], [rec], [stages], ho, mv, mcl, stride) == want, (grid, mcl)
    finally:
        debug_grid(0, 0)
    return want


@pytest.mark.parametrize("row", TRUE_ROWS, ids=_id)
def test_true_rows_give_models(row):
    kind, name = row
    _, stages_of, ho, entry = KIND[kind]
    f, r = C.formula(*row), solved(*row)
    rec, stages = record_of(r), stages_of(f, r)
    assert len(rec) == C.table(*row)[1]
    (w,) = witness_models([f], [rec], [stages], ho)
    assert [w[k] for k in _capi.WITNESS_WORDS] == [wr.MODEL, 0, -1, 0, 0, -1] and w["ok"], w
    model = w["model"]
    assert [abs(l) for l in model] == C.variables(f)
    assert C.satisfies(f, model) and C.falsified(f, model) == []
    assert check_models([f], [[model]])[0][0]["ok"]
    words, lens, rows_ = witness_all_forms(f, rec, stages, ho)
    assert words == [[wr.MODEL, 0, -1, 0, 0, -1]] and lens == [len(model)] and rows_ == [model]
    assert entry(f) == (True, {abs(l): l > 0 for l in model})


# ------------------------------------------------------------------ False rows: trim, then the forward check of what it kept
def trim_all_forms(f, p):
    """test_trim_gpu.trim_both_forms for one large instance: the device form at the true
    max_clause_len (with the host form beside it) and at 0, each under the default grid and one
    wave, identical within a form.  Returns {max_clause_len: (words, core marks, lemma marks)}."""
    mv = rr.max_vars_of(f, p)
    got = {}
    try:
        for mcl in (_mcl(f, p), 0):
            runs = []
            for grid in GRIDS:
                trim_debug_grid(*grid)
                runs.append(TG.run_device([f], [p], mv, mcl))
                if mcl:
                    runs.append(TG.run_host([f], [p]))
            assert all(x == runs[0] for x in runs[1:]), mcl
            (words,), core, lemma = runs[0]
            got[mcl] = (words, core, lemma)
    finally:
        trim_debug_grid(0, 0)
    return got


@functools.lru_cache(maxsize=None)
def _core_is_certified(f, p, core_idx, kept_idx):
    """What tests/trim_rows.py's check_properties asks of a PROVEN answer, with the plain
    propagation of cert_rows.Rup in place of the naive rounds; then the forward check on the GPU
    and the oracle's verdict of the core.  (Cached: the two clause forms often agree.)"""
    core, kept = [list(f[i]) for i in core_idx], [list(p[j]) for j in kept_idx]
    assert kept[-1] == [] and C.rup_proof(core, kept)
    (chk,) = check_refutations([core], [kept])
    assert chk["proven"] and chk["failed"] == 0, chk
    assert C.unsat_by_oracle(core) and C.plain_unsat(core)
    return True


def assert_proven(f, p, words, core, lemma):
    """tests/trim_rows.py's check_properties for an answer that must be PROVEN."""
    end = p.index([])
    assert len(words) == tr.NWORDS and len(core) == len(f) and len(lemma) == len(p)
    assert set(core) <= {0, 1} and set(lemma) <= {-1, 1}
    assert words == [rr.PROVEN, 0, -1, 0, sum(core), sum(x >= 0 for x in lemma)]
    assert lemma[end] == 1 and all(x == -1 for x in lemma[end + 1:])
    ft, pt = tuple(map(tuple, f)), tuple(map(tuple, p))
    assert _core_is_certified(ft, pt, tuple(i for i, x in enumerate(core) if x), tuple(j for j, x in enumerate(lemma) if x >= 0))


@pytest.mark.parametrize("row", FALSE_ROWS, ids=_id)
def test_false_rows_trim_to_a_certified_core(row):
    kind, name = row
    proof_of = KIND[kind][0]
    f, r = C.formula(*row), solved(*row)
    p = proof_of(r)
    assert p[-1] == [] and [] not in p[:-1] and len(p) == C.table(*row)[1] + 1
    (t,) = trim_refutations([f], [p])
    if row in C.UNSOUND_FALSE:                # False for a satisfiable formula: nothing may be PROVEN
        assert not t["proven"] and t["failed"] >= 1 and not check_refutations([f], [p])[0]["proven"]
        for mcl, (words, core, lemma) in trim_all_forms(f, p).items():
            assert words[0] == rr.FAILED and words[1] == lemma.count(0) >= 1, mcl
        return
    assert t["proven"] and t["failed"] == 0 and t["first_failed"] == -1 and t["flags"] == 0
    for mcl, (words, core, lemma) in trim_all_forms(f, p).items():
        assert_proven(f, p, words, core, lemma)
        if name in C.chain_unsat_rows():      # minimally unsatisfiable: the core is every clause
            assert core == [1] * len(f), mcl
    assert t["core"] and t["proof"][-1] == []


@pytest.mark.parametrize("row", FALSE_ROWS, ids=_id)
def test_false_rows_whole_record_through_the_forward_check(row):
    """Every lemma of the record verified, up to and including the empty one: host form and both
    device forms (test_refute_gpu.check_all), and the dict form."""
    kind, name = row
    f, p = C.formula(*row), KIND[kind][0](solved(*row))
    RG.check_all([f], [p], want=([[rr.PROVEN, 0, -1, 0]], [1] * len(p)))
    (chk,) = check_refutations([f], [p], lemmas=True)
    assert chk["proven"] and chk["lemma_ok"] == [1] * len(p)


def test_forward_rows_are_covered():
    """The rows the whole-record check must never lose (cert_rows.forward_rows, pinned on the CPU)."""
    assert {"many_20", "chain_64_unsat", "chain_65_unsat", "chain_128_unsat", "chain_129_unsat", "php65"} <= \
        {n for _, n in FALSE_ROWS}


# ------------------------------------------------------------------ soundness at size
def first_plain_failure(g, p):
    """The first lemma of p that the plain propagation does not verify against g and the lemmas before it."""
    rup = C.Rup(g)
    for j, lemma in enumerate(p):
        if not rup.conflict(lemma):
            return j
        rup.add(lemma)
    return -1


def fails_alone(g, p, j):
    """tests/refute_rows.py's rule on lemma j alone, against the premises before it."""
    return not rr.propagates_to_conflict([set(c) for c in g + p[:j]], {-l for l in p[j]})


@pytest.mark.parametrize("which", [0, 1, 2], ids=["no_x1", "no_not_xn", "no_link"])
@pytest.mark.parametrize("name", C.chain_unsat_rows())
def test_a_chains_record_proves_nothing_of_the_chain_without_one_clause(name, which):
    """The reduced formula is satisfiable (tests/test_cert_rows.py shows the model): the unchanged
    record must come out FAILED, forwards and backwards, in every form, and the lemma each check
    points at fails by the plain rule."""
    f, p = C.formula("dp", name), proof_of_elimination(solved("dp", name))
    g = C.drop_clause(f, C.chain_positions(name)[which])
    assert C.satisfies(g, C.chain_model(name, which))
    first = first_plain_failure(g, p)
    assert first >= 0 and fails_alone(g, p, first)
    mv, mcl = rr.max_vars_of(g, p), _mcl(g, p)
    runs = [RG.run_host([g], [p]), RG.run_device([g], [p], mv, mcl), RG.run_device([g], [p], mv, 0)]
    assert runs[1] == runs[0] and runs[2] == runs[0]
    (words,), ok = runs[0]
    assert words[0] == rr.FAILED and words[1] >= 1 and words[1] == ok.count(0) and words[3] == 0
    assert words[2] == first == ok.index(0)               # exact: the forward check has one answer
    for form, (words, core, lemma) in trim_all_forms(g, p).items():
        assert words[0] == rr.FAILED and words[1] >= 1 and words[1] == lemma.count(0), form
        assert words[2] == lemma.index(0) and fails_alone(g, p, words[2]), form
        assert ok[words[2]] == 0 and all(ok[j] == 0 for j, x in enumerate(lemma) if x == 0), form


@pytest.mark.parametrize("name", SMALL_TRUE_DP)
def test_a_true_rows_record_closed_with_the_empty_clause_fails(name):
    """Every recorded clause is a resolvent of two before it and verifies; [] follows from nothing
    a satisfiable formula implies: exactly that lemma fails."""
    f, r = C.formula("dp", name), solved("dp", name)
    p = record_of(r) + [[]]
    assert C.satisfies(f, witness_models([f], [record_of(r)], [stages_of_elimination(f, r)])[0]["model"])
    want = ([[rr.FAILED, 1, len(p) - 1, 0]], [1] * (len(p) - 1) + [0])
    RG.check_all([f], [p], want=want)
    for form, (words, core, lemma) in trim_all_forms(f, p).items():
        assert words == [rr.FAILED, 1, len(p) - 1, 0, 0, 1] and not any(core), form
        assert lemma == [-1] * (len(p) - 1) + [0], form


@pytest.mark.parametrize("row", FALSE_ROWS, ids=_id)
def test_a_false_answer_forged_into_true_gives_no_model(row, monkeypatch):
    kind, name = row
    _, stages_of, ho, entry = KIND[kind]
    f = C.formula(*row)
    forged = dict(solved(*row), result=1)
    rec, stages = record_of(forged), stages_of(f, forged)
    (w,) = witness_models([f], [rec], [stages], ho)
    assert w["status"] == wr.NOT_MODEL and not w["ok"] and w["falsified"] >= 1
    bad = C.falsified(f, w["model"])
    assert len(bad) == w["falsified"] and bad[0] == w["first_falsified"]
    words, _, rows_ = witness_all_forms(f, rec, stages, ho)
    assert words == [[w[k] for k in _capi.WITNESS_WORDS]] and rows_ == [w["model"]]
    monkeypatch.setattr(dp_mod if kind == "dp" else res_mod, "eliminate" if kind == "dp" else "resolve",
                        lambda *a, **k: forged)
    with pytest.raises(_capi.SatmiError, match="falsifies %d of its clauses" % w["falsified"]):
        entry(f)


# ------------------------------------------------------------------ batched rows
@pytest.mark.parametrize("name", list(C.batch_rows()))
def test_batched_rows(name, monkeypatch):
    """One batched solve of the list with its record; every True answer through one witness
    launch, every False answer through one trim and one forward check, with the assertions of
    the single rows.  The answers the reference gets wrong (cert_rows.BATCH_UNSOUND: True for a
    formula with the empty clause, False by resolving on a tautology) come out NOT_MODEL and
    FAILED.  Instances handed to the single-call path are certified from the record it returns."""
    kind, fs, cap = C.batch_rows()[name]
    proof_of, stages_of, ho, _ = KIND[kind]
    mod = dp_mod if kind == "dp" else res_mod
    solve = mod.eliminate_batch if kind == "dp" else mod.resolve_batch
    try:
        mod.debug_batch(0, cap)
        rs = solve(fs, record=True)
    finally:
        mod.debug_batch(0, 0)
    assert tuple(r["result"] for r in rs) == C.batch_verdicts(name)
    if name in ("dp_edge", "dp_capacity", "dp_wave"):
        assert {r["path"] for r in rs} == {"batch", "single"}
    unsound_true, unsound_false = C.BATCH_UNSOUND.get(name, ((), ()))
    true = [b for b, r in enumerate(rs) if r["result"] == 1]
    false = [b for b, r in enumerate(rs) if r["result"] == 0]
    assert true and false                                  # (no list lacks a verdict: cert_rows.BATCH_COUNTS)

    # True answers: one witness launch, one model check
    tf = [fs[b] for b in true]
    recs, sts = [record_of(rs[b]) for b in true], [stages_of(fs[b], rs[b]) for b in true]
    ws = witness_models(tf, recs, sts, ho)
    checked = check_models(tf, [[w["model"]] for w in ws])
    for b, f, w, c in zip(true, tf, ws, checked):
        assert w["flags"] == 0, (name, b)
        if b in unsound_true:
            assert w["status"] == wr.NOT_MODEL and w["falsified"] >= 1 and not c[0]["ok"], (name, b)
            assert C.falsified(f, w["model"])[0] == w["first_falsified"], (name, b)
        else:
            assert [w[k] for k in _capi.WITNESS_WORDS] == [wr.MODEL, 0, -1, 0, 0, -1], (name, b, f)
            assert C.satisfies(f, w["model"]) and c[0]["ok"], (name, b)
    try:
        for grid in GRIDS:                                 # host and both device forms against the plain rule
            debug_grid(*grid)
            words, _, rows_ = WG.check_all(tf, recs, sts, ho)
            assert words == [[w[k] for k in _capi.WITNESS_WORDS] for w in ws] and rows_ == [w["model"] for w in ws]
    finally:
        debug_grid(0, 0)

    # False answers: one trim, one forward check of the cores, one of the whole records
    ff, ps = [fs[b] for b in false], [proof_of(rs[b]) for b in false]
    sound = [b not in unsound_false for b in false]
    got = TG.trim_both_forms(ff, ps, grids=GRIDS)          # (every property of tests/trim_rows.py, both forms)
    for words, _, _ in got.values():
        assert [w[0] == rr.PROVEN for w in words] == sound and all(w[0] != rr.OPEN for w in words)
    ts = trim_refutations(ff, ps)
    assert [t["proven"] for t in ts] == sound
    cores = [([f[c] for c in t["core"]], t["proof"]) for f, t, s in zip(ff, ts, sound) if s]
    for chk in check_refutations([c for c, _ in cores], [k for _, k in cores]):
        assert chk["proven"] and chk["failed"] == 0
    for core, kept in cores:
        assert C.unsat_by_oracle(core) and kept[-1] == []
    words, oks = RG.check_all(ff, ps)                      # (against tests/refute_rows.py's evaluator)
    assert [w == [rr.PROVEN, 0, -1, 0] for w in words] == sound and -1 not in oks
    for f, s in zip(ff, sound):
        assert C.unsat_by_oracle(f) == s

    # the sound False answers forged into True: no model, and the entry point refuses
    fb = [b for b, s in zip(false, sound) if s]
    forged = [dict(rs[b], result=1) for b in fb]
    gf = [fs[b] for b in fb]
    ws = witness_models(gf, [record_of(r) for r in forged], [stages_of(f, r) for f, r in zip(gf, forged)], ho)
    for f, w in zip(gf, ws):
        assert w["status"] == wr.NOT_MODEL and w["falsified"] >= 1
        assert C.falsified(f, w["model"])[0] == w["first_falsified"]
    monkeypatch.setattr(mod, "eliminate_batch" if kind == "dp" else "resolve_batch", lambda *a, **k: forged)
    with pytest.raises(_capi.SatmiError, match="formula 0"):
        (davis_putnam_witness_batch if kind == "dp" else resolution_witness_batch)(gf)
