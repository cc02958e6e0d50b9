"""GPU checks of the sound CDCL (csrc/cdcl_sound.hip) at the rows of tests/cdcl_sound_rows.py:
the kernel is the Python rule exactly, in both clause forms and on a one-wave grid; its
verdicts are sound DPLL's; its models and proofs pass the library's own checkers, in the
host form and in the device pipeline solve -> pack -> check -> trim on one stream, which also
reads every row's region, SAT rows included, against the rule's lemma list."""
import functools
import random
import sys

import numpy as np
import pytest

import cdcl_sound_rows as R
import refute_rows as rr
from satmi import _capi, cdcl_sound, solvers
from satmi.check import check_models
from satmi.cnf import pack
from satmi.dpll import dpll_batch
from satmi.refute import (check_refutations, check_refutations_device, proof_of_cdcl, trim_refutations,
                          trim_refutations_device)

pytestmark = pytest.mark.gpu

ROWS = R.rows()
FORMULA = dict(ROWS)
NAMES = [n for n, _ in ROWS]
# the rows the lane-per-clause form takes: no clause beyond its 8 literals (and small ids, so the
# batch is not laid out for the sparse row's 8,191 variables)
SHORT = [n for n, f in ROWS if max([len(c) for c in f] + [0]) <= R.SHORT_MAX and n != "sparse ids"]
GROUPS = {"all": NAMES, "short": SHORT}     # "all" holds 300-literal clauses: the wave-per-clause form


@functools.lru_cache(maxsize=None)
def want(name):
    return R.solve(FORMULA[name])


@functools.lru_cache(maxsize=None)
def got(group, grid=0):
    """The host form on the group's rows in one call: name -> cdcl_sound_batch dict."""
    cdcl_sound.debug_grid(grid, 1 if grid else 0)
    try:
        return dict(zip(GROUPS[group], cdcl_sound.cdcl_sound_batch([FORMULA[n] for n in GROUPS[group]])))
    finally:
        cdcl_sound.debug_grid(0, 0)


def _same(name, g, w):
    assert g["status"] == w["status"], name
    assert [g["counters"][k] for k in R.COUNTERS] == w["counters"], name
    assert g["model"] == w["model"], name
    if w["status"] == R.UNSAT:
        assert g["proof"] == w["lemmas"], name
    assert g["records"] == len(w["lemmas"]) and g["region_words"] == R.region_words(w["lemmas"]), name


@pytest.mark.parametrize("group,grid", [("all", 0), ("short", 0), ("short", 1)])
def test_kernel_is_the_python_rule(group, grid):
    """Status, counters, model row and the lemma list in order, on every row: in the
    wave-per-clause form ("all"), the lane-per-clause form ("short"), and with one wave
    taking every formula of the batch in turn (grid 1 x 1)."""
    assert len(GROUPS["short"]) > 70 and "long clause" not in GROUPS["short"]
    res = got(group, grid)
    for name in GROUPS[group]:
        _same(name, res[name], want(name))


def test_record_counts_of_sat_rows_that_learned():
    """The host form hands out the lemmas of UNSAT rows only; of a SAT row that learned it reports
    the exact record counts (test_device_form_regions_are_the_python_rules_lemmas reads the
    clauses themselves)."""
    res = got("all")
    learned_sat = [n for n in NAMES if want(n)["status"] == R.SAT and want(n)["lemmas"]]
    assert len(learned_sat) >= 8
    for n in learned_sat:
        assert res[n]["proof"] is None and res[n]["records"] == len(want(n)["lemmas"])


def test_verdicts_are_sound_dplls():
    """(Sound DPLL never looks at an empty clause of its input: the one such row is left out.)"""
    names = [n for n in NAMES if [] not in FORMULA[n]]
    d = dpll_batch([FORMULA[n] for n in names], mode="sound", max_solutions=1)
    res = got("all")
    for b, n in enumerate(names):
        assert int(d.status[b]) in (_capi.DPLL_EXHAUSTED, _capi.DPLL_STOPPED), n
        assert res[n]["sat"] is (d.num_solutions(b) > 0), n


def test_every_answer_is_certified_by_the_librarys_checkers():
    res = got("all")
    sat = [n for n in NAMES if res[n]["sat"]]
    unsat = [n for n in NAMES if res[n]["sat"] is False]
    assert len(sat) + len(unsat) == len(NAMES) and len(sat) >= 8 and len(unsat) >= 8
    for n, c in zip(sat, check_models([FORMULA[n] for n in sat], [[res[n]["model"]] for n in sat])):
        assert c[0]["ok"], n
    fs, ps = [FORMULA[n] for n in unsat], [proof_of_cdcl(res[n]) for n in unsat]
    for n, c, t in zip(unsat, check_refutations(fs, ps), trim_refutations(fs, ps)):
        assert c["proven"] and c["failed"] == 0, n
        assert t["proven"], n


@pytest.mark.parametrize("holes", [5, 6])
def test_pigeonhole_proofs_are_proven(holes):
    """The proof is PROVEN, forwards and by the trim.  (Soundness alone here; PHP(6) word for word
    against the rule, past its 256th conflict, is the row `php 6` of
    tests/test_cdcl_sound_paths_gpu.py.)"""
    f = R.php(holes)
    r = cdcl_sound.cdcl_sound_batch([f])[0]
    assert r["sat"] is False and r["counters"]["learned"] > holes
    assert check_refutations([f], [proof_of_cdcl(r)])[0]["proven"]
    assert trim_refutations([f], [proof_of_cdcl(r)])[0]["proven"]


def test_a_proof_without_a_needed_lemma_is_not_proven():
    """QUAD + [-1] is not refuted by unit propagation alone, and its proof is one learned unit
    clause and the empty clause: the trim marks both needed, and without the first the empty
    clause does not follow."""
    name = "quad needs learning"
    f, proof = FORMULA[name], proof_of_cdcl(got("all")[name])
    t = trim_refutations([f], [proof])[0]
    assert t["proven"] and t["kept"] == [0, 1] and len(proof) == 2
    dropped = [c for j, c in enumerate(proof) if j != t["kept"][0]]
    assert not check_refutations([f], [dropped])[0]["proven"]
    # and a larger proof, every needed lemma in turn: none of the results may be PROVEN unless the
    # rest still is a proof, which the plain-Python evaluator decides
    f, proof = FORMULA["php 3"], proof_of_cdcl(got("all")["php 3"])
    t = trim_refutations([f], [proof])[0]
    cuts = [[c for j, c in enumerate(proof) if j != k] for k in t["kept"][:-1]]
    checked = check_refutations([f] * len(cuts), cuts)
    for cut, c in zip(cuts, checked):
        assert c["proven"] == (rr.evaluate(f, cut)[0][0] == rr.PROVEN)
    # (by the evaluator no cut of this proof, of a needed lemma or another, is a proof)
    assert cuts and not any(c["proven"] for c in checked)


def test_a_proof_fails_against_a_satisfiable_weakening():
    for name in ("php 3", "php 4", "sparse ids", "quad needs learning"):
        f, proof = FORMULA[name], proof_of_cdcl(got("all")[name])
        weak = next(f[:i] + f[i + 1:] for i in range(len(f)) if R.brute_force(f[:i] + f[i + 1:])) \
            if name != "php 4" else f[1:]        # php without a pigeon's clause: the others fit
        assert check_refutations([weak], [proof])[0]["status"] != _capi.REFUTE_PROVEN, name


def test_conflict_limit_gives_limit():
    f = FORMULA["php 4"]
    w = R.solve(f, conflict_limit=3)
    r = cdcl_sound.cdcl_sound_batch([f, FORMULA["php 3"]], conflict_limit=3)
    assert r[0]["status"] == _capi.CDCL_SOUND_LIMIT == w["status"] and r[0]["sat"] is None
    assert [r[0]["counters"][k] for k in R.COUNTERS] == w["counters"]
    assert r[0]["proof"] is None and r[0]["records"] == 2
    assert r[1]["status"] == R.solve(FORMULA["php 3"], conflict_limit=3)["status"]


def test_time_limit_gives_limit_and_solver_timeout():
    """A limit of ten ticks of the 100 MHz device clock has passed by the first decision: an
    instance that needs one ends LIMIT with no verdict, one that unit propagation settles
    is answered, and nothing waits.  cdcl_sound_solve turns LIMIT into SolverTimeout."""
    f = R.php(6)
    r = cdcl_sound.cdcl_sound_batch([f, [[1], [-1]], [[1], [-1, 2]]], time_limit=1e-7)
    assert r[0]["status"] == _capi.CDCL_SOUND_LIMIT and r[0]["sat"] is None and r[0]["proof"] is None
    assert r[0]["counters"]["decisions"] == 0 and r[0]["counters"]["learned"] == 0
    assert r[1]["sat"] is False and r[2]["sat"] is True and r[2]["model"] == [1, 2]
    solvers.set_time_limit(1e-7)
    try:
        with pytest.raises(solvers.SolverTimeout):
            solvers.cdcl_sound_solve(f)
        assert solvers.cdcl_sound_solve([[1], [-1, 2]]) == (True, {1: True, 2: True}, None)
    finally:
        solvers.set_time_limit(0)
    assert solvers.cdcl_sound_solve(R.php(3))[0] is False


def test_a_small_first_room_runs_again_to_the_same_answer():
    names = ["php 4", "empty formula", "php 3", "random 3-SAT 0", "random 3-SAT 1"]
    cdcl_sound.debug_room(8)
    try:
        res = cdcl_sound.cdcl_sound_batch([FORMULA[n] for n in names])
    finally:
        cdcl_sound.debug_room(0)
    assert R.region_words(want("php 4")["lemmas"]) > 8 * 4     # more than one run-again
    for n, r in zip(names, res):
        _same(n, r, want(n))


def test_a_room_cap_below_the_need_gives_full_beside_untouched_neighbours():
    names = ["php 3", "php 4", "quad needs learning"]
    need = R.region_words(want("php 4")["lemmas"])
    small = max(R.region_words(want(n)["lemmas"]) for n in ("php 3", "quad needs learning"))
    cap = 64
    assert small <= cap < need
    res = cdcl_sound.cdcl_sound_batch([FORMULA[n] for n in names], room_cap=cap)
    assert res[1]["status"] == _capi.CDCL_SOUND_FULL and res[1]["sat"] is None and res[1]["proof"] is None
    assert res[1]["region_words"] > cap
    _same(names[0], res[0], want(names[0]))
    _same(names[2], res[2], want(names[2]))


class Pipeline:
    """satmi_cdcl_sound_batch_device -> pack -> check -> trim on one stream, on torch tensors.
    Every second formula is empty: it ends SAT at once and writes nothing, so its region is a
    run of guard words behind the region before it."""
    GUARD, NG = 0x5A5A5A5A, 8

    def __init__(self, formulas, rooms, ccap, lcap, grid=0):
        import torch
        dev = torch.device("cuda", 0)
        fs = []
        for f in formulas:
            fs += [f, []]
        batch = pack(fs)
        self.B = B = batch.num_instances
        nv = int(batch.inst_nvars.max(initial=0))
        mlen = max([len(c) for f in fs for c in f] + [0])
        lb = np.zeros(B + 1, dtype=np.int64)
        for b in range(B):
            lb[b + 1] = lb[b] + (rooms[b // 2] if b % 2 == 0 else self.NG)
        self.lb = lb

        def up(a, dt=np.int32):
            return torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)

        def zeros(n, dt=torch.int32):
            return torch.zeros(max(n, 1), dtype=dt, device=dev)

        t = [up(batch.inst_clause_begin), up(batch.clause_lit_begin), up(batch.lits)]
        d_nv, d_lb = up(batch.inst_nvars), up(lb, np.int64)
        self.lemmas = torch.full((int(lb[-1]) + self.NG,), self.GUARD, dtype=torch.int32, device=dev)
        self.status, self.counters = zeros(B), zeros(B * 8, torch.int64)
        self.row_len, self.row_lits = zeros(B), zeros(B * max(nv, 1))
        self.info, self.totals = zeros(B * 4, torch.int64), zeros(2, torch.int64)
        self.pib = zeros(B + 1)
        self.pcb = torch.full((ccap + 1 + self.NG,), self.GUARD, dtype=torch.int32, device=dev)
        self.plits = torch.full((lcap + self.NG,), self.GUARD, dtype=torch.int32, device=dev)
        self.out, self.tout = zeros(B * 4), zeros(B * 6)
        self.core, self.lemma = zeros(len(batch.clause_lit_begin)), zeros(ccap)
        s = torch.cuda.current_stream(dev).cuda_stream
        ptr = [x.data_ptr() for x in t]
        self.long_form = not 1 <= mlen <= R.SHORT_MAX
        cdcl_sound.debug_grid(grid, 1 if grid else 0)
        try:
            cdcl_sound.cdcl_sound_device(B, *ptr, d_nv.data_ptr(), nv, mlen, self.lemmas.data_ptr(),
                                         d_lb.data_ptr(), self.status.data_ptr(), self.counters.data_ptr(),
                                         self.row_len.data_ptr(), self.row_lits.data_ptr(), max(nv, 1),
                                         self.info.data_ptr(), stream=s)
        finally:
            cdcl_sound.debug_grid(0, 0)
        cdcl_sound.pack_device(B, self.status.data_ptr(), self.lemmas.data_ptr(), d_lb.data_ptr(),
                               self.info.data_ptr(), self.pib.data_ptr(), self.pcb.data_ptr(), ccap,
                               self.plits.data_ptr(), lcap, self.totals.data_ptr(), stream=s)
        # (longest clause of formulas and lemmas: unknown)
        check_refutations_device(B, *ptr, self.pib.data_ptr(), self.pcb.data_ptr(), self.plits.data_ptr(), nv, 0,
                                 self.out.data_ptr(), None, s)
        trim_refutations_device(B, *ptr, self.pib.data_ptr(), self.pcb.data_ptr(), self.plits.data_ptr(), nv, 0,
                                self.tout.data_ptr(), self.core.data_ptr(), self.lemma.data_ptr(), s)
        torch.cuda.current_stream(dev).synchronize()
        for k in ("lemmas", "status", "counters", "row_len", "row_lits", "info", "totals", "pib", "pcb", "plits",
                  "out", "tout"):
            setattr(self, k, getattr(self, k).cpu().numpy())
        self.info, self.row_lits = self.info.reshape(B, 4), self.row_lits.reshape(B, max(nv, 1))
        self.out, self.tout = self.out.reshape(B, 4), self.tout.reshape(B, 6)

    def region(self, i):
        """(the words of formula i's region, the guard words behind it)."""
        b = 2 * i
        return self.lemmas[self.lb[b]:self.lb[b + 1]], self.lemmas[self.lb[b + 1]:self.lb[b + 1] + self.NG]

    def proof(self, i):
        lo, hi = self.pib[2 * i], self.pib[2 * i + 1]
        return [self.plits[self.pcb[p]:self.pcb[p + 1]].tolist() for p in range(lo, hi)]


def _records(lemmas):
    out = []
    for c in lemmas:
        out += [len(c)] + list(c)
    return out


@pytest.mark.parametrize("group,grid", [("all", 0), ("short", 0), ("short", 1)])
def test_device_form_regions_are_the_python_rules_lemmas(group, grid):
    """Every row through the device form, each region exactly as large as the rule says it must
    be: the region of a SAT row that learned, which the host form never hands out, holds the
    rule's lemmas in order like that of an UNSAT row, in the wave-per-clause form ("all"), the
    lane-per-clause form ("short") and with one wave taking every formula in turn (grid 1 x 1).
    Status, counters and the model row are compared here too, and the guard words behind every
    region."""
    names = GROUPS[group]
    ws = [want(n) for n in names]
    total = sum(len(w["lemmas"]) for w in ws if w["status"] == R.UNSAT)
    lits = sum(len(c) for w in ws if w["status"] == R.UNSAT for c in w["lemmas"])
    p = Pipeline([FORMULA[n] for n in names], [R.region_words(w["lemmas"]) for w in ws], total, lits, grid)
    assert p.long_form == (group == "all")
    assert sum(1 for w in ws if w["status"] == R.SAT and w["lemmas"]) >= 8
    for i, (n, w) in enumerate(zip(names, ws)):
        region, guard = p.region(i)
        assert p.status[2 * i] == w["status"], n
        assert p.counters.reshape(-1, 8)[2 * i].tolist() == w["counters"], n
        assert region.tolist() == _records(w["lemmas"]), n
        assert (guard == Pipeline.GUARD).all(), n
        assert p.info[2 * i].tolist()[:3] == [len(w["lemmas"]), R.region_words(w["lemmas"]), 0], n
        model = p.row_lits[2 * i, :p.row_len[2 * i]].tolist()
        assert model == (w["model"] or []), n
        if w["status"] == R.UNSAT:
            assert p.proof(i) == w["lemmas"] and p.out[2 * i, 0] == p.tout[2 * i, 0] == _capi.REFUTE_PROVEN, n
        else:
            assert p.proof(i) == [] and p.out[2 * i, 0] == _capi.REFUTE_OPEN, n
    assert p.totals.tolist() == [total, lits]


def test_device_pipeline_on_one_stream_and_nothing_past_a_region():
    names = ["php 3", "php 4", "quad needs learning", "random 3-SAT 0", "learned clause of 65", "opposite units"]
    ws = [want(n) for n in names]
    rooms = [R.region_words(w["lemmas"]) for w in ws]       # exactly what each needs ...
    rooms[1] = 40                                           # ... but php 4: FULL
    assert rooms[1] < R.region_words(ws[1]["lemmas"])
    total = sum(len(w["lemmas"]) for i, w in enumerate(ws) if w["status"] == R.UNSAT and i != 1)
    lits = sum(len(c) for i, w in enumerate(ws) if w["status"] == R.UNSAT and i != 1 for c in w["lemmas"])
    p = Pipeline([FORMULA[n] for n in names], rooms, total, max(lits, 1))
    assert p.totals.tolist() == [total, lits]
    for i, (n, w) in enumerate(zip(names, ws)):
        region, guard = p.region(i)
        assert (guard == Pipeline.GUARD).all(), n
        assert p.status[2 * i + 1] == _capi.CDCL_SOUND_SAT and p.row_len[2 * i + 1] == 0
        if i == 1:
            # the records that fit, whole, and the first that does not counted and unwritten
            fit, used = [], 0
            for c in w["lemmas"]:
                if used + 1 + len(c) > rooms[1]:
                    break
                fit.append(c)
                used += 1 + len(c)
            nxt = w["lemmas"][len(fit)]
            assert p.status[2] == _capi.CDCL_SOUND_FULL
            assert region[:used].tolist() == _records(fit) and (region[used:] == Pipeline.GUARD).all()
            assert p.info[2].tolist()[:3] == [len(fit) + 1, used + 1 + len(nxt), _capi.CDCL_SOUND_TRUNCATED]
            assert p.proof(i) == [] and p.out[2, 0] == _capi.REFUTE_OPEN
            continue
        assert p.status[2 * i] == w["status"], n
        assert p.counters.reshape(-1, 8)[2 * i].tolist() == w["counters"], n
        assert region.tolist() == _records(w["lemmas"]), n         # SAT rows too: the clause database
        if w["status"] == R.UNSAT:
            assert p.proof(i) == w["lemmas"], n
            assert p.out[2 * i].tolist() == [_capi.REFUTE_PROVEN, 0, -1, 0], n
            assert p.tout[2 * i, 0] == _capi.REFUTE_PROVEN, n
        else:
            assert p.proof(i) == [] and p.out[2 * i, 0] == _capi.REFUTE_OPEN, n
    assert (p.pcb[total + 1:] == Pipeline.GUARD).all() and (p.plits[lits:] == Pipeline.GUARD).all()


def test_proof_arrays_one_short_report_the_totals_and_stay_unwritten():
    names = ["php 3", "quad needs learning"]
    ws = [want(n) for n in names]
    total = sum(len(w["lemmas"]) for w in ws)
    lits = sum(len(c) for w in ws for c in w["lemmas"])
    p = Pipeline([FORMULA[n] for n in names], [R.region_words(w["lemmas"]) for w in ws], total, lits - 1)
    assert p.totals.tolist() == [total, lits] and (p.pib == 0).all()
    assert (p.plits == Pipeline.GUARD).all() and (p.pcb[1:] == Pipeline.GUARD).all()
    assert (p.out[:, 0] == _capi.REFUTE_OPEN).all()


def test_past_the_variable_limit_the_call_is_refused_before_any_launch():
    with pytest.raises(_capi.SatmiError, match=r"\(-3\).*8192 is beyond the layout's 8191"):
        cdcl_sound.cdcl_sound_batch([[[1, -8192]]])
    assert cdcl_sound.lds_bytes(_capi.CDCL_SOUND_MAX_VARS) <= 160 * 1024 and cdcl_sound.lds_bytes(8192) == 0
    assert cdcl_sound.cdcl_sound_batch([R.sparse_row()])[0]["sat"] is False


@pytest.fixture
def no_pysat(monkeypatch):
    """`import pysat` fails, whether or not python-sat is installed."""
    for k in [k for k in sys.modules if k == "pysat" or k.startswith("pysat.")]:
        monkeypatch.delitem(sys.modules, k)
    monkeypatch.setitem(sys.modules, "pysat", None)


def _large(seed):
    random.seed(seed)
    return solvers.generate_large_formula(1200, 3, 150)


def _answers(f, models):
    if models:
        assert len(models) == 1 and sorted(models[0]) == list(range(1, max(abs(l) for c in f for l in c) + 1))
        assert solvers.check_assignment(f, models[0])
        return True
    sat, model, proof = solvers.cdcl_sound_solve(f)
    assert not sat and model is None and solvers.check_refutation(f, proof)
    return False


def test_pysat_solver_answers_without_pysat(no_pysat):
    seen = {_answers(f, solvers.pysat_solver(f)) for f in (_large(1), _large(2), [[1, 3], [-1]], rr.QUAD + [[-1]])}
    assert seen == {True, False}
    assert solvers.pysat_solver([[1, 3], [-1]]) == [{1: False, 2: False, 3: True}]


def test_hybrid_solver_above_its_threshold_answers_without_pysat(no_pysat):
    f = _large(3)
    assert len(f) > 1000
    _answers(f, solvers.hybrid_solver(f))
    small = [[1, 2], [-1]] * 3
    assert _answers(small, solvers.hybrid_solver(small, threshold=5))
