"""GPU checks of the sound CDCL under assumptions (csrc/cdcl_sound.hip's assumption-carrying
kernels) at the rows of tests/cdcl_assume_rows.py: the kernel is the Python rule exactly --
status, counters, model row, core and the region's lemma list -- in both clause forms and on a
one-wave grid; without assumptions it is the existing entry point word for word; its three
answers pass the library's own checkers, in the host form and in the device pipeline
solve -> pack -> check on one stream."""
import functools

import numpy as np
import pytest

import cdcl_assume_rows as A
import cdcl_sound_rows as R
from satmi import _capi, cdcl_sound, solvers
from satmi.check import check_models
from satmi.cnf import pack
from satmi.refute import check_refutations, check_refutations_device, proof_of_cdcl_assumed, trim_refutations

pytestmark = pytest.mark.gpu

ROWS = A.rows()
FORMULA = {n: f for n, f, _ in ROWS}
ASSUME = {n: a for n, _, a in ROWS}
NAMES = [n for n, _, _ in ROWS]
SHORT = [n for n in NAMES if max([len(c) for c in FORMULA[n]] + [0]) <= R.SHORT_MAX and n != "sparse ids"]
GROUPS = {"all": NAMES, "short": SHORT}     # "all" holds 300-literal clauses: the wave-per-clause form
REFUTED = (A.UNSAT, A.ASSUMED)


def _units(lits):
    return [[l] for l in lits]


@functools.lru_cache(maxsize=None)
def want(name):
    return A.solve(FORMULA[name], ASSUME[name])


@functools.lru_cache(maxsize=None)
def got(group, grid=0):
    """The host form on the group's rows in one call: name -> cdcl_assume_batch dict."""
    names = GROUPS[group]
    cdcl_sound.debug_grid(grid, 1 if grid else 0)
    try:
        res = cdcl_sound.cdcl_assume_batch([FORMULA[n] for n in names], [ASSUME[n] for n in names])
    finally:
        cdcl_sound.debug_grid(0, 0)
    return dict(zip(names, res))


def _same(name, g, w):
    assert g["status"] == w["status"], name
    assert [g["counters"][k] for k in A.COUNTERS] == w["counters"], name
    assert g["model"] == w["model"], name
    assert g["core"] == (w["core"] if w["status"] in REFUTED else None), name
    assert g["core_len"] == len(w["core"] or []), name
    if w["status"] in REFUTED:
        assert g["proof"] == w["lemmas"], name
    assert g["records"] == len(w["lemmas"]) and g["region_words"] == R.region_words(w["lemmas"]), name


def test_rows_reach_every_answer_on_the_cpu():
    random_rows = [want(n)["status"] for n in NAMES if n.endswith("assumed")]
    assert len(random_rows) == A.RANDOM_COUNT
    assert all(random_rows.count(s) >= 4 for s in (A.SAT, A.UNSAT, A.ASSUMED))
    assert want("php 3 under six selectors")["status"] == A.ASSUMED
    assert sorted(want("php 3 under six selectors")["core"]) == A.SELECTORS
    assert len(GROUPS["short"]) > 140 and "long clause" not in GROUPS["short"]
    assert "chain of 64" not in GROUPS["short"] and "chain of 2" in GROUPS["short"]


@pytest.mark.parametrize("group,grid", [("all", 0), ("short", 0), ("short", 1)])
def test_kernel_is_the_python_rule(group, grid):
    """Every row, in the wave-per-clause form ("all"), the lane-per-clause form ("short"), and
    with one wave taking every formula of the batch in turn (grid 1 x 1)."""
    res = got(group, grid)
    for name in GROUPS[group]:
        _same(name, res[name], want(name))


def test_without_assumptions_every_output_is_the_existing_entry_points():
    """The rows of cdcl_sound_rows with k = 0 everywhere, through both host forms: status,
    counters, model rows, info words and the proof arrays, word for word."""
    batch = pack([f for _, f in R.rows()])
    old = cdcl_sound.cdcl_sound_packed(batch)
    begin, lits, _ = cdcl_sound.pack_assumptions(None, batch.num_instances)
    new = cdcl_sound.cdcl_assume_packed(batch, begin, lits)
    for o, n in zip(old[:4] + (old[5],), new[:4] + (new[5],)):
        assert np.array_equal(o, n)
    for k in ("inst_clause_begin", "clause_lit_begin", "lits"):
        assert np.array_equal(getattr(old[4], k), getattr(new[4], k)), k
    assert not new[6].any() and not new[7].any()
    assert (old[0] == _capi.CDCL_SOUND_UNSAT).sum() >= 8 and (old[0] == _capi.CDCL_SOUND_SAT).sum() >= 8


@pytest.mark.parametrize("n", [1, 2, 64, 65])
def test_core_stride_sufficient_and_one_short(n):
    f, a = A.chain_row(n)
    full, short = (cdcl_sound.cdcl_assume_batch([f, [[1]]], [a, [-1]], core_stride=s)[0] for s in (n, n - 1))
    assert full["status"] == short["status"] == _capi.CDCL_SOUND_ASSUMED
    assert full["core"] == list(range(n, 0, -1)) and full["core_len"] == n
    assert short["core"] == list(range(n, 1, -1)) and short["core_len"] == n      # the count, and what fits
    with pytest.raises(ValueError, match="core_stride"):
        proof_of_cdcl_assumed(f, short)


def test_every_answer_is_certified_by_the_librarys_checkers():
    res = got("all")
    assumed = [n for n in NAMES if res[n]["status"] == _capi.CDCL_SOUND_ASSUMED]
    sat = [n for n in NAMES if res[n]["sat"]]
    assert len(assumed) >= 12 and len(sat) >= 12
    pairs = [proof_of_cdcl_assumed(FORMULA[n], res[n]) for n in assumed]
    fs, ps = [p[0] for p in pairs], [p[1] for p in pairs]
    for n, c, t in zip(assumed, check_refutations(fs, ps), trim_refutations(fs, ps)):
        assert c["proven"] and c["failed"] == 0, n
        assert t["proven"], n
    # against F alone the same proof does not stand where F is satisfiable: the core is needed
    alone = [n for n in assumed if res[n]["core"] and A.solve(FORMULA[n])["status"] == A.SAT]
    assert alone
    unproven = [not c["proven"] for c in check_refutations([FORMULA[n] for n in alone], [res[n]["proof"] for n in alone])]
    assert any(unproven) and unproven[alone.index("unit against its assumption")]
    # the PHP selector row needs every selector: without any one of them, not PROVEN
    name = "php 3 under six selectors"
    core, proof = res[name]["core"], res[name]["proof"]
    assert sorted(core) == A.SELECTORS
    cuts = [FORMULA[name] + _units(core[:i] + core[i + 1:]) for i in range(len(core))]
    assert not any(c["proven"] for c in check_refutations(cuts, [proof] * len(cuts)))
    # SAT rows: the model satisfies the formula and the assumptions
    models = check_models([FORMULA[n] + _units(ASSUME[n]) for n in sat], [[res[n]["model"]] for n in sat])
    for n, c in zip(sat, models):
        assert c[0]["ok"], n


class Pipeline:
    """satmi_cdcl_assume_batch_device -> satmi_cdcl_assume_pack_device -> refutation check on one
    stream, on torch tensors.  Every region is exactly as large as the rule says it must be and
    guard words lie behind the last one, behind every core's count and behind the core array."""
    GUARD, NG = 0x5A5A5A5A, 8

    def __init__(self, names, core_stride, old_pack=False):
        import torch
        dev = torch.device("cuda", 0)
        ws = [want(n) for n in names]
        batch = pack([FORMULA[n] for n in names])
        begin, alits, top = cdcl_sound.pack_assumptions([ASSUME[n] for n in names], len(names))
        self.B = B = batch.num_instances
        nvars = np.maximum(batch.inst_nvars, top).astype(np.int32)
        nv = int(nvars.max(initial=0))
        mlen = max([len(c) for n in names for c in FORMULA[n]] + [0])
        self.lb = lb = np.zeros(B + 1, dtype=np.int64)
        np.cumsum([R.region_words(w["lemmas"]) for w in ws], out=lb[1:])
        refuted = [w for w in ws if w["status"] in (REFUTED[:1] if old_pack else REFUTED)]
        self.ccap = ccap = max(sum(len(w["lemmas"]) for w in refuted), 1)
        self.lcap = lcap = max(sum(len(c) for w in refuted for c in w["lemmas"]), 1)

        def up(a, dt=np.int32):
            return torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)

        def zeros(n, dt=torch.int32):
            return torch.zeros(max(n, 1), dtype=dt, device=dev)

        def guarded(n):
            return torch.full((n + self.NG,), self.GUARD, dtype=torch.int32, device=dev)

        t = [up(batch.inst_clause_begin), up(batch.clause_lit_begin), up(batch.lits)]
        d_nv, d_lb, d_ab, d_al = up(nvars), up(lb, np.int64), up(begin), up(alits)
        self.lemmas = guarded(int(lb[-1]))
        self.status, self.counters = zeros(B), zeros(B * 8, torch.int64)
        self.row_len, self.row_lits = zeros(B), zeros(B * max(nv, 1))
        self.core_len, self.core_lits = zeros(B), guarded(B * core_stride)
        self.info, self.totals = zeros(B * 4, torch.int64), zeros(2, torch.int64)
        self.pib, self.pcb, self.plits = zeros(B + 1), guarded(ccap + 1), guarded(lcap)
        self.out = zeros(B * 4)
        s = torch.cuda.current_stream(dev).cuda_stream
        ptr = [x.data_ptr() for x in t]
        cdcl_sound.cdcl_assume_device(B, *ptr, d_nv.data_ptr(), nv, mlen, self.lemmas.data_ptr(), d_lb.data_ptr(),
                                      self.status.data_ptr(), self.counters.data_ptr(), self.row_len.data_ptr(),
                                      self.row_lits.data_ptr(), max(nv, 1), self.info.data_ptr(), d_ab.data_ptr(),
                                      d_al.data_ptr(), self.core_len.data_ptr(), self.core_lits.data_ptr(),
                                      core_stride, stream=s)
        (cdcl_sound.pack_device if old_pack else cdcl_sound.assume_pack_device)(
            B, self.status.data_ptr(), self.lemmas.data_ptr(), d_lb.data_ptr(), self.info.data_ptr(),
            self.pib.data_ptr(), self.pcb.data_ptr(), ccap, self.plits.data_ptr(), lcap, self.totals.data_ptr(),
            stream=s)
        check_refutations_device(B, *ptr, self.pib.data_ptr(), self.pcb.data_ptr(), self.plits.data_ptr(), nv, 0,
                                 self.out.data_ptr(), None, s)
        torch.cuda.current_stream(dev).synchronize()
        for k in ("lemmas", "status", "counters", "row_len", "row_lits", "core_len", "core_lits", "info", "totals",
                  "pib", "pcb", "plits", "out"):
            setattr(self, k, getattr(self, k).cpu().numpy())
        self.info, self.out = self.info.reshape(B, 4), self.out.reshape(B, 4)
        self.core_guard = self.core_lits[B * core_stride:]
        self.core_lits = self.core_lits[:B * core_stride].reshape(B, core_stride)

    def proof(self, b):
        return [self.plits[self.pcb[p]:self.pcb[p + 1]].tolist() for p in range(self.pib[b], self.pib[b + 1])]


def _records(lemmas):
    out = []
    for c in lemmas:
        out += [len(c)] + list(c)
    return out


PIPE = ["php 3 under six selectors", "php 3", "empty levels and a new variable", "chain of 65",
        "random 3-SAT 3 assumed", "unit against its assumption", "php 3 under five selectors"]


def test_device_pipeline_on_one_stream_and_nothing_past_a_buffer():
    stride = 8       # holds the six selectors; the chain's 65 are cut
    p = Pipeline(PIPE, stride)
    ws = [want(n) for n in PIPE]
    assert {w["status"] for w in ws} >= {A.SAT, A.UNSAT, A.ASSUMED}
    assert (p.lemmas[p.lb[-1]:] == Pipeline.GUARD).all() and (p.core_guard == Pipeline.GUARD).all()
    assert (p.pcb[p.ccap + 1:] == Pipeline.GUARD).all() and (p.plits[p.lcap:] == Pipeline.GUARD).all()
    assert p.totals.tolist() == [p.ccap, p.lcap]
    for b, (n, w) in enumerate(zip(PIPE, ws)):
        assert p.status[b] == w["status"], n
        assert p.counters.reshape(-1, 8)[b].tolist() == w["counters"], n
        assert p.lemmas[p.lb[b]:p.lb[b + 1]].tolist() == _records(w["lemmas"]), n     # SAT rows too
        assert p.info[b].tolist()[:3] == [len(w["lemmas"]), R.region_words(w["lemmas"]), 0], n
        core = w["core"] or []
        assert p.core_len[b] == len(core), n
        k = min(len(core), stride)
        assert p.core_lits[b, :k].tolist() == core[:k] and (p.core_lits[b, k:] == Pipeline.GUARD).all(), n
        if w["status"] == A.UNSAT:       # the refutation of F alone, checked where the pack left it
            assert p.proof(b) == w["lemmas"] and p.out[b].tolist() == [_capi.REFUTE_PROVEN, 0, -1, 0], n
        elif w["status"] == A.ASSUMED:   # its lemmas are there; against F alone the empty clause does not follow
            assert p.proof(b) == w["lemmas"], n
            if A.solve(FORMULA[n])["status"] == A.SAT:
                assert p.out[b].tolist() == [_capi.REFUTE_FAILED, 1, len(w["lemmas"]) - 1, 0], n
        else:
            assert p.proof(b) == [] and p.out[b, 0] == _capi.REFUTE_OPEN, n


def test_the_existing_pack_gives_assumed_instances_no_lemma():
    p = Pipeline(PIPE, 8, old_pack=True)
    for b, n in enumerate(PIPE):
        w = want(n)
        assert p.status[b] == w["status"], n
        assert p.proof(b) == (w["lemmas"] if w["status"] == A.UNSAT else []), n
    assert p.totals.tolist() == [p.ccap, p.lcap]


def test_conflict_limit_under_three_assumptions_gives_limit():
    f, a = R.php(4), [1, 6, 11]
    w = A.solve(f, a, conflict_limit=1)
    r = cdcl_sound.cdcl_assume_batch([f, [[1, 2]]], [a, [-1]], conflict_limit=1)
    assert r[0]["status"] == _capi.CDCL_SOUND_LIMIT == w["status"] and r[0]["sat"] is None
    assert [r[0]["counters"][k] for k in A.COUNTERS] == w["counters"] and w["counters"][6] == 3
    assert r[0]["proof"] is None and r[0]["core"] is None and r[0]["core_len"] == 0
    assert r[1]["model"] == [-1, 2]


def test_more_assumptions_than_the_limit_is_too_large_beside_an_untouched_neighbour():
    many = [1] * (_capi.CDCL_SOUND_MAX_VARS + 1)
    r = cdcl_sound.cdcl_assume_batch([[[1]], [[1]], [[1]]], [many, many[:-1], [-1]])
    assert r[0]["status"] == _capi.CDCL_SOUND_TOO_LARGE and r[0]["sat"] is None and r[0]["records"] == 0
    assert r[0]["counters"]["rounds"] == 0 and r[0]["core_len"] == 0
    assert r[1]["status"] == _capi.CDCL_SOUND_SAT and r[1]["counters"]["max_level"] == _capi.CDCL_SOUND_MAX_VARS
    assert r[2]["core"] == [-1]


def test_a_small_first_room_runs_again_to_the_same_answer():
    names = ["php 3 under six selectors", "unit against its assumption", "php 3", "random 3-SAT 3 assumed"]
    assert R.region_words(want(names[0])["lemmas"]) > 4 and want(names[0])["status"] == A.ASSUMED
    cdcl_sound.debug_room(2)
    try:
        res = cdcl_sound.cdcl_assume_batch([FORMULA[n] for n in names], [ASSUME[n] for n in names])
    finally:
        cdcl_sound.debug_room(0)
    for n, r in zip(names, res):
        _same(n, r, want(n))


def test_solvers_entry_point():
    f, a = A.php_selector_row()
    assert solvers.cdcl_sound_solve(R.php(3))[:2] == (False, None) and len(solvers.cdcl_sound_solve(R.php(3))) == 3
    assert solvers.cdcl_sound_solve([[1], [-1, 2]]) == (True, {1: True, 2: True}, None)
    sat, model, proof, core = solvers.cdcl_sound_solve(f, a)
    assert (sat, model) == (False, None) and sorted(core) == A.SELECTORS and proof == want("php 3 under six selectors")["lemmas"]
    assert solvers.check_refutation(f + _units(core), proof) and not solvers.check_refutation(f, proof)
    sat, model, proof, core = solvers.cdcl_sound_solve([[1, 2]], [1, 1, 5])
    assert (sat, model, proof, core) == (True, {1: True, 2: False, 5: True}, None, None)
    assert solvers.cdcl_sound_solve([[1], [-1]], [2]) == (False, None, [[]], [])     # refuted at level 0: of F alone
    # (PHP(3) under one assumption learns its negation first and ends on it: a core of one, by the rule)
    sat, _, proof, core = solvers.cdcl_sound_solve(R.php(3), [2])
    assert not sat and core == [2] and solvers.check_refutation(R.php(3) + [[2]], proof)
