"""GPU checks of the batched refutation trim (csrc/trim.hip) through the C ABI.

Which core the trim finds depends on the propagation order, so the kernel is held
to the properties of tests/trim_rows.py on every row (its PROVEN is re-checked by
the forward check on the GPU and by the plain Python evaluator), and compared
exactly only on the rows whose answer is unique.  Every batch runs in both clause
forms -- the host form and the device form at the true max_clause_len, and the
device form at 0 (wave-per-clause) -- and each form also with one workgroup of 1,
2 and 4 waves: within a form all runs must return identical arrays.  The device
form's outputs are allocated with guard words on both sides and pre-filled with
garbage: the kernel initialises its own ranges."""
import ctypes

import numpy as np
import pytest

import refute_rows as rr
import trim_rows as tr
from satmi import _capi
from satmi.dp import eliminate_batch
from satmi.refute import (check_refutations, proof_of_elimination, proof_of_resolution, trim_debug_grid,
                          trim_refutations, trim_refutations_device)
from satmi.resolution import resolve_batch
from satmi.solvers import check_refutation, trim_refutation

pytestmark = pytest.mark.gpu

GUARD = 0x5A5A5A5A
NG = 16   # guard words on each side
GRIDS = ((0, 0), (1, 1), (1, 2), (1, 4))


def _p(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))


def _csr(lists):
    """Lists of clause lists -> (inst_begin, clause_begin, lits) int32, any literal kept as it is."""
    icb, clb, lits = [0], [0], []
    for f in lists:
        for c in f:
            lits += c
            clb.append(len(lits))
        icb.append(len(clb) - 1)
    return tuple(np.array(a or [0], dtype=np.int64).astype(np.int32) for a in (icb, clb, lits))


def _guarded(n):
    buf = np.full(2 * NG + n, GUARD, dtype=np.uint32).view(np.int32)
    return buf, buf[NG:NG + n]


def _intact(buf):
    g = np.asarray(buf).view(np.uint32)
    return (g[:NG] == GUARD).all() and (g[-NG:] == GUARD).all()


def run_host(formulas, proofs):
    """satmi_trim_refutations_host into guarded outputs -> ([B][6] words, core marks, lemma marks)."""
    B, C, P = len(formulas), sum(map(len, formulas)), sum(map(len, proofs))
    f, p = _csr(formulas), _csr(proofs)
    obuf, out = _guarded(B * tr.NWORDS)
    cbuf, core = _guarded(C)
    lbuf, lemma = _guarded(P)
    rc = _capi.load().satmi_trim_refutations_host(B, *map(_p, f), *map(_p, p), _p(out), _p(core), _p(lemma))
    _capi.check(rc, "satmi_trim_refutations_host")
    assert _intact(obuf) and _intact(cbuf) and _intact(lbuf)
    return out.reshape(B, tr.NWORDS).tolist(), core.tolist(), lemma.tolist()


def run_device(formulas, proofs, max_vars, max_clause_len):
    """satmi_trim_refutations_device on torch tensors; the outputs start as guard words throughout."""
    import torch
    dev = torch.device("cuda", 0)
    B, C, P = len(formulas), sum(map(len, formulas)), sum(map(len, proofs))
    t = [torch.from_numpy(a).to(dev) for a in _csr(formulas) + _csr(proofs)]
    bufs = [torch.full((2 * NG + n,), GUARD, dtype=torch.int32, device=dev) for n in (B * tr.NWORDS, C, P)]
    s = torch.cuda.current_stream(dev)
    trim_refutations_device(B, *(x.data_ptr() for x in t), max_vars, max_clause_len,
                            *(x.data_ptr() + 4 * NG for x in bufs), s.cuda_stream)
    s.synchronize()
    ho, hc, hl = (x.cpu().numpy() for x in bufs)
    assert _intact(ho) and _intact(hc) and _intact(hl)
    return ho[NG:-NG].reshape(B, tr.NWORDS).tolist(), hc[NG:NG + C].tolist(), hl[NG:NG + P].tolist()


def _true_max_len(formulas, proofs):
    return max([len(c) for f in formulas + proofs for c in f] + [0])


def _batch_max_vars(formulas, proofs):
    return max([rr.max_vars_of(f, p) for f, p in zip(formulas, proofs)] + [0])


def trim_both_forms(formulas, proofs, max_vars=None, grids=GRIDS, host=True, brute_nvars=None):
    """Both clause forms under every grid, identical within a form; the properties of every row
    in both forms; every PROVEN re-checked by the forward check on the GPU.  Returns
    {max_clause_len: (words, core, lemma)} for the true max_clause_len and for 0."""
    mv = _batch_max_vars(formulas, proofs) if max_vars is None else max_vars
    got = {}
    try:
        for mcl in (_true_max_len(formulas, proofs), 0):
            runs = []
            for grid in grids:
                trim_debug_grid(*grid)
                runs.append(run_device(formulas, proofs, mv, mcl))
                if host and mcl and grid == (0, 0):
                    runs.append(run_host(formulas, proofs))
            assert all(r == runs[0] for r in runs[1:]), mcl
            got[mcl] = runs[0]
    finally:
        trim_debug_grid(0, 0)
    for mcl, (words, core, lemma) in got.items():
        rows = tr.split(words, core, lemma, formulas, proofs)
        cores, kepts = [], []
        for (f, p), (w, c, le) in zip(zip(formulas, proofs), rows):
            tr.check_properties(f, p, w, c, le, max_vars=mv, brute_nvars=brute_nvars)
            if w[0] == rr.PROVEN:
                cores.append([f[i] for i in range(len(f)) if c[i]])
                kepts.append([p[j] for j in range(len(p)) if le[j] >= 0])
        if cores and max_vars is None:   # (the forward check's host form computes max_vars itself)
            for r in check_refutations(cores, kepts):
                assert r["proven"] and r["failed"] == 0, mcl
    return got


def _marks(rows_out):
    """[(status, core indices, kept indices)] of split rows."""
    return [(w[0], [i for i, x in enumerate(c) if x], [j for j, x in enumerate(le) if x >= 0])
            for w, c, le in rows_out]


# ------------------------------------------------------------------ 1. rows whose answer is unique
def test_rows_with_a_unique_answer():
    rows = tr.unique_rows()
    fs, ps = [r[0] for r in rows], [r[1] for r in rows]
    want = [(r[2], r[3], r[4]) for r in rows]
    for mcl, (words, core, lemma) in trim_both_forms(fs, ps).items():
        assert _marks(tr.split(words, core, lemma, fs, ps)) == want, mcl


def test_forward_failed_trim_proven_example_through_python():
    f, p = tr.XOR2 + [[3, 4]], [[5, 6], [2], []]
    assert not check_refutation(f, p)
    (r,) = trim_refutations([f], [p])
    assert r == dict(status=rr.PROVEN, proven=True, failed=0, first_failed=-1, flags=0, core=[0, 1, 2, 3],
                     kept=[1, 2], proof=[[2], []])
    core, proof = trim_refutation(f, p)
    assert (core, proof) == (tr.XOR2, [[2], []]) and check_refutation(core, proof)
    assert trim_refutation([[1, 2]], [[]]) is None and trim_refutation([[1], [-1]], [[2]]) is None


def test_edge_cases_of_the_forward_check():
    """Every refute_rows.EDGE_CASES row, with and without [] in it: properties."""
    fs, ps = [c[0] for c in rr.EDGE_CASES], [c[1] for c in rr.EDGE_CASES]
    got = trim_both_forms(fs, ps, brute_nvars=4)
    for words, _, _ in got.values():
        assert [w[0] == rr.OPEN for w in words] == [[] not in p for p in ps]


# ------------------------------------------------------------------ 2. random small pairs
def test_random_small_pairs():
    rows = tr.random_rows(seeds=[0], count=150)
    fs, ps = [r[0] for r in rows], [r[1] for r in rows]
    got = trim_both_forms(fs, ps, brute_nvars=5)
    statuses = {w[0] for w in got[0][0]}
    assert statuses == {rr.FAILED, rr.PROVEN, rr.OPEN}


# ------------------------------------------------------------------ 3. counts and lengths
def test_clause_and_lemma_counts():
    rows = tr.counts_rows()
    got = trim_both_forms([r[0] for r in rows], [r[1] for r in rows])
    for words, _, lemma in got.values():
        n = len(rr.CLAUSE_COUNTS)
        assert [w[0] for w in words[1:n]] == [rr.PROVEN] * (n - 1) and words[0][0] == rr.FAILED
        # the chain of unforced implications: every one of them is needed and fails
        assert [w[:3] for w in words[n:]] == [[rr.PROVEN, 0, -1]] + [[rr.FAILED, k - 1, 0] for k in rr.LEMMA_COUNTS[1:]]


@pytest.mark.parametrize("k", rr.CLAUSE_LENGTHS)
def test_clause_lengths_in_both_forms(k):
    """k = 8 is the last length of the lane-per-clause form; 64, 65 and 300 are read and marked
    in one, two and five 64-literal steps."""
    rows = tr.length_rows(k)
    got = trim_both_forms([r[0] for r in rows], [r[1] for r in rows])
    for words, _, _ in got.values():
        assert words[0][0] == rr.PROVEN


# ------------------------------------------------------------------ 4. reuse of a wave's region
def test_forty_instances_through_one_wave():
    """A table bit, a side bit or a reason that survived an instance changes the next one's core
    (tests/trim_rows.py says how); one wave takes all 40 under the (1, 1) grid."""
    rows = tr.reuse_rows()
    assert len(rows) == 40
    fs, ps = [r[0] for r in rows], [r[1] for r in rows]
    want = [(rr.PROVEN, r[2], r[3]) for r in rows]
    for mcl, (words, core, lemma) in trim_both_forms(fs, ps, grids=GRIDS + ((3, 2), (3, 4))).items():
        assert _marks(tr.split(words, core, lemma, fs, ps)) == want, mcl


# ------------------------------------------------------------------ 5. bad literals, tautologies
def test_bad_literals_and_tautologies_through_the_device_form():
    """max_vars = 3 where the arrays hold 9, 0 and INT32_MIN.  A clause that holds one is no
    premise and sets the flag; a lemma that holds one is no premise either, so nothing can mark
    it: it changes nothing, and what would have needed it fails instead.  A tautological lemma
    is never a reason or a conflict, so it is never needed and the flag stays 0 where the forward
    check sets it.  (The kernel treats a needed lemma of either kind as the forward check does;
    only the ending lemma is needed without being marked, and it is empty.)"""
    fs = [[[1], [-1]], [[1, 9], [-1]], [[2, 0], [-2, rr.I32_MIN], [1], [-1]], [[1]], [[-9, 1], [-1]], [[1], [-1]]]
    ps = [[[9], []], [[]], [[]], [[-1, 9], []], [[1], []], [[2, -2], []]]
    want = [([rr.PROVEN, 0, -1, 0, 2, 1], [1, 1], [-1, 1]),
            ([rr.FAILED, 1, 0, 2, 0, 1], [0, 0], [0]),
            ([rr.PROVEN, 0, -1, 2, 2, 1], [0, 0, 1, 1], [1]),
            ([rr.FAILED, 1, 1, 0, 0, 1], [0], [-1, 0]),
            ([rr.FAILED, 1, 0, 2, 1, 2], [0, 1], [0, 1]),
            ([rr.PROVEN, 0, -1, 0, 2, 1], [1, 1], [-1, 1])]
    assert rr.evaluate(fs[5], ps[5], 3)[0][3] == rr.TAUTOLOGY
    for mcl, (words, core, lemma) in trim_both_forms(fs, ps, max_vars=3, host=False).items():
        assert tr.split(words, core, lemma, fs, ps) == [(w, c, le) for w, c, le in want], mcl


# ------------------------------------------------------------------ 6. the solvers' own records
@pytest.mark.parametrize("name", ["resolution", "elimination"])
def test_recorded_proofs_trim(name):
    solve, build = ((resolve_batch, proof_of_resolution) if name == "resolution" else
                    (eliminate_batch, proof_of_elimination))
    fs = rr.random_3sat(16, 7, 49, 4)
    rs = solve(fs, record=True)
    ps = [build(r) for r in rs]
    unsat = [b for b, r in enumerate(rs) if r["result"] == 0]
    assert len(unsat) >= 8
    got = trim_both_forms(fs, ps)
    for words, _, _ in got.values():
        assert all(words[b][0] == rr.PROVEN for b in unsat)
        assert all(words[b][0] == rr.OPEN for b in range(16) if b not in unsat)
    res = trim_refutations(fs, ps)
    trimmed = [([fs[b][c] for c in res[b]["core"]], res[b]["proof"]) for b in unsat]
    assert all(res[b]["proven"] and res[b]["proof"][-1] == [] for b in unsat)
    checked = check_refutations([c for c, _ in trimmed], [p for _, p in trimmed])
    assert all(r["proven"] and r["failed"] == 0 for r in checked)
    assert sum(len(p) for _, p in trimmed) < sum(len(ps[b]) for b in unsat)   # something was trimmed


# ------------------------------------------------------------------ 7. the variable limit
def test_the_variable_limit():
    """Two instances at exactly SATMI_TRIM_MAX_VARS, where a region is 102 KiB and a workgroup
    one wave.  Every variable a unit clause, and [-1, -top] falsified: the trail fills to its
    last entry, and the analysis walks all of it to reach [1], skipping 254 chunks by ballot.  A
    chain of 130 implications at the top of the range, ending in [-top]."""
    top = tr.MAX_VARS
    units = [[v] for v in range(1, top + 1)] + [[-1, -top]]
    lo = top - 130
    chain = [[lo]] + [[-v, v + 1] for v in range(lo, top)] + [[-top]]
    fs, ps = [units, chain], [[[]], [[]]]
    want = [(rr.PROVEN, [0, top - 1, top], [0]), (rr.PROVEN, list(range(len(chain))), [0])]
    for mcl, (words, core, lemma) in trim_both_forms(fs, ps, grids=((0, 0), (1, 1))).items():
        assert _marks(tr.split(words, core, lemma, fs, ps)) == want, mcl
    with pytest.raises(_capi.SatmiError, match=r"\(-3\)"):
        run_device(fs, ps, top + 1, 2)
    try:
        trim_debug_grid(1, 2)   # two regions of 102 KiB do not fit a CU: refused, not launched
        with pytest.raises(_capi.SatmiError, match=r"\(-3\)"):
            run_device(fs, ps, top, 2)
    finally:
        trim_debug_grid(0, 0)


# ------------------------------------------------------------------ 8. the host form's arrays
def test_host_form_null_marks_and_clauses_before_the_first_instance():
    """Either mark pointer may be NULL; clauses and lemmas in front of the first instance's
    ranges belong to no instance and read 0 / -1."""
    f, p = tr.XOR2 + [[3, 4]], [[5, 6], [2], []]
    (icb, clb, lits), (pib, pcb, plits) = _csr([[[7], [8, 9]], f]), _csr([[[7]], p])
    icb, pib = icb[1:].copy(), pib[1:].copy()   # one instance, whose ranges start at clause 2 and lemma 1
    L = _capi.load()
    want_core, want_lemma = [0, 0, 1, 1, 1, 1, 0], [-1, -1, 1, 1]
    for use_core, use_lemma in ((True, True), (True, False), (False, True), (False, False)):
        out = np.full(tr.NWORDS, GUARD, np.int32)
        core, lemma = np.full(7, 77, np.int32), np.full(4, 77, np.int32)
        rc = L.satmi_trim_refutations_host(1, _p(icb), _p(clb), _p(lits), _p(pib), _p(pcb), _p(plits), _p(out),
                                           _p(core) if use_core else None, _p(lemma) if use_lemma else None)
        _capi.check(rc, "satmi_trim_refutations_host")
        assert out.tolist() == [rr.PROVEN, 0, -1, 0, 4, 2]
        assert core.tolist() == (want_core if use_core else [77] * 7)
        assert lemma.tolist() == (want_lemma if use_lemma else [77] * 4)
