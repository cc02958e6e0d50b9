"""GPU checks of the batched model check (csrc/check.hip) through the C ABI: every
word of every row against the plain Python evaluator of tests/check_rows.py
(held to brute force by tests/test_check.py).  Outputs are allocated with guard
words on both sides, and the guards are asserted intact."""
import ctypes
import json
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import check_rows as cr
from satmi import _capi, cnf
from satmi.cdcl import CDCL_SAT, cdcl_batch_packed
from satmi.check import check_device, check_models, check_packed, debug_grid
from satmi.dpll import dpll_batch
from satmi.solvers import check_assignment

pytestmark = pytest.mark.gpu

GUARD = 0x5A5A5A5A
NG = 16   # guard words on each side


def _p(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))


def _row_arrays(rows_of, cap=None, stride=None):
    B = len(rows_of)
    cap = cap or max([len(r) for r in rows_of] + [1])
    stride = stride or max([len(x) for r in rows_of for x in r] + [1])
    rows = np.array([len(r) for r in rows_of], dtype=np.int32)
    lens = np.zeros((B, cap), dtype=np.int32)
    lits = np.zeros((B, cap, stride), dtype=np.int32)
    for b, r in enumerate(rows_of):
        for k, x in enumerate(r):
            lens[b, k] = len(x)
            lits[b, k, :len(x)] = x
    return rows, lens, lits, cap, stride


def run_host(formulas, rows_of, cap=None, stride=None):
    """satmi_check_models_host into a guarded output -> the words as [B][cap][4] lists."""
    batch = cnf.pack(formulas)
    rows, lens, lits, cap, stride = _row_arrays(rows_of, cap, stride)
    B = len(formulas)
    buf = np.full(2 * NG + B * cap * 4, GUARD, dtype=np.uint32).view(np.int32)
    out = buf[NG:NG + B * cap * 4]
    rc = _capi.load().satmi_check_models_host(B, _p(batch.inst_clause_begin), _p(batch.clause_lit_begin),
                                              _p(batch.lits), _p(rows), _p(lens), _p(lits), cap, stride, _p(out))
    _capi.check(rc, "satmi_check_models_host")
    g = buf.view(np.uint32)
    assert (g[:NG] == GUARD).all() and (g[-NG:] == GUARD).all()
    return out.reshape(B, cap, 4).tolist()


def run_device(formulas, rows_of, max_vars, max_clause_len, cap=None, stride=None, with_rows=True):
    """satmi_check_models_device on torch tensors, guarded output -> [B][cap][4] lists."""
    import torch
    dev = torch.device("cuda", 0)
    batch = cnf.pack(formulas)
    rows, lens, lits, cap, stride = _row_arrays(rows_of, cap, stride)
    B = len(formulas)
    t = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in
         (batch.inst_clause_begin, batch.clause_lit_begin, batch.lits, rows, lens, lits)]
    buf = torch.full((2 * NG + B * cap * 4,), GUARD, dtype=torch.int32, device=dev)
    s = torch.cuda.current_stream(dev)
    check_device(B, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), max_vars, max_clause_len,
                 t[3].data_ptr() if with_rows else None, t[4].data_ptr(), t[5].data_ptr(), cap, stride,
                 buf.data_ptr() + 4 * NG, s.cuda_stream)
    s.synchronize()
    h = buf.cpu().numpy()
    assert (h[:NG] == GUARD).all() and (h[-NG:] == GUARD).all()
    return h[NG:-NG].reshape(B, cap, 4).tolist()


def _true_max_len(formulas):
    return max([len(c) for f in formulas for c in f] + [0])


# ------------------------------------------------------------------ 1. edge rows in one batch
def test_edge_rows_in_one_batch():
    fs = [f for f, _ in cr.EDGE_CASES]
    rows_of = [[r] for _, r in cr.EDGE_CASES]
    # the host form computes max_vars over formulas and rows (9 here): no literal is beyond it
    got = run_host(fs, rows_of)
    assert got == cr.expected(fs, rows_of, 1)
    assert [g[0][3] for g in got[-5:]] == [1, 2, 2, 0, 1]
    # the device form at the formulas' own max_vars: 9 is beyond the table, flags 2
    for mcl in (_true_max_len(fs), 0):
        got = run_device(fs, rows_of, cr.EDGE_MAX_VARS, mcl)
        assert got == cr.expected(fs, rows_of, 1, cr.EDGE_MAX_VARS), mcl
        assert [g[0][3] for g in got[-5:]] == [1, 2, 2, 2, 3]
    res = check_models(fs, rows_of)
    assert [[r["falsified"], r["undetermined"], r["first_falsified"], r["flags"]] for r in res[4]] == [[1, 0, 2, 0]]
    assert [r[0]["ok"] for r in res[:8]] == [True, True, False, False, False, False, False, True]
    assert check_assignment([[1, -2], [2, 3]], {1: True, 2: False, 3: True})
    assert not check_assignment([[1, -2], [2, 3]], {1: True, 2: False})       # [2, 3] undetermined
    assert not check_assignment([[1, -2], [2, 3]], [-1, 2, 3])                # [1, -2] falsified


# ------------------------------------------------------------------ 2. the reference's own non-models
def test_reference_non_models(golden_dir):
    with open(os.path.join(golden_dir, "dpll_ref.json")) as fh:
        cases = json.load(fh)["cases"]
    fs = [c["formula"] for c in cases]
    cap = max(len(c["solutions"]) for c in cases) + 1
    r = dpll_batch(fs, mode="ref", max_solutions=0, sol_cap=cap, inits=[c["init"] for c in cases], time_limit=20.0)
    got = r.check(fs)
    assert got.shape == (len(fs), cap, 4)
    models = non_models = 0
    for b, c in enumerate(cases):
        sols = r.solutions(b)
        assert sols == c["solutions"]
        want = [cr.evaluate(c["formula"], s) for s in sols]
        assert got[b, :len(sols)].tolist() == want, b
        assert not got[b, len(sols):].any(), b
        models += sum(cr.is_ok(w) for w in want)
        non_models += sum(not cr.is_ok(w) for w in want)
    assert models > 0 and non_models > 0
    assert (models, non_models, models + non_models) == (107, 4973, 5080)


# ------------------------------------------------------------------ 3. sound models (shared with 10)
@pytest.fixture(scope="module")
def sound_mix():
    fs = cr.random_mix()
    batch = cnf.pack(fs)
    r = dpll_batch(batch, mode="sound", max_solutions=1, time_limit=20.0)
    return fs, batch, r


def _rows_of_result(r, lits=None, lens=None):
    lits = r.sol_lits if lits is None else lits
    lens = r.sol_len if lens is None else lens
    return [[lits[b, 0, :lens[b, 0]].tolist()] if r.num_solutions(b) else [] for b in range(lens.shape[0])]


def test_sound_models_and_their_neighbours(sound_mix):
    fs, batch, r = sound_mix
    got = r.check(batch)
    sat = [b for b in range(len(fs)) if r.num_solutions(b)]
    assert 0 < len(sat) < len(fs)
    for b in range(len(fs)):
        assert got[b, 0].tolist() == ([0, 0, -1, 0] if b in sat else [0, 0, 0, 0]), fs[b]
    rows = np.minimum(r.counters[:, 5], 1).astype(np.int32)
    # one literal flipped per row; the last literal dropped
    flipped = r.sol_lits.copy()
    for b in sat:
        if r.sol_len[b, 0]:
            flipped[b, 0, b % r.sol_len[b, 0]] *= -1
    got = check_packed(batch, rows, r.sol_len, flipped)
    assert got.tolist() == cr.expected(fs, _rows_of_result(r, lits=flipped), 1)
    dropped = np.maximum(r.sol_len - 1, 0)
    got = check_packed(batch, rows, dropped, r.sol_lits)
    assert got.tolist() == cr.expected(fs, _rows_of_result(r, lens=dropped), 1)
    assert any(not cr.is_ok(w[0]) for b, w in enumerate(got.tolist()) if b in sat)


# ------------------------------------------------------------------ 4. clause length, both forms
@pytest.mark.parametrize("k", cr.CLAUSE_LENGTHS)
def test_clause_lengths_in_both_forms(k):
    """k = SHORT_MAX is the last length of the lane-per-clause form, SHORT_MAX + 1 the first of
    the wave-per-clause form; max_clause_len = 0 (unknown) takes the latter at every length."""
    f, row = cr.length_case(k)
    fs, rows_of = [f, f[::-1], f], [[row], [row], [row[:-1]]]
    want = cr.expected(fs, rows_of, 1, 3 * k)
    assert want[0] == [[1, 1, 1, 0]] and want[1] == [[1, 1, 1, 0]]
    for mcl in (k, 0):
        assert run_device(fs, rows_of, 3 * k, mcl) == want, mcl
    assert run_host(fs, rows_of) == want


def test_mixed_clause_lengths_in_one_formula():
    """Every length in one formula (the true max_clause_len is 300: the long form), and the
    lengths up to SHORT_MAX in one formula (the short form), their variables renumbered apart."""
    for lengths in (cr.CLAUSE_LENGTHS, tuple(range(1, cr.SHORT_MAX + 1))):
        f, row, base = [], [], 0
        for k in lengths:
            fk, rk = cr.length_case(k)
            f += [[l + base if l > 0 else l - base for l in c] for c in fk]
            row += [l + base if l > 0 else l - base for l in rk]
            base += 3 * k
        want = cr.expected([f], [[row]], 1, base)
        assert want == [[[len(lengths), len(lengths), 1, 0]]]
        for mcl in (max(lengths), 0):
            assert run_device([f], [[row]], base, mcl) == want


# ------------------------------------------------------------------ 5. clause count
def test_clause_counts_and_first_falsified():
    cases = cr.count_cases()
    fs, rows_of = [f for f, _, _ in cases], [[r] for _, r, _ in cases]
    want = [[w] for _, _, w in cases]
    assert cr.expected(fs, rows_of, 1) == want
    assert run_host(fs, rows_of) == want
    for mcl in (2, 0):
        assert run_device(fs, rows_of, 2, mcl) == want, mcl


# ------------------------------------------------------------------ 6. table reuse
def _reuse_batch():
    fs, rows_of = [], []
    for i in range(20):
        for f, rows in (cr.reuse_alternating(8), cr.reuse_disjoint(8)):
            fs.append(f)
            rows_of.append(rows if i % 5 else rows[:5])   # some instances check fewer rows than cap
    return fs, rows_of


@pytest.mark.parametrize("grid", [(0, 0), (1, 1), (1, 2), (1, 4), (3, 2), (3, 4), (0, 1)])
def test_table_reuse_across_rows_instances_and_regions(grid):
    """40 instances of 8 rows; (1, 1): one wave takes them all, so a bit that survived a row
    or an instance shows in the next; 2- and 4-wave workgroups: the regions do not overlap."""
    fs, rows_of = _reuse_batch()
    assert len(fs) == 40
    want = cr.expected(fs, rows_of, 8)
    assert want[1][3] == [1, 14, 6, 0] and want[0][7] == [0, 0, 0, 0] and want[2][7] == [2, 0, 0, 0]
    try:
        debug_grid(*grid)
        assert run_host(fs, rows_of) == want
        for mcl in (2, 0):
            assert run_device(fs, rows_of, 16, mcl) == want, mcl
    finally:
        debug_grid(0, 0)


def test_null_rows_checks_every_slot():
    fs, rows_of = _reuse_batch()
    full = [(r + r)[:8] for r in rows_of]   # d_rows = NULL: all cap rows are rows
    _, lens, _, _, _ = _row_arrays(full)
    assert (lens > 0).all()
    assert run_device(fs, full, 16, 2, with_rows=False) == cr.expected(fs, full, 8)


# ------------------------------------------------------------------ 7. variable range
def test_variable_range():
    top = cr.MAX_VARS
    f = [[1, top], [-top], [-1, top]]
    rows = [[1, -top], [-1, top], [-1], [1, top, -top]]
    want = cr.expected([f], [rows], 4)
    assert want == [[[1, 0, 2, 0], [1, 0, 1, 0], [0, 2, -1, 0], [0, 0, -1, 1]]]
    assert run_host([f], [rows]) == want
    for mcl in (2, 0):
        assert run_device([f, f], [rows, rows[::-1]], top, mcl) == cr.expected([f, f], [rows, rows[::-1]], 4, top)
    g = [[1, top + 1]]
    with pytest.raises(_capi.SatmiError, match=r"\(-3\)"):
        check_models([g], [[[1]]])
    with pytest.raises(_capi.SatmiError, match=r"\(-3\)"):
        run_device([f], [rows], top + 1, 2)
    # sparse ids
    f = [[70000, -3], [-70000], [3, 69999]]
    rows = [[70000, 3], [-70000, -3]]
    want = cr.expected([f], [rows], 2)
    assert want == [[[1, 0, 1, 0], [0, 1, -1, 0]]]
    assert run_host([f], [rows]) == want


# ------------------------------------------------------------------ 8. device form on the solver's outputs
def test_device_form_on_the_solvers_own_outputs():
    import torch
    dev = torch.device("cuda", 0)
    L = _capi.load()
    B, n, m, k = 2048, 100, 426, 3
    icb, clb, lits, nv = cnf.uniform_ksat_device(B, n, m, k, 77, dev)
    status = torch.zeros(B, dtype=torch.int32, device=dev)
    counters = torch.zeros((B, _capi.NCOUNTERS), dtype=torch.int64, device=dev)
    sol_len = torch.zeros(B, dtype=torch.int32, device=dev)
    sol_lits = torch.zeros((B, n), dtype=torch.int32, device=dev)
    buf = torch.full((2 * NG + B * 4,), GUARD, dtype=torch.int32, device=dev)
    s = torch.cuda.Stream(dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        rc = L.satmi_dpll_batch_device(B, icb.data_ptr(), clb.data_ptr(), lits.data_ptr(), nv.data_ptr(), n, m, m * k,
                                       k, None, None, _capi.MODE_SOUND, 1, 0, 20.0, 1, n, status.data_ptr(),
                                       counters.data_ptr(), sol_len.data_ptr(), sol_lits.data_ptr(), None, None,
                                       s.cuda_stream)
        _capi.check(rc, "satmi_dpll_batch_device")
        # no synchronisation: the check reads the solver's outputs in stream order
        check_device(B, icb.data_ptr(), clb.data_ptr(), lits.data_ptr(), n, k, None, sol_len.data_ptr(),
                     sol_lits.data_ptr(), 1, n, buf.data_ptr() + 4 * NG, s.cuda_stream)
    s.synchronize()
    h = buf.cpu().numpy()
    assert (h[:NG] == GUARD).all() and (h[-NG:] == GUARD).all()
    got = h[NG:-NG].reshape(B, 4)
    st, nsol = status.cpu().numpy(), counters[:, 5].cpu().numpy()
    assert ((st == _capi.DPLL_EXHAUSTED) | (st == _capi.DPLL_STOPPED)).all()
    sat = nsol > 0
    assert 0 < sat.sum() < B
    assert (got[sat] == np.array([0, 0, -1, 0])).all()
    hl, hlen = lits.cpu().numpy().reshape(B, m, k), sol_len.cpu().numpy()
    hs = sol_lits.cpu().numpy()
    for b in range(0, B, B // 64):
        assert got[b].tolist() == cr.evaluate(hl[b].tolist(), hs[b, :hlen[b]].tolist(), n), b


# ------------------------------------------------------------------ 9. CDCL
def test_cdcl_assignments(golden_dir):
    """The reference decides whether its CDCL's SAT answers are models; here the check's words
    equal the evaluator's on them, whatever they are."""
    with open(os.path.join(golden_dir, "cdcl_ref.json")) as fh:
        cases = [c for c in json.load(fh)["cases"] if c["result"] == 1]
    assert len(cases) > 50
    by_cap = {}
    for c in cases:
        by_cap.setdefault(c["max_iter"], []).append(c)
    for max_iter, cs in by_cap.items():
        fs = [c["formula"] for c in cs]
        batch = cnf.pack(fs)
        a = cdcl_batch_packed(batch, max_iter=max_iter, arrays=True)
        assert (a["status"] == CDCL_SAT).all()
        got = check_packed(batch, None, a["assign_len"], a["assign"])   # the layout with cap = 1, as it is
        rows_of = [[a["assign"][b, :a["assign_len"][b]].tolist()] for b in range(len(fs))]
        assert [r[0] for r in rows_of] == [c["assignment"] for c in cs]
        assert got.tolist() == cr.expected(fs, rows_of, 1)


# ------------------------------------------------------------------ 10. four host threads
def test_four_host_threads(sound_mix):
    fs, batch, r = sound_mix
    whole = r.check(batch)
    cuts = [0, 60, 150, 220, 300]
    rows = np.minimum(r.counters[:, 5], 1).astype(np.int32)

    def part(t):
        a, b = cuts[t], cuts[t + 1]
        return check_packed(cnf.pack(fs[a:b]), rows[a:b], r.sol_len[a:b], r.sol_lits[a:b])

    with ThreadPoolExecutor(4) as ex:
        for _ in range(3):
            parts = list(ex.map(part, range(4)))
            assert (np.concatenate(parts) == whole).all()
