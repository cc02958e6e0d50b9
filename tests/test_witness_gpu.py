"""GPU checks of the witness kernel (csrc/witness.hip) through the C ABI: every word
and every row literal of every instance against the plain Python rule of
tests/witness_rows.py (held to brute force by tests/test_witness.py).  Outputs are
allocated with guard words on both sides, and the guards are asserted intact.  The
host form is run, and the device form at the true max_clause_len (the lane-per-clause
form up to 8) and at 0 (the wave-per-clause form)."""
import ctypes
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import dp_batch_rows
import res_batch_rows
import witness_rows as wr
from satmi import _capi
from satmi.check import check_models
from satmi.dp import eliminate, eliminate_batch
from satmi.resolution import resolve, resolve_batch
from satmi.solvers import (davis_putnam_witness, davis_putnam_witness_batch, resolution_witness,
                           resolution_witness_batch)
from satmi.witness import (debug_grid, record_of, stages_of_elimination, stages_of_resolution, witness_models,
                           witness_models_device)

pytestmark = pytest.mark.gpu

GUARD = 0x5A5A5A5A
NG = 16   # guard words on each side
FINE = [wr.MODEL, 0, -1, 0, 0, -1]


def _p(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))


def _i32(a):
    return np.array(a or [0], dtype=np.int64).astype(np.int32)


def _csr(lists):
    """Lists of clause lists -> (inst_begin, clause_begin, lits) int32, any literal kept as it is."""
    icb, clb, lits = [0], [0], []
    for f in lists:
        for c in f:
            lits += c
            clb.append(len(lits))
        icb.append(len(clb) - 1)
    return tuple(_i32(a) for a in (icb, clb, lits))


def _stages(stages):
    isb = [0]
    for s in stages:
        isb.append(isb[-1] + len(s))
    return (_i32(isb),) + tuple(_i32([t[k] for s in stages for t in s]) for k in range(3))


def _guarded(n):
    buf = np.full(2 * NG + n, GUARD, dtype=np.uint32).view(np.int32)
    return buf, buf[NG:NG + n]


def _intact(buf):
    g = np.asarray(buf).view(np.uint32)
    return (g[:NG] == GUARD).all() and (g[-NG:] == GUARD).all()


def _stride_of(formulas):
    return max([len({abs(l) for c in f for l in c}) for f in formulas] + [1])


def _cut(B, words, lens, rows, stride):
    return (words.reshape(B, wr.NWORDS).tolist(), lens.tolist(),
            [rows[b * stride:b * stride + min(int(lens[b]), stride)].tolist() for b in range(B)])


def run_host(formulas, records, stages, ho, stride):
    """satmi_witness_models_host into guarded outputs -> ([B][6] words, [B] lengths, [B] rows)."""
    B = len(formulas)
    obuf, out = _guarded(B * wr.NWORDS)
    lbuf, lens = _guarded(B)
    rbuf, rows = _guarded(B * stride)
    rc = _capi.load().satmi_witness_models_host(B, *map(_p, _csr(formulas) + _csr(records) + _stages(stages)),
                                                int(ho), _p(out), _p(lens), _p(rows), stride)
    _capi.check(rc, "satmi_witness_models_host")
    assert _intact(obuf) and _intact(lbuf) and _intact(rbuf)
    return _cut(B, out, lens, rows, stride)


def run_device(formulas, records, stages, ho, max_vars, max_clause_len, stride):
    """satmi_witness_models_device on torch tensors, guarded outputs; what the row arrays hold
    behind a row's length (or its stride) is the caller's: asserted untouched."""
    import torch
    dev = torch.device("cuda", 0)
    B = len(formulas)
    t = [torch.from_numpy(a).to(dev) for a in _csr(formulas) + _csr(records) + _stages(stages)]
    bufs = [torch.full((2 * NG + n,), GUARD, dtype=torch.int32, device=dev) for n in (B * wr.NWORDS, B, B * stride)]
    s = torch.cuda.current_stream(dev)
    witness_models_device(B, *(x.data_ptr() for x in t), ho, max_vars, max_clause_len,
                          *(x.data_ptr() + 4 * NG for x in bufs), stride, s.cuda_stream)
    s.synchronize()
    ho_, hl, hr = (x.cpu().numpy() for x in bufs)
    assert _intact(ho_) and _intact(hl) and _intact(hr)
    lens, rows = hl[NG:-NG], hr[NG:-NG]
    for b in range(B):
        assert (rows[b * stride + min(int(lens[b]), stride):(b + 1) * stride].view(np.uint32) == GUARD).all()
    return _cut(B, ho_[NG:-NG], lens, rows, stride)


def _true_max_len(formulas, records):
    return max([len(c) for f in formulas + records for c in f] + [0])


def check_all(formulas, records, stages, ho=False, stride=None, host=True, max_vars=None):
    """Host form and both device forms against the rule; returns what the rule says."""
    stride = stride or _stride_of(formulas)
    mv = max_vars if max_vars is not None else max([wr.max_vars_of(f, r) for f, r in zip(formulas, records)] + [0])
    want = wr.expected(formulas, records, stages, ho, mv, stride)
    if host:
        assert run_host(formulas, records, stages, ho, stride) == want
    for mcl in (_true_max_len(formulas, records), 0):
        assert run_device(formulas, records, stages, ho, mv, mcl, stride) == want, mcl
    return want


def _cases(cases):
    return [c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases]


# ------------------------------------------------------------------ 1. the edge batch
def test_edge_batch_in_one_launch():
    """Stuck, highest_only on and off, a tautologous clause, a variable decided twice, vanishing
    variables, a range straddling m, empty and repeated ranges, the unsound True."""
    for ho in (False, True):
        cases = [c for c in wr.EDGE_CASES if c[3] == ho]
        words, lens, rows = check_all(*_cases(cases), ho)
        assert words == [c[4] for c in cases] and rows == [c[5] for c in cases] and lens == [len(c[5]) for c in cases]
    f, r, st, ho, words, row = wr.STUCK
    assert words == [0, 1, 0, 0, 1, 1]
    res = witness_models([f], [r], [st], ho)[0]
    assert [res[k] for k in _capi.WITNESS_WORDS] == words and res["model"] == row and not res["ok"]
    # [[1, 2]] with stages for 1 then 2: not forced under the flag, forced without it
    assert witness_models([[[1, 2]]] * 2, [[]] * 2, [[(1, 0, 1), (2, 0, 1)]] * 2, True)[0]["model"] == [-1, 2]
    assert witness_models([[[1, 2]]], [[]], [[(1, 0, 1), (2, 0, 1)]], False)[0]["model"] == [1, -2]


# ------------------------------------------------------------------ 2. stage sizes
@pytest.mark.parametrize("n", sorted({n for n, _ in wr.STAGE_SIZES}))
def test_stage_sizes_with_the_forcing_clause_at_every_edge(n):
    cases = [wr.stage_size_case(n, at) for m, at in wr.STAGE_SIZES if m == n]
    words, _, rows = check_all(*_cases(cases))
    assert words == [FINE] * len(cases) and rows == [[1, -2]] * len(cases)


# ------------------------------------------------------------------ 3. clause lengths, both forms
@pytest.mark.parametrize("k", wr.CLAUSE_LENGTHS)
def test_clause_lengths_with_the_decisive_literal_last(k):
    """k = 8 is the last length of the lane-per-clause form, 9 the first of the wave-per-clause
    form; max_clause_len = 0 (unknown) takes the latter at every length."""
    f, r, st, ho = wr.length_case(k)
    words, _, rows = check_all([f], [r], [st], ho)
    assert words == [FINE] and rows[0][:2] == ([1, -2] if k > 1 else [1])


def test_mixed_clause_lengths_in_one_instance():
    for lengths in (wr.CLAUSE_LENGTHS, tuple(range(1, wr.SHORT_MAX + 1))):
        f, st, base = [], [], 0
        for k in lengths:
            fk, _, sk, _ = wr.length_case(k, base)
            st += [(x, lo + len(f), hi + len(f)) for x, lo, hi in sk]
            f += fk
            base += k + 1
        words, lens, _ = check_all([f], [[]], [st])
        assert words == [FINE] and lens == [len({abs(l) for c in f for l in c})]


# ------------------------------------------------------------------ 4. variable ids
def test_variable_ids_around_the_table_words():
    cases = [wr.variable_case(v) for v in wr.VARIABLE_IDS]
    words, _, rows = check_all(*_cases(cases))
    assert words == [FINE] * len(cases) and rows == [[v - 1, v, -(v + 1)] for v in wr.VARIABLE_IDS]


def test_sparse_pair_and_the_limit():
    top = wr.MAX_VARS
    f, st = [[-1], [1, top]], [(1, 0, 1), (top, 0, 2)]
    words, _, rows = check_all([f], [[]], [st])
    assert words == [FINE] and rows == [[-1, top]]
    assert check_models([f], [[rows[0]]])[0][0]["ok"]
    with pytest.raises(_capi.SatmiError, match=r"\(-3\)"):
        witness_models([[[1, top + 1]]], [[]], [[]])
    with pytest.raises(_capi.SatmiError, match=r"\(-3\)"):
        run_device([f], [[]], [st], False, top + 1, 2, 2)


# ------------------------------------------------------------------ 5. bad literals, bad stages, truncation
def test_bad_literals_and_stages_through_the_device_form():
    """max_vars = 3 where the arrays hold 9, 0 and INT32_MIN and stages name 0, 4 and -1."""
    fs = [[[1, 9], [-1, 0], [2, wr.I32_MIN]], [[1]], [[1]], [[1, 9]], [[1, wr.I32_MIN]], [[1, 0]]]
    rs = [[], [[7]], [[7]], [], [], []]
    ss = [[(1, 0, 3), (2, 0, 3), (0, 0, 3), (4, 0, 3), (-1, 0, 3)], [(1, 0, 1)], [(1, 0, 2)], [(1, 0, 1)], [(1, 0, 1)],
          [(1, 0, 1)]]
    words, _, rows = check_all(fs, rs, ss, False, host=False, max_vars=3)
    assert words[0] == [wr.NOT_MODEL, 1, 0, wr.BAD_LITERAL | wr.BAD_STAGE, 1, 1] and rows[0] == [1, 2]
    assert [w[3] for w in words[1:3]] == [0, wr.BAD_LITERAL]
    _, _, rows = check_all(fs[3:], rs[3:], ss[3:], True, host=False, max_vars=3)
    assert rows == [[-1], [-1], [1]]           # under highest_only a bad literal is a magnitude
    # ranges beyond the clause lists are clamped by the device form
    check_all([[[1], [2]]], [[[3]]], [[(1, -5, 9), (2, 7, 9), (3, 2, 1)]], host=False)


def test_row_truncation():
    f, st = [[1, 2, 3], [-2, 5]], [(3, 0, 1), (5, 0, 2)]
    words, lens, rows = check_all([f, f], [[], []], [st, []], stride=4)
    assert [w[3] for w in words] == [0, 0] and lens == [4, 4]
    words, lens, rows = check_all([f, f], [[], []], [st, []], stride=3)
    assert [w[3] for w in words] == [wr.ROW_TRUNCATED] * 2 and lens == [4, 4] and rows[0] == [-1, -2, 3]
    assert not witness_models([f], [[]], [st])[0]["flags"]


# ------------------------------------------------------------------ 6. grids and table reuse
@pytest.mark.parametrize("grid", [(1, 1), (1, 2), (1, 4), (3, 2), (3, 4), (0, 0)])
def test_forty_instances_under_every_grid(grid):
    """(1, 1): one wave takes all 40, and a bit that survived an instance would change the next
    one's row; 2- and 4-wave workgroups: the regions do not overlap."""
    fs, rs, ss = wr.forty()
    try:
        debug_grid(*grid)
        words, _, rows = check_all(fs, rs, ss)
        assert words == [FINE] * 40 and all((l > 0) == (i % 2 == 0) for i, row in enumerate(rows) for l in row)
    finally:
        debug_grid(0, 0)


# ------------------------------------------------------------------ 7. the solvers' own records
@pytest.fixture(scope="module")
def records():
    """name -> (formulas, records, stages, highest_only, what the rule says) of the True answers
    of the batched solver and of a few single calls."""
    out = {}
    for name, fs, batch, single, build, ho in (
            ("elimination", dp_batch_rows.EDGE + dp_batch_rows.mix()[:48], eliminate_batch, eliminate,
             stages_of_elimination, False),
            ("resolution", res_batch_rows.EDGE + res_batch_rows.mix()[:48], resolve_batch, resolve,
             stages_of_resolution, True)):
        rs = batch(fs, record=True)
        true = [b for b, r in enumerate(rs) if r["result"] == 1]
        assert 8 < len(true) < len(fs)
        ones = true[-6:]
        for tag, ids, res in ((name + "_batch", true, [rs[b] for b in true]),
                              (name, ones, [single(fs[b], record=True) for b in ones])):
            assert all(r["result"] == 1 for r in res)
            sub = [fs[b] for b in ids]
            recs, sts = [record_of(r) for r in res], [build(f, r) for f, r in zip(sub, res)]
            out[tag] = (sub, recs, sts, ho, wr.expected(sub, recs, sts, ho, None, _stride_of(sub)))
    return out


@pytest.mark.parametrize("name", ["elimination_batch", "elimination", "resolution_batch", "resolution"])
def test_recorded_true_answers_give_models(records, name):
    fs, recs, sts, ho, want = records[name]
    assert check_all(fs, recs, sts, ho) == want
    res = witness_models(fs, recs, sts, ho)
    assert [[r[k] for k in _capi.WITNESS_WORDS] for r in res] == want[0] and [r["model"] for r in res] == want[2]
    sound = [[] not in f for f in fs]
    assert [r["ok"] for r in res] == sound and sum(sound) >= 4
    assert all(r["stuck"] == 0 for r, s in zip(res, sound) if s)
    checked = check_models(fs, [[r["model"]] for r in res])
    assert [c[0]["ok"] for c in checked] == sound


def test_solver_entry_points(records):
    fs = [f for f in records["resolution_batch"][0] if f and [] not in f][:6] + [[[1, 2], [-1, 2], [1, -2], [-1, -2]]]
    for one, many in ((davis_putnam_witness, davis_putnam_witness_batch),
                      (resolution_witness, resolution_witness_batch)):
        got = many(fs)
        assert [g[0] for g in got] == [True] * (len(fs) - 1) + [False] and got[-1] == (False, None)
        for f, (_, model) in zip(fs[:-1], got):
            assert sorted(model) == sorted({abs(l) for c in f for l in c})
            assert check_models([f], [[model]])[0][0]["ok"]
        assert one(fs[0]) == got[0] and one(fs[-1]) == (False, None)


# ------------------------------------------------------------------ 8. the reference's unsound True
def test_the_references_unsound_true_is_refused():
    f = [[1], []]
    for one, many in ((davis_putnam_witness, davis_putnam_witness_batch),
                      (resolution_witness, resolution_witness_batch)):
        with pytest.raises(_capi.SatmiError, match="falsifies 1 of its clauses"):
            one(f)
        with pytest.raises(_capi.SatmiError, match="formula 1"):
            many([[[1]], f])
    for solve, build, ho in ((eliminate, stages_of_elimination, False), (resolve, stages_of_resolution, True)):
        r = solve(f, record=True)
        assert r["result"] == 1
        w = witness_models([f], [record_of(r)], [build(f, r)], ho)[0]
        assert (w["status"], w["falsified"], w["first_falsified"], w["ok"]) == (wr.NOT_MODEL, 1, 1, False)


# ------------------------------------------------------------------ 9. four host threads
def test_four_host_threads(records):
    fs, recs, sts, ho, _ = records["elimination_batch"]
    n = len(fs)
    cuts = [0, n // 5, n // 2, n - 3, n]
    stride = _stride_of(fs)

    def part(t):
        a, b = cuts[t], cuts[t + 1]
        return run_host(fs[a:b], recs[a:b], sts[a:b], ho, stride)

    want = [wr.expected(fs[a:b], recs[a:b], sts[a:b], ho, None, stride) for a, b in zip(cuts, cuts[1:])]
    with ThreadPoolExecutor(4) as ex:
        for _ in range(3):
            assert list(ex.map(part, range(4))) == want
