"""GPU parity of batched resolution saturation (csrc/resolution_batch.hip: one
workgroup per formula, saturated in LDS) against the CPU oracle and the
single-call path: verdicts, per-pass counts and the exact clause set of every
pass; workgroup reuse, the capacity (UNFIT) contract, the limits, the record's
truncation and concurrent calls."""
import ctypes
import threading

import numpy as np
import pytest

import oracle
import res_batch_rows
from satmi import _capi, cnf
from satmi import resolution as res_mod
from satmi.resolution import debug_batch, resolve, resolve_batch

pytestmark = pytest.mark.gpu

GUARD = 8
G32, G64 = 0x5A5A5A5A, 0x5A5A5A5A5A5A5A5A
UNFIT = -2


def _sets(passes):
    return [sorted(p) for p in passes]


def _same(r, o, what=None):
    assert (r["result"], r["passes"], list(r["pass_new"])) == (o["result"], o["passes"], list(o["pass_new"])), what
    if "clauses" in r and "clauses" in o:
        assert _sets(r["clauses"]) == _sets(o["clauses"]), what


@pytest.fixture(scope="module")
def mix():
    """The 200 formulas of tests/res_batch_rows.py (drawn as
    test_resolution_gpu.py::test_matches_oracle_random draws its 60), their
    oracle results and one recorded batch run of them all."""
    fs = res_batch_rows.mix()
    want = [oracle.resolution(f, record=True) for f in fs]
    got = resolve_batch(fs, record=True)
    return fs, want, got


@pytest.fixture(scope="module")
def bench_set():
    return cnf.uniform_ksat(16, 7, 49, 3, seed=7001)


def test_edge_cases_in_one_batch():
    fs = res_batch_rows.EDGE
    got = resolve_batch(fs)
    assert [r["result"] for r in got[:7]] == [1, 1, 1, 0, 1, 0, 1]
    for f, r in zip(fs, got):
        assert r["path"] == "batch", f
        _same(r, oracle.resolution(f), f)
        _same(r, resolve(f), f)


def test_random_mix_matches_oracle(mix):
    fs, want, got = mix
    assert len(got) == 200
    assert {o["result"] for o in want} == {0, 1}       # both verdicts occur
    for f, o, r in zip(fs, want, got):
        assert r["path"] == "batch", f
        _same(r, o, f)


def test_workgroup_reuse(mix):
    """Two workgroups take all 200 formulas, large and small ones alternating:
    whatever a formula leaves in LDS (table, counters, stop word -- an UNSAT
    one leaves its stop word set, a large one a full table) must not reach the
    next one."""
    fs, want, got = mix
    by_size = sorted(range(200), key=lambda b: len(fs[b]) + sum(want[b]["pass_new"]))
    order = [by_size[-1 - k // 2] if k % 2 == 0 else by_size[k // 2] for k in range(200)]
    assert sorted(order) == list(range(200))
    debug_batch(2, 0)
    try:
        again = resolve_batch([fs[b] for b in order], record=True)
    finally:
        debug_batch(0, 0)
    for k, b in enumerate(order):
        assert again[k] == got[b], (k, b, fs[b])


def _want_limited(f, lim):
    """The oracle's saturation of f as clause_limit=lim ends it: after the first
    pass that brings the clause count over lim (the oracle's own clause_limit
    stops in the middle of that pass, so max_passes is the comparison)."""
    o = oracle.resolution(f, record=True)
    over = [p for p, n in enumerate(len(f) + np.cumsum(o["pass_new"])) if n > lim]
    if not over:
        return o
    o = oracle.resolution(f, max_passes=over[0] + 1, record=True)
    assert o["result"] == -1 and o["passes"] == over[0] + 1
    return o


def test_sparse_ids(mix):
    """Variable ids above 63 take the host encoder's sorted path: every third of
    the first 40 formulas renamed v -> 1000 v (both paths in one batch), a
    formula over {1, 70, INT32_MAX}, a chain of 31 sparse variables (still one
    key: the batch path, stopped by clause_limit) and one of 32 (handed back)."""
    fs, _, _ = mix
    big = 2 ** 31 - 1
    rows = [[[1000 * l for l in c] for c in f] if b % 3 == 0 else f for b, f in enumerate(fs[:40])]
    rows.append([[1, -70], [70, big], [-big, -1], [1, 70, big], [-70, -big]])
    rows.append([[i, -(i + 1)] for i in range(100, 130)])      # ids 100 .. 130: 31 variables
    rows.append([[i, -(i + 1)] for i in range(100, 131)])      # ids 100 .. 131: 32
    assert [len({abs(l) for c in f for l in c}) for f in rows[-3:]] == [3, 31, 32]
    want = [_want_limited(f, 64) for f in rows]
    assert all(o["result"] in (0, 1) for o in want[:41]) and [o["result"] for o in want[41:]] == [-1, -1]
    got = resolve_batch(rows, clause_limit=64, record=True)
    assert [r["path"] for r in got] == ["batch"] * 42 + ["single"]
    for f, r, o in zip(rows, got, want):
        _same(r, o, f)


def _c_call(formulas, pass_cap, rec_lit_cap=None, rec_clause_cap=None, max_passes=0):
    """satmi_resolution_batch_host with guard words after every output array."""
    L = _capi.load()
    cb = cnf.pack(formulas)
    B = cb.num_instances
    P32, P64 = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int64)
    out = {"res": np.full(B + GUARD, G32, np.int32), "passes": np.full(B + GUARD, G32, np.int32),
           "pn": np.full(B * pass_cap + GUARD, G64, np.int64)}
    sizes = {"res": B, "passes": B, "pn": B * pass_cap}
    record = rec_lit_cap is not None
    if record:
        out.update(rl=np.full(rec_lit_cap + GUARD, G32, np.int32), rco=np.full(rec_clause_cap + GUARD, G64, np.int64),
                   rpo=np.full(B * (pass_cap + 1) + GUARD, G64, np.int64))
        sizes.update(rl=rec_lit_cap, rco=rec_clause_cap, rpo=B * (pass_cap + 1))
    p = {k: v.ctypes.data_as(P32 if v.dtype == np.int32 else P64) for k, v in out.items()}
    rc = L.satmi_resolution_batch_host(B, cb.inst_clause_begin.ctypes.data_as(P32),
                                       cb.clause_lit_begin.ctypes.data_as(P32), cb.lits.ctypes.data_as(P32),
                                       max_passes, 0, p["res"], p["passes"], p["pn"], pass_cap,
                                       p.get("rl"), rec_lit_cap or 0, p.get("rco"), rec_clause_cap or 0, p.get("rpo"))
    _capi.check(rc, "satmi_resolution_batch_host")
    for k, v in out.items():   # nothing written past an array's capacity
        assert (v[sizes[k]:] == (G32 if v.dtype == np.int32 else G64)).all(), k
    r = {k: v[:sizes[k]] for k, v in out.items()}
    r["pn"] = r["pn"].reshape(B, pass_cap)
    if record:
        r["rpo"] = r["rpo"].reshape(B, pass_cap + 1)
    return r


def _recorded(r, b, p):
    rpo, rco, rl = r["rpo"], r["rco"], r["rl"]
    return [rl[rco[c]:rco[c + 1]].tolist() for c in range(rpo[b, p], rpo[b, p + 1])]


def test_capacity_and_fallback():
    fit = [[[1, 2], [-1, 2], [1, -2], [-1, -2]], [[1, 2, 3], [-1, 2], [-2, 3]], [[1, -2], [2, -3], [3]]]
    chain32 = [[i, -(i + 1)] for i in range(1, 32)]     # 32 variables: not a packed key
    grows = [[i, -(i + 1)] for i in range(1, 13)]       # 13 variables, saturates at 78 clauses
    fs = [fit[0], chain32, fit[1], grows, fit[2]]
    want = [oracle.resolution(f, record=True) for f in fs]
    assert len({abs(l) for c in chain32 for l in c}) == 32
    assert want[3]["result"] == 1 and len(grows) + sum(want[3]["pass_new"]) > 64
    for b in (0, 2, 4):   # no order of claims can take a fit formula to 64 keys: 3^d + m < 64
        assert 3 ** len({abs(l) for c in fs[b] for l in c}) + len(fs[b]) < 64
        assert len(fs[b]) + sum(want[b]["pass_new"]) < 64
    debug_batch(0, 64)
    try:
        r = _c_call(fs, 16, rec_lit_cap=4096, rec_clause_cap=4096)
        via = resolve_batch(fs, record=True)
    finally:
        debug_batch(0, 0)
    assert [int(x) if x == UNFIT else "ok" for x in r["res"]] == ["ok", UNFIT, "ok", UNFIT, "ok"]
    for b in (1, 3):
        assert r["passes"][b] == 0 and not r["pn"][b].any()
        assert (r["rpo"][b] == r["rpo"][b, 0]).all()      # nothing recorded
    for b in (0, 2, 4):
        o = want[b]
        n = o["passes"]
        assert (int(r["res"][b]), int(r["passes"][b])) == (o["result"], n)
        assert r["pn"][b, :n].tolist() == o["pass_new"] and not r["pn"][b, n:].any()
        assert [_recorded(r, b, p) for p in range(n)] == _sets(o["clauses"])
    assert [x["path"] for x in via] == ["batch", "single", "batch", "single", "batch"]
    for f, x, o in zip(fs, via, want):
        _same(x, o, f)


def test_bench_set(bench_set):
    fs = [bench_set.instance(b) for b in range(16)]
    got = resolve_batch(bench_set, record=True)
    assert [r["path"] for r in got] == ["batch"] * 16     # none is UNFIT at the default capacity
    for b, f in enumerate(fs):
        s = resolve(f)
        assert (got[b]["result"], got[b]["passes"], got[b]["pass_new"]) == (s["result"], s["passes"], s["pass_new"]), b
    for b in (0, 1):
        _same(got[b], oracle.resolution(fs[b], record=True), b)
    assert resolve_batch(fs) == [{k: v for k, v in r.items() if k != "clauses"} for r in got]


def test_limits():
    batch = cnf.uniform_ksat(4, 8, 20, 3, seed=3)
    fs = [batch.instance(b) for b in range(4)]
    for mp in (1, 2):
        got = resolve_batch(batch, max_passes=mp)
        for f, r in zip(fs, got):
            o = oracle.resolution(f, max_passes=mp)
            _same(r, o, (mp, f))
            if len(f) + sum(o["pass_new"]) <= 4096:
                assert r["path"] == "batch", (mp, f)
    # clause_limit at and beside the sizes the clause list has after passes 1..3
    limits = set()
    for f in fs:
        cum = len(f) + np.cumsum(resolve(f, max_passes=3)["pass_new"])
        limits.update(int(c) + d for c in cum for d in (-1, 0, 1))
    stopped_in_batch = 0
    for lim in sorted(limits):
        got = resolve_batch(batch, clause_limit=lim)
        for f, r in zip(fs, got):
            s = resolve(f, clause_limit=lim)
            _same(r, s, (lim, f))
            if s["result"] != 0 and len(f) + sum(s["pass_new"]) <= 4096:
                assert r["path"] == "batch", (lim, f)
                stopped_in_batch += s["result"] == -1
    assert stopped_in_batch > 0


def test_record_truncation(bench_set):
    f = bench_set.instance(0)
    full = _c_call([f], 16, rec_lit_cap=1 << 16, rec_clause_cap=1 << 14)
    n = int(full["passes"][0])
    assert n >= 2
    whole = [_recorded(full, 0, p) for p in range(n)]
    assert [len(p) for p in whole] == full["pn"][0, :n].tolist()      # nothing truncated
    assert all(p == sorted(p) for p in whole)
    lits1 = sum(len(c) for c in whole[0])
    lits2 = sum(len(c) for c in whole[1])
    for lit_cap, clause_cap in ((lits1 + lits2 // 2, 1 << 14),                   # literals run out in pass 2
                                (1 << 16, len(whole[0]) + len(whole[1]) // 2)):  # clause offsets do
        t = _c_call([f], 16, rec_lit_cap=lit_cap, rec_clause_cap=clause_cap)
        assert (t["res"][0], t["passes"][0]) == (full["res"][0], full["passes"][0])
        assert (t["pn"] == full["pn"]).all()
        got = [_recorded(t, 0, p) for p in range(n)]
        assert got[0] == whole[0] and 0 < len(got[1]) < len(whole[1])
        for p in range(n):   # a sorted prefix of the pass
            assert got[p] == whole[p][:len(got[p])], p


def test_two_threads(mix):
    fs, want, got = mix
    out = [None, None]

    def run(k):
        out[k] = resolve_batch(fs[100 * k:100 * (k + 1)], record=True)

    th = [threading.Thread(target=run, args=(k,)) for k in (0, 1)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert out[0] + out[1] == got


def test_more_passes_than_the_first_call_keeps(mix, monkeypatch):
    """resolve_batch keeps a bounded number of per-pass counts per formula and
    runs a formula with more passes again with room for all: with one count
    kept, every multi-pass formula takes that path."""
    fs, want, got = mix
    monkeypatch.setattr(res_mod, "_PASS_CAP", 1)
    assert max(o["passes"] for o in want[:40]) > 1
    assert resolve_batch(fs[:40], record=True) == got[:40]
