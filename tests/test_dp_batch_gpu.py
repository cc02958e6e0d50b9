"""GPU parity of batched Davis-Putnam elimination (csrc/dp_batch.hip: one
workgroup per formula, every step in LDS) against the CPU oracle and the
single-call path: verdict, eliminated variables, steps, the clause count and
(recorded) the exact clause list after every completed step; the slot rule and
its collisions, wave and chunk boundaries, workgroup reuse, the capacity
(UNFIT) contract, the limits, the record's truncation and concurrent calls.
tests/test_dp_batch.py proves on the CPU that every hand-built row below takes
the path it is named for."""
import ctypes
import threading

import numpy as np
import pytest

import dp_batch_rows as R
import oracle
from satmi import _capi, cnf
from satmi.dp import debug_batch, eliminate, eliminate_batch

pytestmark = pytest.mark.gpu

GUARD = 8
G32, G64 = 0x5A5A5A5A, 0x5A5A5A5A5A5A5A5A
UNFIT = -2


def _want(f, **lim):
    """The oracle's elimination in eliminate_batch's shape."""
    o = oracle.dp(f, record=True, **lim)
    n = R.completed(o)
    cl = [[R.lit_order(c) for c in l] for l in o["clauses"][:n]]
    return {"result": o["result"], "vars": o["vars"], "steps": o["steps"], "step_clauses": [len(l) for l in cl],
            "clauses": cl}


def _same(r, w, what=None, path="batch"):
    assert r["path"] == path, what
    for k in ("result", "vars", "steps", "step_clauses"):
        assert r[k] == w[k], (k, what)
    if "clauses" in r:
        assert r["clauses"] == w["clauses"], what


def _same_single(r, f, what=None, **lim):
    s = eliminate(f, **lim)
    assert (r["result"], r["vars"], r["steps"]) == (s["result"], s["vars"], s["steps"]), what


@pytest.fixture(scope="module")
def mix():
    fs = R.mix()
    want = [_want(f) for f in fs]
    got = eliminate_batch(fs, record=True)
    return fs, want, got


def test_edge_cases_in_one_batch():
    got = eliminate_batch(R.EDGE, record=True)
    assert [r["result"] for r in got[:8]] == [1, 1, 1, 0, 1, 0, 1, 0]
    for f, r in zip(R.EDGE, got):
        # ({5, 13} collide in 8 slots: the slot rule hands that one row back)
        _same(r, _want(f), f, path="single" if f == [[5], [-5, 13]] else "batch")
        _same_single(r, f, f)


def test_random_mix_matches_oracle(mix):
    fs, want, got = mix
    assert len(got) == 200
    assert {w["result"] for w in want} == {0, 1}           # both verdicts occur
    for f, w, r in zip(fs, want, got):
        _same(r, w, f)                                     # every one on the batch path
    plain = eliminate_batch(fs)
    assert plain == [{k: v for k, v in r.items() if k != "clauses"} for r in got]


def test_sparse_ids():
    """Variable ids above 63 take the host encoder's sorted path: the first 40
    formulas of the mix renamed v -> v + 64 (tests/test_dp_batch.py proves that
    the kernel takes every one), exact against the oracle with the record."""
    fs = R.sparse_mix()
    got = eliminate_batch(fs, record=True)
    assert len(got) == 40
    for f, r in zip(fs, got):
        _same(r, _want(f), f)                              # every one on the batch path


def test_slot_order_and_collisions():
    fs = [R.SLOT, R.SLOT37, R.COLLIDE0, R.COLLIDE1]
    got = eliminate_batch(fs, record=True)
    assert (got[0]["result"], got[0]["vars"]) == (1, [1, 2, 9])
    for f, r, path in zip(fs, got, ("batch", "batch", "single", "single")):
        _same(r, _want(f), f, path=path)
        _same_single(r, f, f)
    raw = _c_call(fs, 8, rec_lit_cap=256, rec_clause_cap=256)
    assert raw["res"].tolist()[2:] == [UNFIT, UNFIT] and raw["res"].tolist()[:2] == [1, 1]
    for b in (2, 3):   # COLLIDE1 completed a step before it collided: nothing of it is reported
        assert raw["steps"][b] == 0 and not raw["tr"][b].any() and not raw["sc"][b].any()
        assert (raw["rso"][b] == raw["rso"][b, 0]).all()


def test_wave_and_chunk_boundaries():
    names = list(R.WAVE_ROWS)
    fs = [R.WAVE_ROWS[k] for k in names] + [R.D32]
    got = eliminate_batch(fs, record=True)
    for k, f, r in zip(names + ["d32"], fs, got):
        _same(r, _want(f), k, path="single" if k == "d32" else "batch")
    raw = _c_call(fs, 4)
    assert raw["res"][-1] == UNFIT and (raw["res"][:-1] != UNFIT).all()


def test_workgroup_reuse(mix):
    """Two workgroups take all 200 formulas, large and small ones, UNSAT and SAT
    ones alternating: whatever a formula leaves in LDS (lists, event words, the
    live mask, the id map) must not reach the next one."""
    fs, want, got = mix
    work = [len(fs[b]) + sum(want[b]["step_clauses"]) for b in range(200)]
    unsat = sorted((b for b in range(200) if want[b]["result"] == 0), key=lambda b: -work[b])
    sat = sorted((b for b in range(200) if want[b]["result"] == 1), key=lambda b: work[b])
    order = [x for pair in zip(unsat, sat) for x in pair]
    order += [b for b in range(200) if b not in set(order)]
    assert sorted(order) == list(range(200))
    debug_batch(2, 0)
    try:
        again = eliminate_batch([fs[b] for b in order], record=True)
    finally:
        debug_batch(0, 0)
    for k, b in enumerate(order):
        assert again[k] == got[b], (k, b, fs[b])


def _c_call(formulas, step_cap, rec_lit_cap=None, rec_clause_cap=None, step_limit=0, clause_limit=0):
    """satmi_dp_batch_host with guard words after every output array."""
    L = _capi.load()
    cb = cnf.pack(formulas)
    B = cb.num_instances
    P32, P64 = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int64)
    out = {"res": np.full(B + GUARD, G32, np.int32), "steps": np.full(B + GUARD, G32, np.int32),
           "tr": np.full(B * step_cap + GUARD, G32, np.int32), "sc": np.full(B * step_cap + GUARD, G64, np.int64)}
    sizes = {"res": B, "steps": B, "tr": B * step_cap, "sc": B * step_cap}
    record = rec_lit_cap is not None
    if record:
        out.update(rl=np.full(rec_lit_cap + GUARD, G32, np.int32), rco=np.full(rec_clause_cap + GUARD, G64, np.int64),
                   rso=np.full(B * (step_cap + 1) + GUARD, G64, np.int64))
        sizes.update(rl=rec_lit_cap, rco=rec_clause_cap, rso=B * (step_cap + 1))
    p = {k: v.ctypes.data_as(P32 if v.dtype == np.int32 else P64) for k, v in out.items()}
    rc = L.satmi_dp_batch_host(B, cb.inst_clause_begin.ctypes.data_as(P32), cb.clause_lit_begin.ctypes.data_as(P32),
                               cb.lits.ctypes.data_as(P32), step_limit, clause_limit, p["res"], p["steps"], p["tr"],
                               p["sc"], step_cap, p.get("rl"), rec_lit_cap or 0, p.get("rco"), rec_clause_cap or 0,
                               p.get("rso"))
    _capi.check(rc, "satmi_dp_batch_host")
    for k, v in out.items():   # nothing written past an array's capacity
        assert (v[sizes[k]:] == (G32 if v.dtype == np.int32 else G64)).all(), k
    r = {k: v[:sizes[k]] for k, v in out.items()}
    r["tr"], r["sc"] = r["tr"].reshape(B, step_cap), r["sc"].reshape(B, step_cap)
    if record:
        r["rso"] = r["rso"].reshape(B, step_cap + 1)
    return r


def _recorded(r, b, k):
    rso, rco, rl = r["rso"], r["rco"], r["rl"]
    return [rl[rco[c]:rco[c + 1]].tolist() for c in range(rso[b, k], rso[b, k + 1])]


def test_capacity_and_fallback():
    fs = R.capacity_rows()
    cap = R.SMALL_CAP
    want = [_want(f) for f in fs]
    over = [len(f) > cap or max(w["step_clauses"], default=0) > cap for f, w in zip(fs, want)]
    assert any(over) and not all(over)
    free = eliminate_batch(fs, record=True)
    debug_batch(0, cap)
    try:
        raw = _c_call(fs, 32, rec_lit_cap=1 << 18, rec_clause_cap=1 << 16)
        via = eliminate_batch(fs, record=True)
    finally:
        debug_batch(0, 0)
    assert [x == UNFIT for x in raw["res"]] == over
    for b, w in enumerate(want):
        if over[b]:
            assert raw["steps"][b] == 0 and not raw["tr"][b].any() and not raw["sc"][b].any()
            assert (raw["rso"][b] == raw["rso"][b, 0]).all()      # nothing recorded
        else:
            n, done = w["steps"], len(w["clauses"])
            assert (int(raw["res"][b]), int(raw["steps"][b])) == (w["result"], n)
            assert raw["tr"][b, :n].tolist() == w["vars"] and not raw["tr"][b, n:].any()
            assert raw["sc"][b, :done].tolist() == w["step_clauses"] and not raw["sc"][b, done:].any()
            assert [_recorded(raw, b, k) for k in range(done)] == w["clauses"]
    assert [x["path"] for x in via] == ["single" if o else "batch" for o in over]
    assert [x["path"] for x in free] == ["batch"] * len(fs)
    for x, y, w in zip(via, free, want):
        assert {k: v for k, v in x.items() if k != "path"} == {k: v for k, v in y.items() if k != "path"}
        _same(y, w)


def test_limits(mix):
    fs = R.mix()[:60]
    for sl in (1, 3):
        got = eliminate_batch(fs, step_limit=sl, record=True)
        for f, r in zip(fs, got):
            _same(r, _want(f, step_limit=sl), (sl, f))
        assert any(r["result"] == -1 for r in got)
    f, lo, hi = R.limit_rows(R.mix())
    for lim, verdict in ((lo, -1), (hi, 0)):   # the limit trips before / after the empty resolvent of one step
        got = eliminate_batch([f, fs[0], f], clause_limit=lim, record=True)
        assert got[0]["result"] == verdict and got[0] == got[2]
        _same(got[0], _want(f, clause_limit=lim), (lim, f))
        _same(got[1], _want(fs[0], clause_limit=lim), (lim, fs[0]))
        _same_single(got[0], f, (lim, f), clause_limit=lim)
    # fewer rows than steps: the rows are truncated, the step count is exact
    _, want, _ = mix
    long = [b for b in range(200) if want[b]["steps"] >= 4][:8]
    assert long
    raw = _c_call([R.mix()[b] for b in long], 2, rec_lit_cap=1 << 14, rec_clause_cap=1 << 12)
    for k, b in enumerate(long):
        w = want[b]
        assert (int(raw["res"][k]), int(raw["steps"][k])) == (w["result"], w["steps"])
        assert raw["tr"][k].tolist() == w["vars"][:2] and raw["sc"][k].tolist() == (w["step_clauses"] + [0, 0])[:2]
        assert [_recorded(raw, k, s) for s in range(2)] == (w["clauses"] + [[], []])[:2]
    none = _c_call([R.mix()[b] for b in long], 0)
    assert none["steps"].tolist() == [want[b]["steps"] for b in long]


def test_bench_set():
    batch = cnf.uniform_ksat(16, 16, 96, 3, seed=7002)
    fs = [batch.instance(b) for b in range(16)]
    got = eliminate_batch(batch, record=True)
    assert [r["path"] for r in got] == ["batch"] * 16      # none is UNFIT at the default capacity
    for b, f in enumerate(fs):
        _same(got[b], _want(f), b)
        _same_single(got[b], f, b)
    assert max(max(r["step_clauses"]) for r in got) == 898


def test_record_truncation_and_guards(mix):
    fs, want, got = mix
    pick = [b for b in range(200) if len(want[b]["clauses"]) >= 2 and len(want[b]["clauses"][1]) >= 2][:3]
    assert len(pick) == 3
    sub = [fs[b] for b in pick]
    whole = [c for b in pick for l in want[b]["clauses"] for c in l]
    nlits, ncl = sum(len(c) for c in whole), len(whole)
    # exactly full: every clause needs a free offset (ncl + 1 of them) and every literal a slot
    full = _c_call(sub, 16, rec_lit_cap=nlits, rec_clause_cap=ncl + 1)
    flat = [c for k in range(3) for s in range(len(want[pick[k]]["clauses"])) for c in _recorded(full, k, s)]
    assert flat == whole
    # one short of each
    t = _c_call(sub, 16, rec_lit_cap=nlits, rec_clause_cap=ncl)
    assert int(t["rso"][-1, -1]) == ncl - 1
    flat = [t["rl"][t["rco"][c]:t["rco"][c + 1]].tolist() for c in range(ncl - 1)]
    assert flat == whole[:-1]
    t = _c_call(sub, 16, rec_lit_cap=nlits - 1, rec_clause_cap=ncl + 1)
    assert int(t["rso"][-1, -1]) == ncl and int(t["rco"][ncl]) == nlits - 1      # the last literal is dropped
    for r in (full, t):
        for k, b in enumerate(pick):
            assert (int(r["res"][k]), int(r["steps"][k])) == (want[b]["result"], want[b]["steps"])
    _c_call(sub, 16, rec_lit_cap=0, rec_clause_cap=0)


def test_four_threads(mix):
    fs, want, got = mix
    out = [None] * 4

    def run(k):
        out[k] = eliminate_batch(fs, record=True)

    th = [threading.Thread(target=run, args=(k,)) for k in range(4)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    for k in range(4):
        assert out[k] == got, k
